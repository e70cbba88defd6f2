// The JPEG 2000 kernels (csrc/jpeg2000_kernels.hip) on the host, for checks that need no GPU: the shim of ../rle_host_emu
// stands in for the HIP runtime (a std::thread per GPU thread, the blocks of a launch one after another), so the kernel
// source compiles unchanged with g++ and runs under AddressSanitizer / UBSan.  drive.py feeds it the rasters of
// tests/jpeg2000_model.py and compares the files.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I../rle_host_emu -x c++ emu.cpp -o emu -lpthread && python drive.py
// Slow (a thread per lane): small shapes.  It checks the algorithm and the bounds, not the timing.  Every device buffer is
// followed by a guard that must come back untouched; `slab_div` > 1 shrinks the slabs to exercise the capacity check.
#include "emu_common.h"
#include "../../../2023-compact-image-compression_amd/csrc/jpeg2000_kernels.hip"
using namespace cct;
// emu src_bits precision shift levels codeblock jp2 rows cols n slab_div in.bin out.bin
int main(int argc, char **argv)
{
	if (argc != 13) { printf("usage\n"); return 2; }
	J2kArgs a{};
	a.src_bits = atoi(argv[1]); a.precision = atoi(argv[2]); a.shift = atoi(argv[3]); a.levels = atoi(argv[4]); a.codeblock = atoi(argv[5]);
	const bool jp2 = atoi(argv[6]);
	a.rows = atoi(argv[7]); a.cols = atoi(argv[8]); a.n = atoi(argv[9]);
	const uint32_t slab_div = atoi(argv[10]);
	auto in = rd(argv[11]);
	J2kLayout L;
	j2k_layout(a.rows, a.cols, a.precision, a.levels, a.codeblock, L);
	if (slab_div > 1) {
		L.slab_bytes = 0;
		for (auto &b : L.blocks) { b.slab_cap = b.slab_cap / slab_div; b.slab_off = (uint32_t)L.slab_bytes; L.slab_bytes += b.slab_cap; }
	}
	const size_t N = (size_t)a.rows * a.cols, stride = (L.bound + 3) & ~(size_t)3, nb = L.blocks.size();
	std::vector<uint8_t> pa(a.n * N * 4 + GUARD, 0xEE), pb(a.n * N * 4 + GUARD, 0xEE), slabs(a.n * L.slab_bytes + GUARD, 0xEE);
	std::vector<uint8_t> cbout(a.n * nb * sizeof(J2kBlockOut) + GUARD, 0xEE), tt((size_t)a.n * 6 * L.tt_nodes + GUARD, 0xEE), out(a.n * stride + GUARD, 0xEE);
	std::vector<uint32_t> status(a.n), sizes(a.n);
	a.images = in.data(); a.plane_a = (int32_t *)pa.data(); a.plane_b = (int32_t *)pb.data();
	a.blocks = L.blocks.data(); a.nblocks = (uint32_t)nb; a.bands = L.bands.data(); a.nbands = (uint32_t)L.bands.size();
	a.slabs = slabs.data(); a.slab_stride = L.slab_bytes; a.cbout = (J2kBlockOut *)cbout.data(); a.tt = tt.data(); a.tt_nodes = L.tt_nodes;
	a.status = status.data(); a.out = out.data(); a.out_stride = stride; a.out_sizes = sizes.data();
	a.hdr_len = j2k_headers(a.rows, a.cols, a.precision, a.levels, a.codeblock, jp2, a.hdr, &a.psot_at, &a.jp2c_at);
	a.stages = 7;
	launch_j2k_encode(a, nullptr);
	std::ofstream f(argv[12], std::ios::binary);
	for (uint32_t i = 0; i < a.n; i++) {
		uint32_t s = sizes[i], stt = status[i];
		if (s > L.bound) { printf("size beyond bound\n"); return 2; }
		f.write((char *)&s, 4); f.write((char *)&stt, 4); f.write((char *)out.data() + i * stride, s);
	}
	if (!guard_ok(pa, a.n * N * 4) || !guard_ok(pb, a.n * N * 4) || !guard_ok(slabs, a.n * L.slab_bytes) || !guard_ok(cbout, a.n * nb * sizeof(J2kBlockOut)) ||
	    !guard_ok(tt, (size_t)a.n * 6 * L.tt_nodes) || !guard_ok(out, a.n * stride)) { printf("guard hit\n"); return 2; }
	return 0;
}
