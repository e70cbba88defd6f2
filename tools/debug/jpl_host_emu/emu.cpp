// The JPEG Lossless kernels (csrc/jpeg_lossless_kernels.hip) on the host, for checks that need no GPU: the shim of
// ../rle_host_emu stands in for the HIP runtime (a std::thread per GPU thread, the blocks of a launch one after another),
// so the kernel source compiles unchanged with g++ and runs under AddressSanitizer / UBSan.  drive.py feeds it rasters and
// files of tests/jpeg_lossless_model.py and compares.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I../rle_host_emu -x c++ emu.cpp -o emu -lpthread && python drive.py
// Slow (a thread per lane): small shapes.  It checks the algorithm and the bounds, not the timing.
#include "emu_common.h"
#include "../../../2023-compact-image-compression_amd/csrc/jpeg_lossless_kernels.hip"
using namespace cct;
// encode: e src_bits precision rows cols n restart_rows predictor in.bin out.bin   (predictor 1 .. 7, 0: the frame's best;
//         out.bin: per frame size, status, Ss and the file)
// decode: d rows cols out_bits nslots job.bin files.bin out.bin   (job.bin: per frame 13 uint32 -- src, len, slot, ss, pt, P, ri,
//         nval, then 16 + 20 bytes BITS / HUFFVAL)
int main(int argc, char **argv)
{
	if (argv[1][0] == 'e') {
		JplEncArgs a{};
		a.src_bits = atoi(argv[2]); a.precision = atoi(argv[3]); a.rows = atoi(argv[4]); a.cols = atoi(argv[5]); a.n = atoi(argv[6]);
		const uint32_t rr = atoi(argv[7]);
		a.rpi = rr ? rr : a.rows; a.n_int = (a.rows + a.rpi - 1) / a.rpi; a.restart = rr > 0;
		a.predictor = atoi(argv[8]); a.ncand = a.predictor ? 1 : JPL_NCAND;
		auto in = rd(argv[9]);
		const size_t N = (size_t)a.rows * a.cols, isz = (size_t)std::min(a.rpi, a.rows) * a.cols;
		const size_t bound = JPL_HDR_MAX + a.n_int * (2 * ((31 * isz + 7) / 8) + 2), stride = (bound + 3) & ~(size_t)3;
		std::vector<uint32_t> status(a.n), sel(a.n), ints((size_t)a.n * a.n_int * 3), sizes(a.n);
		std::vector<uint8_t> hist((size_t)a.n * a.ncand * 17 * 4 + GUARD, 0xEE), codes((size_t)a.n * a.ncand * sizeof(JplCode) + GUARD, 0xEE);
		memset(hist.data(), 0, hist.size() - GUARD);
		std::vector<uint8_t> bitbuf(a.n * N * 4 + GUARD, 0xEE), out(a.n * stride + GUARD, 0xEE);
		a.images = in.data(); a.hist = (uint32_t *)hist.data(); a.status = status.data(); a.sel = sel.data(); a.codes = (JplCode *)codes.data(); a.bitbuf = (uint32_t *)bitbuf.data();
		a.ibytes = ints.data(); a.iff = a.ibytes + (size_t)a.n * a.n_int; a.ioff = a.iff + (size_t)a.n * a.n_int;
		a.out = out.data(); a.out_stride = stride; a.out_sizes = sizes.data();
		if (launch_jpl_encode(a, nullptr) != hipSuccess) { printf("launch refused\n"); return 2; }
		std::ofstream f(argv[10], std::ios::binary);
		for (uint32_t i = 0; i < a.n; i++) {
			uint32_t s = sizes[i], stt = status[i];
			if (s > bound) { printf("size beyond bound\n"); return 2; }
			f.write((char *)&s, 4); f.write((char *)&stt, 4); f.write((char *)&sel[i], 4); f.write((char *)out.data() + i * stride, s);
		}
		if (!guard_ok(bitbuf, a.n * N * 4) || !guard_ok(out, a.n * stride) || !guard_ok(hist, (size_t)a.n * a.ncand * 17 * 4) ||
		    !guard_ok(codes, (size_t)a.n * a.ncand * sizeof(JplCode))) { printf("guard hit\n"); return 2; }
	} else {
		JplDecArgs a{};
		a.rows = atoi(argv[2]); a.cols = atoi(argv[3]); a.out_bits = atoi(argv[4]);
		const size_t nslots = atoi(argv[5]), N = (size_t)a.rows * a.cols, px = a.out_bits / 8;
		auto job = rd(argv[6]); auto files = rd(argv[7]);
		const size_t rec = 8 * 4 + 36, nf = job.size() / rec;
		std::vector<JplFrame> frames(nf);
		std::vector<uint32_t> int_frame;
		uint64_t nsub = 0;
		for (size_t i = 0; i < nf; i++) {
			const uint32_t *w = (const uint32_t *)(job.data() + i * rec);
			const uint8_t *tb = job.data() + i * rec + 32;
			JplFrame f{};
			f.src = w[0]; f.len = w[1]; f.slot = w[2]; f.ss = w[3]; f.pt = w[4]; f.init = 1u << (w[5] - w[4] - 1);
			f.rpi = w[6] ? w[6] / a.cols : a.rows; f.n_int = (a.rows + f.rpi - 1) / f.rpi;
			f.int0 = (uint32_t)int_frame.size(); f.sub0 = (uint32_t)nsub;
			nsub += (uint64_t)f.len * 8 / JPL_SUB + f.n_int;
			int code = 0, k = 0;
			f.maxcode[0] = -1;
			for (int l = 1; l <= 16; l++) { const int b = tb[l - 1]; f.delta[l] = k - code; code += b; k += b; f.maxcode[l] = b ? code - 1 : -1; code <<= 1; }
			memcpy(f.huffval, tb + 16, w[7]);
			a.any_generic |= f.ss != 1;
			int_frame.insert(int_frame.end(), f.n_int, (uint32_t)i);
			frames[i] = f;
		}
		const size_t ni = int_frame.size(), fbytes = files.size();
		files.resize(fbytes + GUARD, 0xEE);
		std::vector<uint8_t> ubuf(fbytes + GUARD, 0xEE), img(nslots * N * px + GUARD, 0xEE), diff(nslots * N * 2 + GUARD, 0xEE);
		std::vector<uint8_t> istart((ni + nf) * 4 + GUARD, 0xEE), sub(nsub * 12 + GUARD, 0xEE);
		std::vector<uint32_t> status(nf);
		a.files = files.data(); a.frames = frames.data(); a.nframes = (uint32_t)nf; a.int_frame = int_frame.data(); a.total_int = (uint32_t)ni;
		a.ubuf = ubuf.data(); a.istart = (uint32_t *)istart.data();
		a.sub_start = (uint32_t *)sub.data(); a.sub_land = a.sub_start + nsub; a.sub_cnt = a.sub_land + nsub;
		a.diff = (uint16_t *)diff.data(); a.status = status.data(); a.images = img.data();
		launch_jpl_decode(a, nullptr);
		std::ofstream f(argv[8], std::ios::binary);
		f.write((char *)status.data(), nf * 4); f.write((char *)img.data(), nslots * N * px);
		if (!guard_ok(ubuf, fbytes) || !guard_ok(img, nslots * N * px) || !guard_ok(diff, nslots * N * 2) || !guard_ok(istart, (ni + nf) * 4) ||
		    !guard_ok(sub, nsub * 12)) { printf("guard hit\n"); return 2; }
	}
	return 0;
}
