// The INFLATE kernel (csrc/inflate_kernels.hip) and the PNG reader kernels (csrc/png_read_kernels.hip) on the host, for checks
// that need no GPU: the shim of ../rle_host_emu stands in for the HIP runtime (a std::thread per GPU thread, the blocks of a
// launch one after another), so both kernel files compile with g++ and run under AddressSanitizer / UBSan.  drive.py feeds it
// the hand-built, walk-edge, damaged and .cct-entrance streams and the PNG files of tests/, judged by CPython's zlib.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined,bounds -fno-sanitize-recover=undefined -I../rle_host_emu -x c++ emu.cpp -o emu -lpthread && python drive.py
// What a GPU run cannot show and this one does:
//   * the LDS of a launch is a heap block of exactly the launch's bytes (sizeof(InfShared<G>), waves * UF_WAVE_LDS);
//   * the kernel file's CCT_INF_LDS_GAP puts 64 bytes behind every array of InfShared and CanonLds.  They are filled with a
//     pattern and poisoned (their 8-byte granules) before a launch, and the pattern is checked after it: an index one past an
//     array, which on the device lands in the neighbouring member and usually changes nothing, is a report here.  With
//     -fsanitize=bounds an index into a member array is checked against the declared extent as well;
//   * the input is allocated at exactly the bytes the library uploads (cct_zlib_decompress_batch, png_read_pass: api.cpp), every
//     output slot at exactly its stride and in an allocation of its own (a stream per launch, the batch's input whole), so a
//     read past the upload or a 16-byte flush past a slot is the sanitizer's to find.  That leaves blockIdx.x at 0, so some
//     batches run as one grid as well (inflate_grid below).
// The PNG chunk table comes from drive.py (png_walk, written after api.cpp's png_walk_file rule by rule), not from the library's
// own walker: that one lives in api.cpp, which does not compile without the HIP runtime.  The parser of tests/png_model.py takes
// whole files only, and the damaged ones are the point here.  ll_tab and d_tab have no gap between them: cl_sequence lays its
// ranking arrays over both as one stretch (2 * CL_WINX words, asserted in the kernel file to fit the two together).
// Slow (a thread per lane): streams of a few KiB, a few larger ones.  It checks the algorithm and the bounds, not the timing.
#include "emu_common.h"
#include <sanitizer/asan_interface.h>

constexpr int GAP = 64;
constexpr uint8_t GAP_FILL = 0xA5;
static uint8_t *g_dyn_lds;
static void (*g_lds_before)(uint8_t *), (*g_lds_after)(uint8_t *);
#define CCT_INF_DYNAMIC_LDS(name) uint8_t *name = g_dyn_lds
#define CCT_PNG_DYNAMIC_LDS(name) uint8_t *name = g_dyn_lds
#define CCT_INF_LDS_GAP(after) uint8_t gap_##after[GAP];
static void lds_begin(size_t bytes)
{
	if (posix_memalign((void **)&g_dyn_lds, 16, bytes ? bytes : 16)) abort();
	memset(g_dyn_lds, 0xEE, bytes);  // LDS is not cleared between workgroups
	if (g_lds_before) g_lds_before(g_dyn_lds);
}
static void lds_end()
{
	if (g_lds_after) g_lds_after(g_dyn_lds);
	free(g_dyn_lds);
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) (lds_begin(sh), emu_launch(k, g, b, __VA_ARGS__), lds_end())

#include "../../../2023-compact-image-compression_amd/csrc/inflate_kernels.hip"
#include "../../../2023-compact-image-compression_amd/csrc/png_read_kernels.hip"
using namespace cct;

// ---- the gaps of InfShared ----
struct GapAt { const char *name; size_t off; };
#define GAP_OF(S, m) GapAt{#m, offsetof(S, gap_##m)}
#define CANON_GAPS(S, c) GapAt{#c ".lim", offsetof(S, c) + offsetof(CanonLds, gap_lim)}, GapAt{#c ".adj", offsetof(S, c) + offsetof(CanonLds, gap_adj)}, \
	GapAt{#c ".offs", offsetof(S, c) + offsetof(CanonLds, gap_offs)}
template <class G>
static const std::vector<GapAt> &gaps()
{
	using S = InfShared<G>;
	static const std::vector<GapAt> g = {GAP_OF(S, ring), GAP_OF(S, inbuf), GAP_OF(S, d_tab), CANON_GAPS(S, ll_canon), CANON_GAPS(S, d_canon),
	                                     GAP_OF(S, ll_sent), GAP_OF(S, d_sent), GAP_OF(S, chunkcnt), GAP_OF(S, cnt), GAP_OF(S, cl_tab), GAP_OF(S, lens),
	                                     GAP_OF(S, mlist), GAP_OF(S, lbase), GAP_OF(S, dbase), GAP_OF(S, lext), GAP_OF(S, dext), GAP_OF(S, land),
	                                     GAP_OF(S, wsum_b), GAP_OF(S, wsum_m), GAP_OF(S, wred), GAP_OF(S, rres)};
	return g;
}
// 20 arrays of InfShared (ll_tab and d_tab count as one: cl_sequence uses them as one stretch) and three in each of its two
// CanonLds: 25 gaps
static_assert(sizeof(InfShared<Geo<512>>) >= 139808 + 25 * GAP && sizeof(InfShared<Geo<256>>) >= 122336 + 25 * GAP, "the gaps are in");
template <class G>
static void gaps_arm(uint8_t *lds)
{
	for (const GapAt &g : gaps<G>()) {
		memset(lds + g.off, GAP_FILL, GAP);
		uint8_t *a = (uint8_t *)(((uintptr_t)(lds + g.off) + 7) & ~(uintptr_t)7), *b = (uint8_t *)((uintptr_t)(lds + g.off + GAP) & ~(uintptr_t)7);
		ASAN_POISON_MEMORY_REGION(a, b - a);
	}
}
template <class G>
static void gaps_check(uint8_t *lds)
{
	ASAN_UNPOISON_MEMORY_REGION(lds, sizeof(InfShared<G>));
	for (const GapAt &g : gaps<G>())
		for (int k = 0; k < GAP; k++)
			if (lds[g.off + k] != GAP_FILL) {
				printf("LDS gap behind %s damaged at byte %d (lanes %d)\n", g.name, k, G::NT);
				fflush(stdout);
				_Exit(3);
			}
}
static void inflate_hooks(int lanes)
{
	g_lds_before = lanes >= 512 ? gaps_arm<Geo<512>> : gaps_arm<Geo<256>>;
	g_lds_after = lanes >= 512 ? gaps_check<Geo<512>> : gaps_check<Geo<256>>;
}
static void no_hooks() { g_lds_before = g_lds_after = nullptr; }

static void *exact(size_t align, size_t bytes, int fill)
{
	void *p;
	if (posix_memalign(&p, align, bytes ? bytes : 1)) abort();
	memset(p, fill, bytes);
	return p;
}
// the last 48 bytes of a padded stream buffer (pad + 16 bytes) are zero: api.cpp zero_read_ahead
static void zero_read_ahead(uint8_t *p, size_t pad) { memset(p + (pad > 32 ? pad - 32 : 0), 0, pad > 32 ? 48 : pad + 16); }

// every stream in a launch of its own, its output slot an allocation of exactly out_stride bytes; the input is the batch's
static void inflate_each(const uint8_t *in, size_t in_total, const uint64_t *offs, int skip, uint32_t n, size_t out_stride, int lanes,
                         std::vector<uint8_t *> &slots, std::vector<uint32_t> &sizes, std::vector<uint32_t> &status)
{
	inflate_hooks(lanes);
	slots.resize(n); sizes.assign(n, 0xEEEEEEEEu); status.assign(n, 0xEEEEEEEEu);
	for (uint32_t s = 0; s < n; s++) {
		slots[s] = (uint8_t *)exact(16, out_stride, 0xEE);
		InflateArgs a{};
		a.in = in; a.in_total = in_total; a.offsets = offs + s; a.skip = skip;
		a.out = slots[s]; a.out_stride = out_stride; a.out_sizes = &sizes[s]; a.status = &status[s];
		if (launch_inflate(a, 1, nullptr, lanes) != hipSuccess) abort();
	}
	no_hooks();
}
// The batch as the library launches it: one grid of n workgroups, the slots side by side in one allocation of n * out_stride
// bytes.  A flush past a slot that is not the last lands in its neighbour and is the comparison's to find, not the sanitizer's;
// what this adds is the kernel's own indexing by blockIdx.x (offsets[s], s * out_stride, out_sizes[s], status[s]).
static void inflate_grid(const uint8_t *in, size_t in_total, const uint64_t *offs, int skip, uint32_t n, size_t out_stride, int lanes,
                         std::vector<uint8_t *> &slots, std::vector<uint32_t> &sizes, std::vector<uint32_t> &status)
{
	inflate_hooks(lanes);
	slots.resize(n); sizes.assign(n, 0xEEEEEEEEu); status.assign(n, 0xEEEEEEEEu);
	uint8_t *base = (uint8_t *)exact(16, n * out_stride, 0xEE);
	for (uint32_t s = 0; s < n; s++) slots[s] = base + s * out_stride;
	InflateArgs a{};
	a.in = in; a.in_total = in_total; a.offsets = offs; a.skip = skip;
	a.out = base; a.out_stride = out_stride; a.out_sizes = sizes.data(); a.status = status.data();
	if (launch_inflate(a, (int)n, nullptr, lanes) != hipSuccess) abort();
	no_hooks();
}

static std::vector<uint64_t> u64s(const uint8_t *p, size_t n) { std::vector<uint64_t> v(n); memcpy(v.data(), p, n * 8); return v; }

// emu <lanes> in.bin out_stride out.bin [skip [each|grid]]      (each: inflate_each, the default; grid: inflate_grid)
//   in.bin: u32 n, n + 1 u64 offsets, the streams back to back (stream i = bytes offsets[i] + skip .. offsets[i + 1]);
//   out.bin: per stream u32 status (CCT_ST_* bits), u32 size, and its bytes when the status is 0.  skip 0: the upload of
//   cct_zlib_decompress_batch (read-ahead zeroed); skip > 0: that of the .cct decode (bytes behind the archive left as they are)
static int main_inflate(int argc, char **argv)
{
	const int lanes = atoi(argv[1]), skip = argc > 5 ? atoi(argv[5]) : 0;
	const bool grid = argc > 6 && !strcmp(argv[6], "grid");
	const size_t out_stride = atoll(argv[3]);
	auto d = rd(argv[2]);
	uint32_t n;
	memcpy(&n, d.data(), 4);
	auto offs = u64s(d.data() + 4, n + 1);
	const size_t blob_at = 4 + (n + 1) * 8, abytes = d.size() - blob_at, apad = (abytes + 31) & ~(size_t)15;
	if (offs[0] != 0 || offs[n] != abytes || (lanes != 256 && lanes != 512) || out_stride == 0 || (out_stride & 15)) { printf("bad arguments\n"); return 2; }
	uint8_t *in = (uint8_t *)exact(256, apad + 16, 0xEE);
	if (!skip) zero_read_ahead(in, apad);
	memcpy(in, d.data() + blob_at, abytes);
	std::vector<uint8_t *> slots;
	std::vector<uint32_t> sizes, status;
	(grid ? inflate_grid : inflate_each)(in, apad, offs.data(), skip, n, out_stride, lanes, slots, sizes, status);
	std::ofstream f(argv[4], std::ios::binary);
	for (uint32_t s = 0; s < n; s++) {
		f.write((char *)&status[s], 4); f.write((char *)&sizes[s], 4);
		if (status[s] == 0) {
			if (sizes[s] > out_stride) { printf("stream %u: %u bytes in a slot of %zu\n", s, sizes[s], out_stride); return 3; }
			f.write((char *)slots[s], sizes[s]);
		}
		if (!grid) free(slots[s]);
	}
	if (grid && n) free(slots[0]);
	free(in);
	return 0;
}

// emu png <lanes> <waves> rows cols shift in.bin out.bin: unpack -> inflate -> unfilter as png_read_pass (api.cpp) chains them
//   in.bin: u32 nfiles, u32 nchunks, u64 file bytes, nfiles + 1 u64 stream offsets, nfiles u32 status words (PNG_ST_SKIP for a
//   file the walk refused), nfiles bytes-per-sample, nchunks PngChunk records, the files back to back
//   out.bin: nfiles x (u32 file status, u32 zlib status, u32 inflated size), then nfiles rasters of rows x cols uint16
static int main_png(int argc, char **argv)
{
	if (argc != 9) { printf("usage\n"); return 2; }
	const int lanes = atoi(argv[2]), waves = atoi(argv[3]), rows = atoi(argv[4]), cols = atoi(argv[5]), shift = atoi(argv[6]);
	auto d = rd(argv[7]);
	uint32_t nf, nch;
	uint64_t abytes;
	memcpy(&nf, d.data(), 4); memcpy(&nch, d.data() + 4, 4); memcpy(&abytes, d.data() + 8, 8);
	size_t p = 16;
	auto zoffs = u64s(d.data() + p, nf + 1); p += (nf + 1) * 8;
	std::vector<uint32_t> fst(nf); memcpy(fst.data(), d.data() + p, nf * 4); p += nf * 4;
	std::vector<uint8_t> bpp(d.begin() + p, d.begin() + p + nf); p += nf;
	PngChunk *tab = (PngChunk *)exact(8, nch * sizeof(PngChunk), 0);
	memcpy(tab, d.data() + p, nch * sizeof(PngChunk)); p += nch * sizeof(PngChunk);
	if (d.size() - p != abytes) { printf("bad input file\n"); return 2; }
	int max_bpp = 0;
	for (uint32_t i = 0; i < nf; i++) if (!(fst[i] & PNG_ST_SKIP)) max_bpp = std::max(max_bpp, (int)bpp[i]);
	const size_t stride = (((size_t)rows * (1 + (size_t)cols * max_bpp) + 15) & ~(size_t)15) + 16;
	const size_t zoff = zoffs[nf], zpad = (zoff + 31) & ~(size_t)15, img = (size_t)rows * cols;
	uint8_t *files = (uint8_t *)exact(256, abytes + 16, 0xEE);  // 256-byte aligned, 16 bytes of padding: what the chunk reads may touch
	memcpy(files, d.data() + p, abytes);
	uint8_t *z = (uint8_t *)exact(256, zpad + 16, 0xEE);
	zero_read_ahead(z, zpad);
	PngUnpackArgs ua{};
	ua.files = files; ua.chunks = tab; ua.streams = z; ua.status = fst.data();
	if (launch_png_unpack(ua, nch, nullptr) != hipSuccess) abort();
	std::vector<uint8_t *> slots;
	std::vector<uint32_t> osz, zst;
	inflate_each(z, zpad, zoffs.data(), 0, nf, stride, lanes, slots, osz, zst);
	std::vector<uint16_t *> out(nf);
	for (uint32_t i = 0; i < nf; i++) {  // a file per launch: its rows and its raster are allocations of their own
		out[i] = (uint16_t *)exact(16, img * 2, 0xEE);
		PngUnfilterArgs fa{};
		fa.rows = slots[i]; fa.rows_stride = stride; fa.row_sizes = &osz[i]; fa.zstatus = &zst[i]; fa.status = &fst[i]; fa.bpp = &bpp[i];
		fa.nrows = rows; fa.cols = cols; fa.shift = shift; fa.images = out[i];
		if (launch_png_unfilter(fa, 1, waves, nullptr) != hipSuccess) abort();
	}
	std::ofstream f(argv[8], std::ios::binary);
	for (uint32_t i = 0; i < nf; i++) { f.write((char *)&fst[i], 4); f.write((char *)&zst[i], 4); f.write((char *)&osz[i], 4); }
	for (uint32_t i = 0; i < nf; i++) { f.write((char *)out[i], img * 2); free(out[i]); free(slots[i]); }
	free(z); free(files); free(tab);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "png")) return main_png(argc, argv);
	if (argc < 5 || argc > 7) { printf("usage: emu <lanes> in.bin out_stride out.bin [skip [each|grid]] | emu png <lanes> <waves> rows cols shift in.bin out.bin\n"); return 2; }
	return main_inflate(argc, argv);
}
