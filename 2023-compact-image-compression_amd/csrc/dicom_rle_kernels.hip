// DICOM RLE Lossless (PS3.5 Annex G, transfer syntax 1.2.840.10008.1.2.5) for one sample per pixel of 8 or 16 bits: the
// device side of cct_dicom_rle_encode_batch / cct_dicom_rle_decode_batch (api_dicom_rle.cpp).  tests/dicom_rle_model.py is the
// CPU restatement of both directions.
//
// ENCODE.  A frame is a 64-byte header and one PackBits-coded segment per byte plane (most significant first), every row of
// the plane coded by itself.  The encoder rule works on maximal groups of equal bytes: a group of one is a literal, a longer
// group a run that leaves as (129, v) per full 128 bytes and (257 - r, v) / (0, v) for a remainder r >= 2 / r = 1; literals
// between runs leave in chunks of 128.  What a byte contributes follows from what lies BEFORE it plus two bytes of look-ahead:
//   run byte, index j in its group       -> the packet (2 bytes) if j % 128 == 127 or the group ends here, else nothing
//   literal byte, index k in its stretch -> itself, plus a header byte if k % 128 == 0; the byte that closes a chunk (k % 128
//                                           == 127, or a run or the row end follows) writes that header, k % 128 places back
// so one wave codes a row in a single forward sweep of 64 bytes per step: ballots give the group start and the last run byte
// before each lane, a wave scan of the contributions gives the output offsets, and nothing is staged in memory.  A 16-bit
// pixel is loaded once and both of its planes are coded from the register.  Three launches: sizes of all coded rows (one
// wave per row), one wave per slice that scans them into row offsets and writes header and pad bytes, the same sweep again
// with stores.  The second sweep re-reads a raster the first one has just pulled through the caches.
//
// DECODE.  Where a packet starts is known only once every packet before it has been read.  A segment is cut into tiles of
// RLE_TILE coded bytes; a packet is at most 129 bytes, so the first head of a tile lies at one of RLE_ENTRIES offsets:
//   1 tabulate (a workgroup per tile): every position of the tile, read as if it were a packet head, gives (next head,
//     bytes produced); pointer doubling in LDS composes these until every position has left the tile; the results for
//     the RLE_ENTRIES entry offsets go to a table: (offset into the next tile, bytes this tile produces)
//   2 chain (a workgroup per segment): the segment's table rows come into LDS 64 tiles at a time and one lane hops through
//     them: true entry offset and output index of every tile, clipped at rows * cols; a segment that ends short is flagged
//   3 expand (a workgroup per tile): the same doubling, now with the true entry marked: a marked position marks the head
//     2^r packets further on in round r, which marks exactly the heads.  A block scan of what the heads produce gives their
//     output offsets, and every output byte finds its packet by bisection in LDS and goes to its byte of the raster
//     (byte 2k+1 / 2k of pixel k for the two segments of a 16-bit frame), directly, with no plane buffer and no merge pass.
// A literal packet cut by the segment end yields what is there, a replicate header without its byte yields nothing, bytes
// behind rows * cols are ignored; rows play no part, so packets of other encoders that cross row ends decode alike.
#include "cct_internal.h"
#include "wave_device.h"
#include "../../include/compact_hip.h"

namespace cct {
namespace {

// ---- encode ---------------------------------------------------------------------------------------------------------

struct PlaneState { uint32_t group_start; int32_t last_run; uint32_t out; };

// one byte plane, 64 bytes of a row: b is the lane's byte (index i = base + lane), pb / n1 / n2 the bytes at i - 1, i + 1, i + 2
template <bool WRITE>
__device__ __forceinline__ void plane_step(uint32_t b, uint32_t pb, uint32_t n1, uint32_t n2, uint32_t base, uint32_t lane, uint32_t cols,
                                           PlaneState &s, uint8_t *dst)
{
	const uint32_t i = base + lane;
	const bool valid = i < cols;
	const bool starts = valid && (i == 0 || pb != b);
	const bool next_eq = valid && i + 1 < cols && n1 == b;
	const bool in_run = valid && (!starts || next_eq);
	const uint64_t le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);  // lanes at or below this one
	const uint64_t sb = __ballot(starts), rb = __ballot(in_run);
	const uint64_t s_upto = sb & le, r_below = rb & (le >> 1);
	const uint32_t gs = s_upto ? base + 63u - (uint32_t)__clzll((long long)s_upto) : s.group_start;
	const int32_t lr = r_below ? (int32_t)(base + 63u - (uint32_t)__clzll((long long)r_below)) : s.last_run;
	if (sb) s.group_start = base + 63u - (uint32_t)__clzll((long long)sb);
	if (rb) s.last_run = (int32_t)(base + 63u - (uint32_t)__clzll((long long)rb));
	uint32_t contrib = 0, hdr = 0, km = 0;
	bool head = false, closes = false;
	if (in_run) {
		const uint32_t jm = (i - gs) & 127u;
		if (jm == 127u || !next_eq) { contrib = 2; hdr = jm == 127u ? 129u : (jm ? 256u - jm : 0u); }  // remainder r = jm + 1
	} else if (valid) {
		km = (uint32_t)((int32_t)i - lr - 1) & 127u;
		head = km == 0;
		closes = km == 127u || i + 1 == cols || (i + 2 < cols && n1 == n2);
		contrib = head ? 2u : 1u;
	}
	uint32_t tot;
	const uint32_t off = s.out + wave_excl_scan(contrib, tot);
	if (WRITE) {
		if (in_run) { if (contrib) { dst[off] = (uint8_t)hdr; dst[off + 1] = (uint8_t)b; } }
		else if (valid) {
			const uint32_t p = off + (head ? 1u : 0u);
			dst[p] = (uint8_t)b;
			if (closes) dst[p - km - 1u] = (uint8_t)km;
		}
	}
	s.out += tot;
}

// one wave per row of one raster: both planes of a 16-bit row from one load per pixel
template <typename Px, bool WRITE>
__global__ void __launch_bounds__(256) rle_rows_kernel(const Px *images, uint64_t total_rows, uint32_t rows, uint32_t cols, uint32_t *rowinfo,
                                                       uint8_t *out, size_t out_stride)
{
	constexpr int PLANES = (int)sizeof(Px);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
	if (g >= total_rows) return;  // a whole wave; the kernel has no barrier
	const uint64_t slice = g / rows;
	const uint32_t r = (uint32_t)(g - slice * rows);
	const Px *src = images + g * cols;
	uint32_t *ri = rowinfo + slice * PLANES * rows + r;  // plane p: ri[p * rows]
	PlaneState st[PLANES];
	uint8_t *dst[PLANES];
#pragma unroll
	for (int p = 0; p < PLANES; p++) {
		st[p] = PlaneState{0u, -1, 0u};
		dst[p] = WRITE ? out + slice * out_stride + ri[(size_t)p * rows] : nullptr;
	}
	uint32_t cur = lane < cols ? (uint32_t)src[lane] : 0u, prev_last = 0;
	for (uint32_t base = 0; base < cols; base += 64) {
		const uint32_t in = base + 64u + lane;
		const uint32_t nxt = in < cols ? (uint32_t)src[in] : 0u;
		const uint32_t up = (uint32_t)__shfl_up((int)cur, 1), d1 = (uint32_t)__shfl_down((int)cur, 1), d2 = (uint32_t)__shfl_down((int)cur, 2);
		const uint32_t x0 = (uint32_t)__shfl((int)nxt, 0), x1 = (uint32_t)__shfl((int)nxt, 1);
		const uint32_t pv = lane ? up : prev_last, n1 = lane < 63 ? d1 : x0, n2 = lane < 62 ? d2 : (lane == 62 ? x0 : x1);
#pragma unroll
		for (int p = 0; p < PLANES; p++) {
			const int sh = 8 * (PLANES - 1 - p);  // plane 0 is the most significant byte
			plane_step<WRITE>((cur >> sh) & 0xFFu, (pv >> sh) & 0xFFu, (n1 >> sh) & 0xFFu, (n2 >> sh) & 0xFFu, base, lane, cols, st[p], dst[p]);
		}
		prev_last = (uint32_t)__shfl((int)cur, 63);
		cur = nxt;
	}
	if (!WRITE && lane == 0) {
#pragma unroll
		for (int p = 0; p < PLANES; p++) ri[(size_t)p * rows] = st[p].out;
	}
}

// one wave per raster: coded row lengths -> row offsets in the frame; header, pad bytes, frame size
__global__ void __launch_bounds__(64) rle_layout_kernel(uint32_t rows, int planes, uint32_t *rowinfo, uint8_t *out, size_t out_stride, uint32_t *out_sizes)
{
	const uint32_t lane = threadIdx.x;
	const size_t slice = blockIdx.x;
	uint8_t *frame = out + slice * out_stride;
	uint32_t pos = 64, seg1 = 0;
	for (int p = 0; p < planes; p++) {
		uint32_t *ri = rowinfo + (slice * planes + p) * rows;
		if (p == 1) seg1 = pos;
		for (uint32_t base = 0; base < rows; base += 64) {
			const uint32_t r = base + lane;
			const uint32_t v = r < rows ? ri[r] : 0u;
			uint32_t tot;
			const uint32_t ex = wave_excl_scan(v, tot);
			if (r < rows) ri[r] = pos + ex;
			pos += tot;
		}
		if (pos & 1u) { if (lane == 0) frame[pos] = 0; pos++; }
	}
	if (lane < 16) ((uint32_t *)frame)[lane] = lane == 0 ? (uint32_t)planes : lane == 1 ? 64u : lane == 2 ? seg1 : 0u;
	if (lane == 0) out_sizes[slice] = pos;
}

// ---- decode ---------------------------------------------------------------------------------------------------------

constexpr uint32_t T = RLE_TILE;
constexpr uint32_t LOOK = 132;            // bytes staged behind a tile: the packet of a head at T - 1 (128 data bytes), whole words
constexpr uint32_t RAW_WORDS = (T + LOOK + 4) / 4;
constexpr uint32_t NX_BITS = 12, NX_MASK = (1u << NX_BITS) - 1u;  // a position <= T + 128 | bytes produced (< 2^20) << 12
constexpr int CHAIN_TILES = 64;

__device__ __forceinline__ uint32_t find_segment(const RleSegment *segs, uint32_t nseg, uint32_t tile)
{
	uint32_t lo = 0, hi = nseg;  // the last segment whose tile0 <= tile
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (segs[mid].tile0 <= tile) lo = mid; else hi = mid;
	}
	return lo;
}

// the tile's bytes, and LOOK behind them as far as the segment goes, as whole words; returns where byte 0 of the tile sits in raw[]
__device__ __forceinline__ uint32_t stage_tile(const uint8_t *frames, uint64_t src, uint32_t rem, uint32_t *raw)
{
	const uint32_t al = (uint32_t)(src & 3u);
	const uint32_t *w = (const uint32_t *)(frames + (src - al));
	const uint32_t nwords = (al + min(rem, T + LOOK) + 3u) >> 2;  // <= RAW_WORDS; at most 3 bytes past the segment's end
	for (uint32_t k = threadIdx.x; k < nwords; k += blockDim.x) raw[k] = w[k];
	return al;
}

// position p of a tile read as a packet head: (next head | bytes produced << 12); rem = bytes of the segment from the tile on
__device__ __forceinline__ uint32_t packet_word(const uint8_t *tile, uint32_t p, uint32_t rem)
{
	if (p >= rem) return T;  // behind the segment: leaves the tile, produces nothing
	const uint32_t h = tile[p], avail = rem - p - 1u;
	if (h < 128u) return (p + h + 2u) | (min(h + 1u, avail) << NX_BITS);
	if (h > 128u) return (p + 2u) | ((avail ? 257u - h : 0u) << NX_BITS);
	return p + 1u;
}

__device__ __forceinline__ uint32_t compose(uint32_t w, uint32_t w2) { return (w2 & NX_MASK) | (((w >> NX_BITS) + (w2 >> NX_BITS)) << NX_BITS); }

__global__ void __launch_bounds__(256) rle_tabulate_kernel(RleDecodeArgs a)
{
	__shared__ uint32_t raw[RAW_WORDS];
	__shared__ uint32_t buf[2][T];
	const uint32_t tile = blockIdx.x, s = find_segment(a.segs, a.nseg, tile);
	const RleSegment sg = a.segs[s];
	const uint32_t base = (tile - sg.tile0) * T, rem = sg.len - base;
	const uint32_t al = stage_tile(a.frames, sg.src + base, rem, raw);
	__syncthreads();
	const uint8_t *tb = (const uint8_t *)raw + al;
	for (uint32_t p = threadIdx.x; p < T; p += 256) buf[0][p] = packet_word(tb, p, rem);
	__syncthreads();
	int cur = 0;
	for (;;) {
		int changed = 0;
		for (uint32_t p = threadIdx.x; p < T; p += 256) {
			uint32_t w = buf[cur][p];
			const uint32_t nx = w & NX_MASK;
			if (nx < T) { w = compose(w, buf[cur][nx]); changed = 1; }
			buf[cur ^ 1][p] = w;
		}
		cur ^= 1;
		if (!__syncthreads_or(changed)) break;
	}
	for (uint32_t e = threadIdx.x; e < RLE_ENTRIES; e += 256) a.table[(size_t)tile * RLE_ENTRIES + e] = buf[cur][e] - T;  // exit offset 0 .. 128
}

__global__ void __launch_bounds__(256) rle_chain_kernel(RleDecodeArgs a)
{
	__shared__ uint32_t tab[CHAIN_TILES * RLE_ENTRIES];
	const uint32_t s = blockIdx.x;
	const RleSegment sg = a.segs[s];
	const uint32_t ntiles = (sg.len + T - 1u) / T;
	uint32_t e = 0, out = 0;
	for (uint32_t t0 = 0; t0 < ntiles; t0 += CHAIN_TILES) {
		const uint32_t nb = min((uint32_t)CHAIN_TILES, ntiles - t0);
		const uint32_t *src = a.table + (size_t)(sg.tile0 + t0) * RLE_ENTRIES;
		__syncthreads();
		for (uint32_t k = threadIdx.x; k < nb * RLE_ENTRIES; k += 256) tab[k] = src[k];
		__syncthreads();
		if (threadIdx.x == 0)
			for (uint32_t k = 0; k < nb; k++) {
				const uint32_t w = tab[k * RLE_ENTRIES + e];
				a.tinfo[sg.tile0 + t0 + k] = make_uint2(e, out);
				out = min(out + (w >> NX_BITS), a.want);
				e = w & NX_MASK;
			}
	}
	if (threadIdx.x == 0) a.short_seg[s] = out < a.want ? 1u : 0u;
}

__global__ void __launch_bounds__(256) rle_expand_kernel(RleDecodeArgs a)
{
	__shared__ uint32_t raw[RAW_WORDS];
	__shared__ uint32_t buf[2][T];
	__shared__ uint8_t mark[T];
	__shared__ uint32_t wsum[2][4];
	const uint32_t tile = blockIdx.x, s = find_segment(a.segs, a.nseg, tile);
	const RleSegment sg = a.segs[s];
	const uint2 ti = a.tinfo[tile];
	const uint32_t entry = ti.x, out0 = ti.y;
	if (out0 >= a.want) return;  // the whole workgroup: the plane is complete before this tile
	const uint32_t base = (tile - sg.tile0) * T, rem = sg.len - base;
	const uint32_t al = stage_tile(a.frames, sg.src + base, rem, raw);
	for (uint32_t p = threadIdx.x; p < T; p += 256) mark[p] = p == entry;
	__syncthreads();
	const uint8_t *tb = (const uint8_t *)raw + al;
	for (uint32_t p = threadIdx.x; p < T; p += 256) buf[0][p] = packet_word(tb, p, rem);
	__syncthreads();
	int cur = 0;
	for (;;) {
		bool m[T / 256];
#pragma unroll
		for (uint32_t q = 0; q < T / 256; q++) m[q] = mark[threadIdx.x + 256u * q] != 0;
		__syncthreads();
		int changed = 0;
#pragma unroll
		for (uint32_t q = 0; q < T / 256; q++) {
			const uint32_t p = threadIdx.x + 256u * q;
			uint32_t w = buf[cur][p];
			const uint32_t nx = w & NX_MASK;
			if (nx < T) {
				if (m[q]) mark[nx] = 1;  // round r: the head 2^r packets on
				w = compose(w, buf[cur][nx]);
				changed = 1;
			}
			buf[cur ^ 1][p] = w;
		}
		cur ^= 1;
		if (!__syncthreads_or(changed)) break;
	}
	// heads that produce bytes, in order, with the offsets of what they produce: thread t owns positions 8t .. 8t + 7
	uint32_t *hoff = buf[0], *hpos = buf[1];
	const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, p0 = threadIdx.x * (T / 256);
	uint32_t prod[T / 256], cnt = 0, sum = 0;
#pragma unroll
	for (uint32_t q = 0; q < T / 256; q++) {
		prod[q] = mark[p0 + q] ? packet_word(tb, p0 + q, rem) >> NX_BITS : 0u;
		cnt += prod[q] != 0;
		sum += prod[q];
	}
	uint32_t ctot, stot;
	uint32_t cex = wave_excl_scan(cnt, ctot), sex = wave_excl_scan(sum, stot);
	__syncthreads();  // every read of buf[] by the loop above is done: it becomes hoff / hpos
	if (lane == 0) { wsum[0][wv] = ctot; wsum[1][wv] = stot; }
	__syncthreads();
	uint32_t H = 0, P = 0;
	for (uint32_t k = 0; k < 4; k++) {
		if (k < wv) { cex += wsum[0][k]; sex += wsum[1][k]; }
		H += wsum[0][k]; P += wsum[1][k];
	}
#pragma unroll
	for (uint32_t q = 0; q < T / 256; q++)
		if (prod[q]) { hoff[cex] = sex; hpos[cex] = p0 + q; cex++; sex += prod[q]; }
	__syncthreads();
	const uint32_t count = min(P, a.want - out0);  // clip at rows * cols
	uint8_t *dst = a.images + sg.dst + (size_t)out0 * a.step;
	for (uint32_t o = threadIdx.x; o < count; o += 256) {
		uint32_t lo = 0, hi = H;  // the last head whose offset <= o (hoff[0] == 0)
		while (hi - lo > 1) {
			const uint32_t mid = (lo + hi) >> 1;
			if (hoff[mid] <= o) lo = mid; else hi = mid;
		}
		const uint32_t pos = hpos[lo], h = tb[pos];
		dst[(size_t)o * a.step] = h < 128u ? tb[pos + 1u + (o - hoff[lo])] : tb[pos + 1u];
	}
}

}  // namespace

hipError_t launch_dicom_rle_encode(const void *d_images, int n, int rows, int cols, int planes, uint32_t *d_rowinfo, uint8_t *d_out,
                                   size_t out_stride, uint32_t *d_out_sizes, hipStream_t st)
{
	const uint64_t total_rows = (uint64_t)n * (uint64_t)rows;
	const dim3 grid((unsigned)((total_rows + 3) / 4)), block(256);
	if (planes == 2) {
		hipLaunchKernelGGL((rle_rows_kernel<uint16_t, false>), grid, block, 0, st, (const uint16_t *)d_images, total_rows, (uint32_t)rows, (uint32_t)cols, d_rowinfo, d_out, out_stride);
		hipLaunchKernelGGL(rle_layout_kernel, dim3(n), dim3(64), 0, st, (uint32_t)rows, planes, d_rowinfo, d_out, out_stride, d_out_sizes);
		hipLaunchKernelGGL((rle_rows_kernel<uint16_t, true>), grid, block, 0, st, (const uint16_t *)d_images, total_rows, (uint32_t)rows, (uint32_t)cols, d_rowinfo, d_out, out_stride);
	} else {
		hipLaunchKernelGGL((rle_rows_kernel<uint8_t, false>), grid, block, 0, st, (const uint8_t *)d_images, total_rows, (uint32_t)rows, (uint32_t)cols, d_rowinfo, d_out, out_stride);
		hipLaunchKernelGGL(rle_layout_kernel, dim3(n), dim3(64), 0, st, (uint32_t)rows, planes, d_rowinfo, d_out, out_stride, d_out_sizes);
		hipLaunchKernelGGL((rle_rows_kernel<uint8_t, true>), grid, block, 0, st, (const uint8_t *)d_images, total_rows, (uint32_t)rows, (uint32_t)cols, d_rowinfo, d_out, out_stride);
	}
	return hipGetLastError();
}

hipError_t launch_dicom_rle_decode(const RleDecodeArgs &a, hipStream_t st)
{
	hipLaunchKernelGGL(rle_tabulate_kernel, dim3(a.ntiles), dim3(256), 0, st, a);
	hipLaunchKernelGGL(rle_chain_kernel, dim3(a.nseg), dim3(256), 0, st, a);
	hipLaunchKernelGGL(rle_expand_kernel, dim3(a.ntiles), dim3(256), 0, st, a);
	return hipGetLastError();
}

}  // namespace cct
