// JPEG 2000 Part-1 (ITU-T T.800) lossless encoder for one unsigned component of precision 2 .. 16: the device side of
// cct_j2k_encode_batch (api_jpeg2000.cpp).  tests/jpeg2000_model.py is the CPU restatement, byte for byte.
//
//   1 convert  sample << shift, checked against the precision, minus 2^(precision - 1), into the int32 plane
//   2 dwt      `levels` stages of the reversible 5/3 lifting, columns and then rows (F.4.2), one lane per output sample:
//              d(n) = x(2n+1) - floor((x(2n) + x(2n+2)) / 2), s(n) = x(2n) + floor((d(n-1) + d(n) + 2) / 4), indices
//              reflected about 0 and len - 1 (whole-sample symmetric extension).  Two launches a stage, plane_a -> plane_b ->
//              plane_a, low half first (the Mallat arrangement), so every subband is a rectangle of plane_a.
//   3 tier1    one wave per code-block (Annex D).  The lanes load the block into LDS -- one word per sample with a
//              one-sample border: magnitude, sign, state and which neighbours are significant -- and reduce the
//              magnitudes to the number of bit-planes; lane 0 codes the planes (significance propagation, magnitude
//              refinement, cleanup) through the MQ coder (Annex C) into the block's slab.  A sample that becomes
//              significant tells its eight neighbours, so a visit reads one word, and the contexts come from two
//              256-entry tables in LDS.
//   4 tier2    one workgroup per frame: lane 0 writes the headers and, resolution by resolution (LRCP, one layer, one
//              precinct), the packet header -- inclusion and zero-bit-plane tag trees, passes, Lblock, length -- straight
//              into the file and notes where every code-block's bytes go; then all lanes copy the slabs.
// LDS of tier1: 64 x 64 blocks take 66 * 66 * 4 = 17 424 B of words + 780 B of tables = 18 204 B, 9 waves on a CU's
// 163 840 B with 4 bytes to spare (one more byte of LDS costs a wave); 32 x 32 blocks take 5 404 B, 30 waves.  The waves
// in flight are what Tier-1's throughput follows: DESIGN.md 5e has the measurements.
// The MQ state table, the word of a sample, its contexts and the tag-tree shape are jpeg2000_device.h, shared with the decoder.
// Bounds: a block's rectangle comes from the host's layout (inside rows x cols); LDS indices from (w, h) <= CB; every slab
// byte is checked against slab_cap and every header byte against out_stride before it is stored.
#include <algorithm>

#include "cct_internal.h"
#include "jpeg2000_device.h"
#include "wave_device.h"
#include "../../include/compact_hip.h"

namespace cct {
namespace {

// ---- convert and transform ------------------------------------------------------------------------------------------

template <typename Px>
__global__ __launch_bounds__(256) void j2k_convert_kernel(J2kArgs a)
{
	const size_t N = (size_t)a.rows * a.cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)a.n * N) return;
	const uint32_t v = (uint32_t)((const Px *)a.images)[i] << a.shift;
	if (v >> a.precision) atomicOr(&a.status[i / N], J2K_ST_OVERFLOW);
	a.plane_a[i] = (int32_t)v - (int32_t)(1u << (a.precision - 1));
}

// One lifting step along the columns (vertical) or the rows of the w x h corner of every frame's plane.
__global__ __launch_bounds__(256) void j2k_dwt_kernel(const int32_t *src, int32_t *dst, uint32_t n, uint32_t rows, uint32_t cols, uint32_t w,
                                                       uint32_t h, uint32_t vertical)
{
	const size_t wh = (size_t)w * h, i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)n * wh) return;
	const size_t frame = i / wh * ((size_t)rows * cols);
	const uint32_t r = (uint32_t)(i % wh), y = r / w, x = r % w;
	const int len = (int)(vertical ? h : w), k = (int)(vertical ? y : x), nl = (len + 1) / 2;
	const int32_t *line = src + frame + (vertical ? (size_t)x : (size_t)y * cols);
	const size_t step = vertical ? cols : 1;
	auto X = [&](int j) {  // len >= 2 and -2 <= j <= len + 1
		if (j < 0) j = -j;
		if (j >= len) j = 2 * (len - 1) - j;
		if (j < 0) j = -j;
		return line[(size_t)j * step];
	};
	auto D = [&](int m) { return X(2 * m + 1) - ((X(2 * m) + X(2 * m + 2)) >> 1); };
	int32_t v;
	if (len == 1) v = line[0];
	else if (k < nl) v = X(2 * k) + ((D(k - 1) + D(k) + 2) >> 2);
	else v = D(k - nl);
	dst[frame + (size_t)y * cols + x] = v;
}

// ---- Tier-1 ---------------------------------------------------------------------------------------------------------

struct MqCoder {  // Annex C.2; the byte before the first (pos -1) is imaginary
	uint32_t a = 0x8000, c = 0, ct = 12, b = 0;
	int pos = -1;
	uint8_t *out; uint32_t cap; bool over = false;
	const uint32_t *table; uint32_t *ctx;  // LDS: the 47 states; per context the table entry of its state | MPS << 29, one read a decision

	__device__ __forceinline__ void next(uint32_t byte)
	{
		if (pos >= 0) { if ((uint32_t)pos < cap) out[pos] = (uint8_t)b; else over = true; }
		pos++; b = byte;
	}
	__device__ __forceinline__ void byteout()
	{
		if (b == 0xFF) { next(c >> 20); c &= 0xFFFFF; ct = 7; return; }
		if (c >= 0x8000000u) {
			b++;
			if (b == 0xFF) { c &= 0x7FFFFFF; next(c >> 20); c &= 0xFFFFF; ct = 7; return; }
		}
		next((c >> 19) & 0xFF); c &= 0x7FFFF; ct = 8;
	}
	__device__ __forceinline__ void encode(uint32_t cx, uint32_t d)
	{
		const uint32_t e = ctx[cx], qe = e & 0xFFFF, mps = (e >> 29) & 1;
		a -= qe;
		if (d == mps) {
			if (a & 0x8000) { c += qe; return; }
			if (a < qe) a = qe; else c += qe;
			ctx[cx] = table[(e >> 16) & 63] | mps << 29;
		} else {
			if (a < qe) c += qe; else a = qe;
			ctx[cx] = table[(e >> 22) & 63] | (mps ^ ((e >> 28) & 1)) << 29;
		}
		uint32_t sh = (uint32_t)__clz((int)a) - 16u;  // RENORME: 0 < a < 0x8000, shifts until bit 15 is set, a byte out whenever ct runs out
		a <<= sh;
		while (sh >= ct) { c <<= ct; sh -= ct; byteout(); }
		c <<= sh; ct -= sh;
	}
	__device__ __forceinline__ uint32_t flush()  // C.2.9; a final 0xFF is not part of the segment.  -> bytes
	{
		const uint32_t t = c + a;
		c |= 0xFFFF;
		if (c >= t) c -= 0x8000;
		c <<= ct; byteout();
		c <<= ct; byteout();
		if (b == 0xFF) return (uint32_t)pos;
		if ((uint32_t)pos < cap) out[pos] = (uint8_t)b; else over = true;
		return (uint32_t)pos + 1;
	}
};

template <int CB>
__global__ __launch_bounds__(64) void j2k_tier1_kernel(J2kArgs a)
{
	constexpr int FW_MAX = CB + 2;
	__shared__ uint32_t s_w[FW_MAX * FW_MAX];  // the block with a border of samples that never become significant
	__shared__ uint32_t s_table[47];
	__shared__ uint32_t s_ctx[N_CTX];
	__shared__ uint8_t s_zc[256], s_sc[256];
	const uint32_t lane = threadIdx.x, frame = blockIdx.x / a.nblocks, blk = blockIdx.x % a.nblocks;
	if (a.status[frame] & J2K_ST_OVERFLOW) return;  // set by the convert kernel: the frame has no file
	const J2kBlock B = a.blocks[blk];
	const uint32_t w = B.w, h = B.h, FW = w + 2;
	const int32_t *src = a.plane_a + (size_t)frame * a.rows * a.cols + (size_t)B.y0 * a.cols + B.x0;
	uint32_t any = 0;
	for (uint32_t i = lane; i < FW * (h + 2); i += 64) {
		const uint32_t yy = i / FW, xx = i % FW;
		uint32_t f = 0;
		if (yy >= 1 && yy <= h && xx >= 1 && xx <= w) {
			const int32_t v = src[(size_t)(yy - 1) * a.cols + (xx - 1)];
			const uint32_t m = (uint32_t)(v < 0 ? -v : v);
			any |= m;
			f = m << T1_MAG_SHIFT | (v < 0 ? T1_NEG : 0);  // m < 2^19, or the block is refused below before a word is read
		}
		s_w[i] = f;
	}
	t1_load_tables(lane, B.orient, s_table, s_ctx, s_zc, s_sc);
	any = wave_or(any);
	__syncthreads();
	if (lane != 0) return;
	J2kBlockOut &res = a.cbout[(size_t)frame * a.nblocks + blk];
	const uint32_t nplanes = any ? 32u - (uint32_t)__clz((int)any) : 0u;
	if (nplanes > B.mb) { atomicOr(&a.status[frame], J2K_ST_GUARD); res = J2kBlockOut{0, 0, B.mb, 0}; return; }  // mb <= 19
	if (nplanes == 0) { res = J2kBlockOut{0, 0, B.mb, 0}; return; }

	MqCoder mq;
	mq.out = a.slabs + (size_t)frame * a.slab_stride + B.slab_off; mq.cap = B.slab_cap; mq.table = s_table; mq.ctx = s_ctx;
	auto significant = [&](uint32_t i, uint32_t f) {  // codes the sign of sample i (word f) and tells the eight neighbours
		const uint32_t n = s_w[i - FW], s = s_w[i + FW], wl = s_w[i - 1], e = s_w[i + 1];
		const uint32_t sc = s_sc[t1_sign_key(n, s, wl, e)];
		mq.encode(sc & 127, ((f >> 9) & 1) ^ (sc >> 7));
		t1_tell_neighbours(s_w, i, FW, n, s, wl, e);
	};
	for (int p = (int)nplanes - 1; p >= 0; p--) {
		const uint32_t pb = T1_MAG_SHIFT + (uint32_t)p;  // the plane's bit in a word
		if (p != (int)nplanes - 1) {
			for (uint32_t y0 = 0; y0 < h; y0 += 4)  // significance propagation
				for (uint32_t x = 0; x < w; x++) {
					if (y0 + 4 <= h) {  // four loads at once: a column without a candidate codes nothing, so nothing in it changes
						const uint32_t i0 = (y0 + 1) * FW + x + 1;
						if (!(spp_candidate(s_w[i0]) | spp_candidate(s_w[i0 + FW]) | spp_candidate(s_w[i0 + 2 * FW]) | spp_candidate(s_w[i0 + 3 * FW]))) continue;
					}
					for (uint32_t y = y0; y < std::min(y0 + 4, h); y++) {
						const uint32_t i = (y + 1) * FW + x + 1, f = s_w[i];
						if ((f & T1_SIG) || !(f & T1_NBR)) continue;
						const uint32_t bit = (f >> pb) & 1;
						mq.encode(s_zc[f & T1_NBR], bit);
						if (bit) significant(i, f);
						s_w[i] = f | T1_VISIT | (bit ? T1_SIG : 0);  // its own word is not among the eight
					}
				}
			for (uint32_t y0 = 0; y0 < h; y0 += 4)  // magnitude refinement
				for (uint32_t x = 0; x < w; x++) {
					if (y0 + 4 <= h) {
						const uint32_t i0 = (y0 + 1) * FW + x + 1;
						if (!(mrp_candidate(s_w[i0]) | mrp_candidate(s_w[i0 + FW]) | mrp_candidate(s_w[i0 + 2 * FW]) | mrp_candidate(s_w[i0 + 3 * FW]))) continue;
					}
					for (uint32_t y = y0; y < std::min(y0 + 4, h); y++) {
						const uint32_t i = (y + 1) * FW + x + 1, f = s_w[i];
						if ((f & (T1_SIG | T1_VISIT)) != T1_SIG) continue;
						mq.encode(f & T1_REFINED ? CTX_MAG + 2 : CTX_MAG + ((f & T1_NBR) ? 1 : 0), (f >> pb) & 1);
						s_w[i] = f | T1_REFINED;
					}
				}
		}
		for (uint32_t y0 = 0; y0 < h; y0 += 4)  // cleanup; it takes the visit marks back
			for (uint32_t x = 0; x < w; x++) {
				uint32_t first = y0;
				if (y0 + 4 <= h) {
					const uint32_t i0 = (y0 + 1) * FW + x + 1;
					const uint32_t f0 = s_w[i0], f1 = s_w[i0 + FW], f2 = s_w[i0 + 2 * FW], f3 = s_w[i0 + 3 * FW];
					if (!((f0 | f1 | f2 | f3) & (T1_SIG | T1_VISIT | T1_NBR))) {
						const uint32_t r = (f0 >> pb) & 1 ? 0 : (f1 >> pb) & 1 ? 1 : (f2 >> pb) & 1 ? 2 : (f3 >> pb) & 1 ? 3 : 4;
						if (r == 4) { mq.encode(CTX_RL, 0); continue; }
						mq.encode(CTX_RL, 1);
						mq.encode(CTX_UNI, r >> 1);
						mq.encode(CTX_UNI, r & 1);
						const uint32_t i = i0 + r * FW, f = r == 0 ? f0 : r == 1 ? f1 : r == 2 ? f2 : f3;
						significant(i, f);
						s_w[i] = f | T1_SIG;
						first = y0 + r + 1;
					}
				}
				for (uint32_t y = first; y < std::min(y0 + 4, h); y++) {
					const uint32_t i = (y + 1) * FW + x + 1, f = s_w[i];
					if (f & (T1_SIG | T1_VISIT)) { s_w[i] = f & ~T1_VISIT; continue; }
					const uint32_t bit = (f >> pb) & 1;
					mq.encode(s_zc[f & T1_NBR], bit);
					if (bit) { significant(i, f); s_w[i] = f | T1_SIG; }
				}
			}
	}
	const uint32_t bytes = mq.flush();
	if (mq.over) atomicOr(&a.status[frame], J2K_ST_CAP);
	res = J2kBlockOut{3 * nplanes - 2, mq.over ? 0u : bytes, B.mb - nplanes, 0};
}

// ---- Tier-2 ---------------------------------------------------------------------------------------------------------

struct BitWriter {  // packet header bits (B.10.1): the byte behind a 0xFF carries 7 bits
	uint8_t *out; size_t pos, cap; bool over = false;
	uint32_t cur = 0, free_bits = 8, full = 8;
	__device__ __forceinline__ void store(uint32_t byte) { if (pos < cap) out[pos] = (uint8_t)byte; else over = true; pos++; }
	__device__ __forceinline__ void put(uint32_t bit)
	{
		cur = cur << 1 | bit;
		if (--free_bits == 0) { store(cur); free_bits = full = cur == 0xFF ? 7 : 8; cur = 0; }
	}
	__device__ __forceinline__ void bits(uint32_t v, uint32_t n) { while (n--) put((v >> n) & 1); }
	__device__ __forceinline__ void finish()  // zero padding; a header does not end in 0xFF
	{
		const bool any = free_bits != full;
		uint32_t last = cur << free_bits;
		if (any) store(last);
		else last = full == 7 ? 0xFF : 0;  // full == 7: the byte stored last was 0xFF
		if (last == 0xFF) store(0);
		cur = 0; free_bits = full = 8;
	}
};

struct TagTree {  // a node: its value, what the decoder knows to be a lower bound, whether it knows the value
	uint8_t *val, *low, *known;
	TagTreeShape<J2K_TT_LEVELS> at;
	__device__ void build(uint32_t ncw, uint32_t nch)  // leaves are in val[0 .. ncw * nch); every other node is the minimum of its children
	{
		at.shape(ncw, nch);
		uint32_t pw = ncw, ph = nch;
		for (uint32_t lv = 0; lv + 1 < at.nlev; lv++) {
			const uint32_t cw = (pw + 1) / 2, ch = (ph + 1) / 2, o = at.off[lv], co = at.off[lv + 1];
			for (uint32_t y = 0; y < ch; y++)
				for (uint32_t x = 0; x < cw; x++) {
					uint32_t m = 255;
					for (uint32_t yy = 2 * y; yy < std::min(2 * y + 2, ph); yy++)
						for (uint32_t xx = 2 * x; xx < std::min(2 * x + 2, pw); xx++) m = std::min<uint32_t>(m, val[o + yy * pw + xx]);
					val[co + y * cw + x] = (uint8_t)m;
				}
			pw = cw; ph = ch;
		}
		const uint32_t total = at.off[at.nlev - 1] + pw * ph;
		for (uint32_t k = 0; k < total; k++) { low[k] = 0; known[k] = 0; }
	}
	__device__ void encode(BitWriter &bw, uint32_t x, uint32_t y, uint32_t threshold)
	{
		uint32_t lo = 0;
		for (int lv = (int)at.nlev - 1; lv >= 0; lv--) {
			const uint32_t k = at.node(lv, x, y);
			lo = std::max<uint32_t>(lo, low[k]);
			while (lo < threshold) {
				if (lo >= val[k]) {
					if (!known[k]) { bw.put(1); known[k] = 1; }
					break;
				}
				bw.put(0);
				lo++;
			}
			low[k] = (uint8_t)lo;
		}
	}
};

__global__ __launch_bounds__(256) void j2k_tier2_kernel(J2kArgs a)
{
	__shared__ uint32_t s_size;
	const uint32_t frame = blockIdx.x;
	uint8_t *out = a.out + (size_t)frame * a.out_stride;
	J2kBlockOut *cb = a.cbout + (size_t)frame * a.nblocks;
	if (threadIdx.x == 0) {
		s_size = 0;
		if (!a.status[frame]) {
			for (uint32_t k = 0; k < a.hdr_len; k++) out[k] = a.hdr[k];  // hdr_len <= J2K_HDR_MAX <= out_stride
			BitWriter bw;
			bw.out = out; bw.pos = a.hdr_len; bw.cap = a.out_stride;
			TagTree incl, zbp;
			uint8_t *tt = a.tt + (size_t)frame * 6 * a.tt_nodes;
			incl.val = tt; incl.low = tt + a.tt_nodes; incl.known = tt + 2 * (size_t)a.tt_nodes;
			zbp.val = tt + 3 * (size_t)a.tt_nodes; zbp.low = tt + 4 * (size_t)a.tt_nodes; zbp.known = tt + 5 * (size_t)a.tt_nodes;
			for (uint32_t res = 0; res <= a.levels; res++) {
				const uint32_t b0 = res ? 3 * res - 2 : 0, b1 = res ? b0 + 3 : 1;
				uint32_t blocks = 0;
				for (uint32_t b = b0; b < b1; b++) blocks += a.bands[b].ncw * a.bands[b].nch;
				bw.put(blocks ? 1 : 0);
				for (uint32_t b = b0; b < b1; b++) {
					const J2kBand bd = a.bands[b];
					const uint32_t nb = bd.ncw * bd.nch;  // nb <= tt_nodes by the host's layout
					if (!nb) continue;
					for (uint32_t k = 0; k < nb; k++) {
						incl.val[k] = cb[bd.cb0 + k].passes ? 0 : 1;
						zbp.val[k] = (uint8_t)(cb[bd.cb0 + k].passes ? cb[bd.cb0 + k].zero_planes : bd.mb);
					}
					incl.build(bd.ncw, bd.nch);
					zbp.build(bd.ncw, bd.nch);
					for (uint32_t k = 0; k < nb; k++) {
						const J2kBlockOut r = cb[bd.cb0 + k];
						const uint32_t x = k % bd.ncw, y = k / bd.ncw;
						incl.encode(bw, x, y, 1);
						if (!r.passes) continue;
						zbp.encode(bw, x, y, 0xFFFFFFFFu);
						const uint32_t np = r.passes;  // Table B.4
						if (np == 1) bw.put(0);
						else if (np == 2) bw.bits(2, 2);
						else if (np <= 5) { bw.bits(3, 2); bw.bits(np - 3, 2); }
						else if (np <= 36) { bw.bits(15, 4); bw.bits(np - 6, 5); }
						else { bw.bits(0x1FF, 9); bw.bits(np - 37, 7); }
						const uint32_t lp = bit_length(np) - 1, need = bit_length(r.bytes), grow = need > lp + 3 ? need - lp - 3 : 0;  // Lblock starts at 3
						for (uint32_t g = 0; g < grow; g++) bw.put(1);
						bw.put(0);
						bw.bits(r.bytes, 3 + grow + lp);
					}
				}
				bw.finish();
				for (uint32_t b = b0; b < b1; b++) {
					const J2kBand bd = a.bands[b];
					for (uint32_t k = 0; k < bd.ncw * bd.nch; k++) { cb[bd.cb0 + k].dst = (uint32_t)bw.pos; bw.pos += cb[bd.cb0 + k].bytes; }
				}
			}
			if (bw.over || bw.pos + 2 > a.out_stride) {
				atomicOr(&a.status[frame], J2K_ST_CAP);
			} else {
				out[bw.pos] = 0xFF; out[bw.pos + 1] = 0xD9;
				const uint32_t total = (uint32_t)bw.pos + 2, psot = (uint32_t)bw.pos - (a.psot_at - 6);  // SOT marker .. the last packet
				for (int k = 0; k < 4; k++) out[a.psot_at + k] = (uint8_t)(psot >> (24 - 8 * k));
				if (a.jp2c_at) {
					const uint32_t box = total - a.jp2c_at;
					for (int k = 0; k < 4; k++) out[a.jp2c_at + k] = (uint8_t)(box >> (24 - 8 * k));
				}
				s_size = total;
			}
		}
	}
	__syncthreads();
	const uint32_t total = s_size;
	if (threadIdx.x == 0) a.out_sizes[frame] = total;
	if (!total) return;
	// dst + bytes <= total - 2 <= out_stride for every block: lane 0 summed exactly these lengths
	const uint8_t *slabs = a.slabs + (size_t)frame * a.slab_stride;
	for (uint32_t b = 0; b < a.nblocks; b++) {
		const uint32_t nbytes = cb[b].bytes, dst = cb[b].dst;
		const uint8_t *s = slabs + a.blocks[b].slab_off;
		for (uint32_t k = threadIdx.x; k < nbytes; k += 256) out[dst + k] = s[k];
	}
}

}  // namespace

hipError_t launch_j2k_encode(const J2kArgs &a, hipStream_t st)
{
	const size_t N = (size_t)a.rows * a.cols;
	const dim3 per_sample((unsigned)(((size_t)a.n * N + 255) / 256));
	if (a.src_bits == 16) hipLaunchKernelGGL(j2k_convert_kernel<uint16_t>, per_sample, dim3(256), 0, st, a);
	else hipLaunchKernelGGL(j2k_convert_kernel<uint8_t>, per_sample, dim3(256), 0, st, a);
	const J2kSizes z = j2k_level_sizes(a.rows, a.cols, a.levels);
	for (uint32_t l = 0; l < a.levels; l++) {
		const uint32_t w = z.w[l], h = z.h[l];
		const dim3 grid((unsigned)(((size_t)a.n * w * h + 255) / 256));
		hipLaunchKernelGGL(j2k_dwt_kernel, grid, dim3(256), 0, st, (const int32_t *)a.plane_a, a.plane_b, a.n, a.rows, a.cols, w, h, 1u);
		hipLaunchKernelGGL(j2k_dwt_kernel, grid, dim3(256), 0, st, (const int32_t *)a.plane_b, a.plane_a, a.n, a.rows, a.cols, w, h, 0u);
	}
	if (TUNING && !(a.stages & 2)) return hipGetLastError();
	if (a.codeblock == 64) hipLaunchKernelGGL(j2k_tier1_kernel<64>, dim3(a.n * a.nblocks), dim3(64), 0, st, a);
	else hipLaunchKernelGGL(j2k_tier1_kernel<32>, dim3(a.n * a.nblocks), dim3(64), 0, st, a);
	if (TUNING && !(a.stages & 4)) return hipGetLastError();
	hipLaunchKernelGGL(j2k_tier2_kernel, dim3(a.n), dim3(256), 0, st, a);
	return hipGetLastError();
}

}  // namespace cct
