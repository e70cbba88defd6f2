// JPEG 2000 Part-1 (ITU-T T.800) lossless decoder for one unsigned component of precision 2 .. 16: the device side of
// cct_j2k_decode_batch (api_jpeg2000.cpp), the mirror of jpeg2000_kernels.hip.  tests/jpeg2000_decode_model.py is the CPU
// restatement on every input, damaged or not.  The host has walked the markers; a file arrives as its tile data and a J2kDecFile.
//
//   1 parse    one workgroup per file: the lanes clear the file's code-block records and tag-tree nodes; lane 0 reads the
//              packet headers bit by bit (B.10: a stuffed bit behind every 0xFF, inclusion and zero-bit-plane tag trees,
//              Table B.4, Lblock, lengths) in one of the two packet sequences, keeps per code-block what the layers add up to
//              and lists the chunks of codeword bytes; then the waves gather every block's chunks into one segment.
//   2 tier1    one wave per code-block (Annex D).  LDS holds what the encoder's holds, laid out by jpeg2000_device.h, which
//              both include: one word per sample with a one-sample border (neighbour significance, state, sign, magnitude),
//              the two context tables, the MQ table and the contexts.  The lanes clear the block and build the tables, lane 0
//              runs exactly the passes the packets declared through the MQ decoder (C.3), the lanes write the signed
//              coefficients into the plane.  A block no packet included is zeros.
//   3 idwt     per level from the coarsest, rows and then columns, one lane per output sample, plane_a -> plane_b -> plane_a:
//              x(2n) = s(n) - floor((d(n-1) + d(n) + 2) / 4), x(2n+1) = d(n) + floor((x(2n) + x(2n+2)) / 2), whole-sample
//              symmetric extension, modulo 2^32.
//   4 finish   + 2^(precision - 1), clamped to 0 .. 2^precision - 1, >> shift, stored as uint8 or uint16.
// The chunks are gathered rather than read through a list: with style 0 all layers of a block form one MQ codeword, the copy
// moves each file byte once (next to a Tier-1 that spends tens of cycles a bit), and the MQ decoder keeps one bounds check
// and one cached word a byte where a list would put a chunk lookup into BYTEIN.
// LDS of tier1 is sized by the launch from the code-block exponents of the files it covers: 776 B of tables +
// (2^xcb + 2)(2^ycb + 2) * 4: 18 200 B at 64 x 64 (9 waves a CU, below the encoder's 18 204), 5 400 B at 32 x 32 (30 waves).
// Bounds.  parse: every byte is read below the file's len; a chunk lies inside the tile data (checked before it is listed)
// and the list holds min(len, blocks * layers) entries, which the chunks cannot exceed (each has a byte of its own and a
// (block, layer) of its own); the segments total at most len.  tier1: a block's rectangle and the LDS indices come from
// the host's layout; the MQ decoder reads segment bytes below the block's length and 0xFF beyond (whole aligned words of the
// segment buffer, which is padded).  Passes: the parse admits at most 3 planes - 2, so the plane index stays >= 0.
#include <algorithm>

#include "cct_internal.h"
#include "jpeg2000_device.h"
#include "../../include/compact_hip.h"

#ifndef J2K_DEC_DYNAMIC_LDS  // the host emulation supplies the launch's bytes its own way
#define J2K_DEC_DYNAMIC_LDS(name) extern __shared__ uint32_t name[]
#endif

namespace cct {
namespace {

// ---- packets --------------------------------------------------------------------------------------------------------

struct DecBits {  // packet header bits (B.10.1); past the end: err, and zeros
	const uint8_t *d; uint32_t pos, end;
	uint32_t cur = 0, left = 0; bool err = false;
	__device__ __forceinline__ uint32_t get()
	{
		if (!left) {
			if (pos >= end) { err = true; return 0; }
			left = cur == 0xFF ? 7 : 8;
			cur = d[pos++];
		}
		left--;
		return (cur >> left) & 1;
	}
	__device__ __forceinline__ uint64_t bits(uint32_t n) { uint64_t v = 0; while (n--) v = v << 1 | get(); return v; }
	__device__ __forceinline__ void align()  // a header that ends in 0xFF is followed by a stuffed zero byte
	{
		if (cur == 0xFF) { if (pos >= end) err = true; else pos++; }
		cur = 0; left = 0;
	}
};

struct DecTagTree {
	TagTreeShape<J2K_DEC_TT_LEVELS> at;  // the shape of both trees of a subband; a value of 255 is not known yet
	__device__ bool decode(DecBits &br, uint8_t *low, uint8_t *val, uint32_t x, uint32_t y, uint32_t threshold) const  // threshold <= 33
	{
		uint32_t lo = 0, k = 0;
		for (int lv = (int)at.nlev - 1; lv >= 0; lv--) {
			k = at.node(lv, x, y);
			lo = std::max<uint32_t>(lo, low[k]);
			while (lo < threshold && lo < val[k]) {
				if (br.get()) val[k] = (uint8_t)lo;
				else lo++;
			}
			low[k] = (uint8_t)lo;
		}
		return val[k] < threshold;
	}
};

__device__ __forceinline__ uint32_t dec_passes(DecBits &br)  // Table B.4
{
	if (!br.get()) return 1;
	if (!br.get()) return 2;
	uint32_t v = (uint32_t)br.bits(2);
	if (v != 3) return 3 + v;
	v = (uint32_t)br.bits(5);
	if (v != 31) return 6 + v;
	return 37 + (uint32_t)br.bits(7);
}

__global__ __launch_bounds__(256) void j2k_dec_parse_kernel(J2kDecArgs a)
{
	__shared__ uint32_t s_nchunks;
	const uint32_t file = blockIdx.x;
	const J2kDecFile F = a.flist[file];
	J2kDecCb *cb = a.cbs + F.cb0;
	uint8_t *tt = a.tt + F.tt0;
	J2kDecChunk *chunks = a.chunks + F.chunk0;
	const size_t T = F.tt_nodes;
	for (uint32_t k = threadIdx.x; k < F.nblocks; k += 256) cb[k] = J2kDecCb{file, 0, 0, 0, 0, 3, 0, 0};
	for (size_t k = threadIdx.x; k < 4 * T; k += 256) tt[k] = (k / T) & 1 ? 255 : 0;  // low, value, low, value
	__syncthreads();
	if (threadIdx.x == 0) {
		DecBits br;
		br.d = a.files + F.src; br.pos = 0; br.end = F.len;
		const J2kDecBand *bands = a.bands + F.band0;
		const uint32_t nres = F.levels + 1, npk = nres * F.layers;
		uint32_t nchunks = 0;
		bool bad = false;
		DecTagTree tree;
		for (uint32_t pk = 0; pk < npk && !bad; pk++) {
			const uint32_t layer = F.seq ? pk % F.layers : pk / nres, res = F.seq ? pk / F.layers : pk % nres;
			const uint32_t b0 = res ? 3 * res - 2 : 0, b1 = res ? b0 + 3 : 1;
			if (br.get()) {
				for (uint32_t b = b0; b < b1 && !bad; b++) {
					const J2kDecBand bd = bands[b];
					const uint32_t nb = bd.ncw * bd.nch;  // cb0 + nb <= nblocks, tt0 + nodes <= tt_nodes by the host's layout
					if (!nb) continue;
					tree.at.shape(bd.ncw, bd.nch);
					uint8_t *il = tt + bd.tt0, *iv = il + T, *zl = iv + T, *zv = zl + T;
					for (uint32_t k = 0; k < nb && !bad; k++) {
						J2kDecCb c = cb[bd.cb0 + k];
						const uint32_t x = k % bd.ncw, y = k / bd.ncw;
						if (!(c.included ? br.get() : (uint32_t)tree.decode(br, il, iv, x, y, layer + 1))) continue;
						if (!c.included) {
							c.included = 1;
							bad = true;  // more zero bit-planes than Mb, unless a threshold finds the value
							for (uint32_t t = 1; t <= bd.mb + 1; t++)
								if (tree.decode(br, zl, zv, x, y, t)) { c.planes = bd.mb - (t - 1); bad = false; break; }
							if (bad) break;
						}
						const uint32_t np = dec_passes(br);
						while (br.get())
							if (++c.lblock > 32) { bad = true; break; }
						if (bad) break;
						const uint64_t ln = br.bits(c.lblock + (31u - (uint32_t)__clz((int)np)));
						c.passes += np;  // <= 32 * 164
						if (br.err || (int)c.passes > 3 * (int)c.planes - 2 || ln > F.len) { bad = true; break; }
						c.pend = (uint32_t)ln;
						cb[bd.cb0 + k] = c;
					}
				}
			}
			br.align();
			if (br.err) bad = true;
			for (uint32_t b = b0; b < b1 && !bad; b++) {
				const J2kDecBand bd = bands[b];
				for (uint32_t k = 0; k < bd.ncw * bd.nch; k++) {
					const uint32_t ln = cb[bd.cb0 + k].pend;
					if (!ln) continue;
					if (ln > br.end - br.pos || nchunks >= F.chunk_cap) { bad = true; break; }
					chunks[nchunks++] = J2kDecChunk{bd.cb0 + k, br.pos, ln, 0};
					cb[bd.cb0 + k].bytes += ln;
					cb[bd.cb0 + k].pend = 0;
					br.pos += ln;
				}
			}
		}
		if (bad) {
			a.status[file] = J2K_DEC_ST_STREAM;
			nchunks = 0;
		} else {
			uint32_t at = 0;  // the segments back to back in block order; pend counts what a segment holds so far
			for (uint32_t k = 0; k < F.nblocks; k++) { cb[k].seg = at; at += cb[k].bytes; }
			for (uint32_t q = 0; q < nchunks; q++) {
				J2kDecCb &c = cb[chunks[q].cb];
				chunks[q].dst = c.seg + c.pend;
				c.pend += chunks[q].len;
			}
		}
		s_nchunks = nchunks;
	}
	__syncthreads();
	const uint32_t nchunks = s_nchunks, lane = threadIdx.x & 63;
	const uint8_t *from = a.files + F.src;
	uint8_t *to = a.segs + F.src;
	for (uint32_t q = threadIdx.x >> 6; q < nchunks; q += 4) {  // src + len <= F.len was checked; dst + len <= the sum of the chunks <= F.len
		const J2kDecChunk ch = chunks[q];
		for (uint32_t k = lane; k < ch.len; k += 64) to[ch.dst + k] = from[ch.src + k];
	}
}

// ---- Tier-1 ---------------------------------------------------------------------------------------------------------

struct MqDecoder {  // Annex C.3; a byte at or beyond len reads as 0xFF, C is a 32-bit register
	uint32_t a, c, ct, pos, len;
	const uint32_t *words; size_t base;  // the segment is bytes base .. base + len of the buffer `words` begins (aligned, padded)
	size_t have = ~(size_t)0; uint32_t word = 0;  // the aligned word read last
	const uint32_t *table; uint32_t *ctx;  // LDS: the 47 states; per context the table entry of its state | MPS << 29

	__device__ __forceinline__ uint32_t byte(uint32_t i)
	{
		if (i >= len) return 0xFF;
		const size_t at = base + i;
		if ((at >> 2) != have) { have = at >> 2; word = words[have]; }
		return (word >> (8 * (uint32_t)(at & 3))) & 0xFF;
	}
	__device__ __forceinline__ void bytein()
	{
		if (byte(pos) == 0xFF) {
			const uint32_t b1 = byte(pos + 1);
			if (b1 > 0x8F) { c += 0xFF00; ct = 8; }
			else { pos++; c += b1 << 9; ct = 7; }
		} else {
			pos++; c += byte(pos) << 8; ct = 8;
		}
	}
	__device__ __forceinline__ void init()
	{
		pos = 0;
		c = byte(0) << 16;
		bytein();
		c <<= 7; ct -= 7; a = 0x8000;
	}
	__device__ __forceinline__ uint32_t decode(uint32_t cx)
	{
		const uint32_t e = ctx[cx], qe = e & 0xFFFF, mps = (e >> 29) & 1;
		bool lps;
		a -= qe;
		if ((c >> 16) < qe) {
			lps = a >= qe;
			a = qe;
		} else {
			c -= qe << 16;
			if (a & 0x8000) return mps;
			lps = a < qe;
		}
		ctx[cx] = lps ? table[(e >> 22) & 63] | (mps ^ ((e >> 28) & 1)) << 29 : table[(e >> 16) & 63] | mps << 29;
		uint32_t sh = (uint32_t)__clz((int)a) - 16u;  // RENORMD: 0 < a < 0x8000, a byte in whenever ct runs out
		while (sh) {
			if (!ct) bytein();
			const uint32_t k = std::min(sh, ct);
			a <<= k; c <<= k; ct -= k; sh -= k;
		}
		return mps ^ (uint32_t)lps;
	}
};

__global__ __launch_bounds__(64) void j2k_dec_tier1_kernel(J2kDecArgs a, uint32_t cb0)
{
	J2K_DEC_DYNAMIC_LDS(s_mem);  // j2k_dec_lds_bytes: 47 + 19 words, 2 x 256 bytes, then the block with its border
	uint32_t *s_table = s_mem, *s_ctx = s_mem + 47, *s_w = s_mem + 194;
	uint8_t *s_zc = (uint8_t *)(s_mem + 66), *s_sc = s_zc + 256;
	const uint32_t lane = threadIdx.x, at = cb0 + blockIdx.x;
	const J2kDecCb C = a.cbs[at];
	if (a.status[C.file]) return;  // the file has no raster
	const J2kDecFile F = a.flist[C.file];
	const J2kDecBlock B = a.blocks[F.blk0 + (at - F.cb0)];
	const uint32_t w = B.w, h = B.h, FW = w + 2;
	int32_t *dst = a.plane_a + (size_t)F.slot * a.rows * a.cols + (size_t)B.y0 * a.cols + B.x0;
	if (!C.passes) {  // never included
		for (uint32_t i = lane; i < w * h; i += 64) dst[(size_t)(i / w) * a.cols + i % w] = 0;
		return;
	}
	for (uint32_t i = lane; i < FW * (h + 2); i += 64) s_w[i] = 0;
	t1_load_tables(lane, B.orient, s_table, s_ctx, s_zc, s_sc);
	__syncthreads();
	if (lane == 0) {
		MqDecoder mq;
		mq.words = (const uint32_t *)a.segs; mq.base = (size_t)F.src + C.seg; mq.len = C.bytes; mq.table = s_table; mq.ctx = s_ctx;
		mq.init();
		auto significant = [&](uint32_t i) {  // decodes the sign of sample i and tells the eight neighbours -> T1_NEG or 0
			const uint32_t n = s_w[i - FW], s = s_w[i + FW], wl = s_w[i - 1], e = s_w[i + 1];
			const uint32_t sc = s_sc[t1_sign_key(n, s, wl, e)];
			const uint32_t neg = mq.decode(sc & 127) ^ (sc >> 7);
			// t1_tell_neighbours, written out: through the helper this kernel measured 0.5 % slower at 64 x 64
			s_w[i - FW] = n | T1_S; s_w[i + FW] = s | T1_N; s_w[i - 1] = wl | T1_E; s_w[i + 1] = e | T1_W;
			s_w[i - FW - 1] |= T1_SE; s_w[i - FW + 1] |= T1_SW;
			s_w[i + FW - 1] |= T1_NE; s_w[i + FW + 1] |= T1_NW;
			return neg ? T1_NEG : 0u;
		};
		for (uint32_t k = 0; k < C.passes; k++) {  // passes <= 3 planes - 2 and planes <= 19: the plane's bit is 12 .. 30
			const uint32_t kind = (k + 2) % 3, one = 1u << (T1_MAG_SHIFT + C.planes - 1 - (k + 2) / 3);
			for (uint32_t y0 = 0; y0 < h; y0 += 4)
				for (uint32_t x = 0; x < w; x++) {
					const uint32_t i0 = (y0 + 1) * FW + x + 1, y1 = std::min(y0 + 4, h);
					if (kind == 0) {  // significance propagation
						if (y0 + 4 <= h &&  // a column without a candidate decodes nothing, so nothing in it changes
						    !(spp_candidate(s_w[i0]) | spp_candidate(s_w[i0 + FW]) | spp_candidate(s_w[i0 + 2 * FW]) | spp_candidate(s_w[i0 + 3 * FW])))
							continue;
						for (uint32_t y = y0; y < y1; y++) {
							const uint32_t i = (y + 1) * FW + x + 1, f = s_w[i];
							if ((f & T1_SIG) || !(f & T1_NBR)) continue;
							uint32_t nf = f | T1_VISIT;
							if (mq.decode(s_zc[f & T1_NBR])) nf |= one | T1_SIG | significant(i);
							s_w[i] = nf;  // its own word is not among the eight
						}
					} else if (kind == 1) {  // magnitude refinement
						if (y0 + 4 <= h &&
						    !(mrp_candidate(s_w[i0]) | mrp_candidate(s_w[i0 + FW]) | mrp_candidate(s_w[i0 + 2 * FW]) | mrp_candidate(s_w[i0 + 3 * FW])))
							continue;
						for (uint32_t y = y0; y < y1; y++) {
							const uint32_t i = (y + 1) * FW + x + 1, f = s_w[i];
							if ((f & (T1_SIG | T1_VISIT)) != T1_SIG) continue;
							const uint32_t bit = mq.decode(f & T1_REFINED ? CTX_MAG + 2 : CTX_MAG + ((f & T1_NBR) ? 1 : 0));
							s_w[i] = f | T1_REFINED | (bit ? one : 0);
						}
					} else {  // cleanup; it takes the visit marks back
						uint32_t first = y0;
						if (y0 + 4 <= h) {
							const uint32_t f0 = s_w[i0], f1 = s_w[i0 + FW], f2 = s_w[i0 + 2 * FW], f3 = s_w[i0 + 3 * FW];
							if (!((f0 | f1 | f2 | f3) & (T1_SIG | T1_VISIT | T1_NBR))) {
								if (!mq.decode(CTX_RL)) continue;
								uint32_t r = mq.decode(CTX_UNI) << 1;
								r |= mq.decode(CTX_UNI);
								const uint32_t i = i0 + r * FW, f = r == 0 ? f0 : r == 1 ? f1 : r == 2 ? f2 : f3;
								s_w[i] = f | one | T1_SIG | significant(i);
								first = y0 + r + 1;
							}
						}
						for (uint32_t y = first; y < y1; y++) {
							const uint32_t i = (y + 1) * FW + x + 1, f = s_w[i];
							if (f & (T1_SIG | T1_VISIT)) { s_w[i] = f & ~T1_VISIT; continue; }
							if (mq.decode(s_zc[f & T1_NBR])) s_w[i] = f | one | T1_SIG | significant(i);
						}
					}
				}
		}
	}
	__syncthreads();
	for (uint32_t i = lane; i < w * h; i += 64) {
		const uint32_t y = i / w, x = i % w, f = s_w[(y + 1) * FW + x + 1], m = f >> T1_MAG_SHIFT;
		dst[(size_t)y * a.cols + x] = (int32_t)(f & T1_NEG ? 0u - m : m);
	}
}

// ---- inverse transform and finish -------------------------------------------------------------------------------------

// One inverse lifting step along the rows or (vertical) the columns of the w x h corner of the plane of every file that has
// at least `level` decompositions.  Sums are unsigned: modulo 2^32, whatever a damaged file holds.
__global__ __launch_bounds__(256) void j2k_dec_idwt_kernel(J2kDecArgs a, const int32_t *src, int32_t *dst, uint32_t level, uint32_t w, uint32_t h,
                                                            uint32_t vertical)
{
	const size_t wh = (size_t)w * h, i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)a.nfiles * wh) return;
	const uint32_t file = (uint32_t)(i / wh);
	if (a.status[file] || level > a.flist[file].levels) return;
	const size_t frame = (size_t)a.flist[file].slot * a.rows * a.cols;
	const uint32_t r = (uint32_t)(i % wh), y = r / w, x = r % w;
	const int len = (int)(vertical ? h : w), k = (int)(vertical ? y : x), nl = (len + 1) / 2, nh = len / 2;
	const int32_t *line = src + frame + (vertical ? (size_t)x : (size_t)y * a.cols);
	const size_t step = vertical ? a.cols : 1;
	auto S = [&](int n) { return (uint32_t)line[(size_t)n * step]; };  // 0 <= n < nl
	auto D = [&](int m) { return (uint32_t)line[(size_t)(nl + std::max(0, std::min(m, nh - 1))) * step]; };  // nh >= 1; d(-1) = d(0), d(nh) = d(nh - 1)
	auto E = [&](int n) { return S(n) - (uint32_t)((int32_t)(D(n - 1) + D(n) + 2u) >> 2); };
	uint32_t v;
	if (len == 1) v = S(0);
	else if (!(k & 1)) v = E(k / 2);
	else {
		const int n = k / 2;
		const uint32_t e0 = E(n), e1 = n + 1 < nl ? E(n + 1) : e0;  // x(len) = x(len - 2)
		v = D(n) + (uint32_t)((int32_t)(e0 + e1) >> 1);
	}
	dst[frame + (size_t)y * a.cols + x] = (int32_t)v;
}

template <typename Px>
__global__ __launch_bounds__(256) void j2k_dec_finish_kernel(J2kDecArgs a)
{
	const size_t N = (size_t)a.rows * a.cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)a.nfiles * N) return;
	const uint32_t file = (uint32_t)(i / N);
	if (a.status[file]) return;
	const size_t at = (size_t)a.flist[file].slot * N + i % N;
	const uint32_t p = a.flist[file].precision;
	const int32_t v = (int32_t)((uint32_t)a.plane_a[at] + (1u << (p - 1)));
	((Px *)a.images)[at] = (Px)((uint32_t)std::max(0, std::min(v, (int32_t)((1u << p) - 1))) >> a.shift);
}

}  // namespace

hipError_t launch_j2k_decode(const J2kDecArgs &a, const J2kDecRun *runs, size_t nruns, hipStream_t st)
{
	hipLaunchKernelGGL(j2k_dec_parse_kernel, dim3(a.nfiles), dim3(256), 0, st, a);
	if (TUNING && !(a.stages & 2)) return hipGetLastError();
	for (size_t r = 0; r < nruns; r++)
		hipLaunchKernelGGL(j2k_dec_tier1_kernel, dim3(runs[r].ncbs), dim3(64), j2k_dec_lds_bytes(runs[r].xcb, runs[r].ycb), st, a, runs[r].cb0);
	if (TUNING && !(a.stages & 4)) return hipGetLastError();
	const J2kSizes z = j2k_level_sizes(a.rows, a.cols, a.max_levels);
	for (uint32_t d = a.max_levels; d >= 1; d--) {
		const uint32_t w = z.w[d - 1], h = z.h[d - 1];
		const dim3 grid((unsigned)(((size_t)a.nfiles * w * h + 255) / 256));
		hipLaunchKernelGGL(j2k_dec_idwt_kernel, grid, dim3(256), 0, st, a, (const int32_t *)a.plane_a, a.plane_b, d, w, h, 0u);
		hipLaunchKernelGGL(j2k_dec_idwt_kernel, grid, dim3(256), 0, st, a, (const int32_t *)a.plane_b, a.plane_a, d, w, h, 1u);
	}
	if (TUNING && !(a.stages & 8)) return hipGetLastError();
	const dim3 per_sample((unsigned)(((size_t)a.nfiles * a.rows * a.cols + 255) / 256));
	if (a.out_bits == 16) hipLaunchKernelGGL(j2k_dec_finish_kernel<uint16_t>, per_sample, dim3(256), 0, st, a);
	else hipLaunchKernelGGL(j2k_dec_finish_kernel<uint8_t>, per_sample, dim3(256), 0, st, a);
	return hipGetLastError();
}

}  // namespace cct
