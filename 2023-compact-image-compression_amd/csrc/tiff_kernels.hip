// Strip-organised grayscale TIFF (TIFF 6.0: LZW of section 13, horizontal differencing of section 14) as libtiff writes and
// reads it: the device side of cct_tiff_encode_batch / cct_tiff_read_batch (api_tiff.cpp).  tests/tiff_model.py restates both
// directions on the CPU.  Deflate strips go through the DEFLATE and INFLATE passes as they are; what is here is the predictor,
// the LZW coder and decoder, and the file layout.
//
// A strip is a stream of its own, so the parallelism of both LZW directions starts with the strips: one wave per strip, one
// wave per workgroup (the LDS of a strip is the workgroup's, and __syncthreads() is the wave's own fence).
//
// LZW numbering.  After a Clear the codes are counted from 1, Clear and EOI included: code j has 9 + (j > 254) + (j > 766) +
// (j > 1790) bits and, for j >= 2, defines table entry 256 + j: the string of code j - 1 plus the first byte of code j's.
// The encoder writes its Clear as code 3837.
//
// ENCODE.  The greedy parse is serial in the strip, so all 64 lanes follow it together: the lanes hold the next 64 input
// bytes (one load per 64 bytes), and a dictionary probe reads 64 consecutive slots of an open-addressed table in LDS at once
// (one conflict-free ds_read_b32); two ballots give the first match and the first free slot, and the match counts only if no
// free slot comes before it, which is linear probing's rule.  A slot holds (prefix code << 8 | byte) << 12 | code; 0 is free.
// TIFF_LZW_SLOTS = 8192 slots are 32 KiB, so a CU holds five strips (160 KiB); with 4096 slots the table would run at 94 %
// load.  Codes leave through a 64-bit accumulator, one big-endian word at a time, stored by lane 0 into the strip's own
// region: no atomics.
//
// DECODE.  The string of entry 256 + j is the output from where code j - 1 began, one byte longer than that code's string:
// every code is an LZ77 copy (destination, source, length) over the strip's own output.  A wave reads 64 codes at once (bit
// position and width of code j are a closed form of j), ballots find the first Clear / EOI / end of data and the first code
// beyond the table, lengths come from the (length, destination) kept in LDS for earlier codes, or, for a code that names one
// of the same 64, by pointer jumping (6 rounds of shuffles), destinations from a wave scan.  Copies whose source lies before
// the group's output run lane-parallel; a code whose source reaches into the group's own output (KwKwK, and any reference to
// one of the last codes) is copied by the whole wave in code order behind a fence.  Decoding stops when `want` bytes are out:
// a last string is cut, what follows is ignored.  Errors: a strip that does not open with a Clear, data or an EOI that ends
// the strip early, a code above 256 + j (for j = 1: anything but a literal), more than TIFF_LZW_MAX_J codes without a Clear.
// Every read of the coded strip is bounded by its length, every store by `want`, every iteration takes at least one code of
// 9 bits, and the loop count is bounded by bits / 9 + 2: a damaged strip ends in status 1.
#include "cct_internal.h"
#include "wave_device.h"
#include "../../include/compact_hip.h"

namespace cct {
namespace {

constexpr uint32_t LZW_CLEAR = 256, LZW_EOI = 257;

// ---- predictor and strip staging ------------------------------------------------------------------------------------

// one workgroup per raster row
template <typename T>
__global__ __launch_bounds__(256) void tiff_stage_kernel(const T *images, uint32_t rows, uint32_t cols, uint32_t predictor, uint32_t rps, uint32_t spf,
                                                         uint8_t *strips, size_t strip_stride, uint32_t *strip_sizes)
{
	const uint32_t i = blockIdx.x / rows, r = blockIdx.x % rows, s = r / rps, r_in = r - s * rps;
	const T *row = images + ((size_t)i * rows + r) * cols;
	const size_t k = (size_t)i * spf + s;
	uint8_t *dst = strips + k * strip_stride + (size_t)r_in * cols * sizeof(T);
	for (uint32_t x = threadIdx.x; x < cols; x += blockDim.x) {
		T v = row[x];
		if (predictor == 2 && x) v = (T)(v - row[x - 1]);
		if (sizeof(T) == 2) {
			dst[2 * (size_t)x] = (uint8_t)v;
			dst[2 * (size_t)x + 1] = (uint8_t)((uint32_t)v >> 8);
		} else {
			dst[x] = (uint8_t)v;
		}
	}
	if (r_in == 0 && threadIdx.x == 0) strip_sizes[k] = (uint32_t)(min(rps, rows - s * rps) * cols * sizeof(T));
}

// four waves per strip, a wave per row: 64 samples a step, the carry in a register
template <typename T>
__global__ __launch_bounds__(256) void tiff_unpredict_kernel(const uint8_t *files, const uint8_t *decoded, const TiffStrip *strips, uint32_t rows, uint32_t cols, T *images)
{
	const TiffStrip t = strips[blockIdx.x];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
	const uint8_t *src = (t.flags & TIFF_F_FROM_FILE) ? files + t.src : decoded + t.dst;
	const bool be = (t.flags & TIFF_F_BIG_ENDIAN) != 0, pred = (t.flags & TIFF_F_PREDICTOR) != 0;
	for (uint32_t r = wave; r < t.nrows; r += nw) {
		const uint8_t *in = src + (size_t)r * cols * sizeof(T);
		T *out = images + ((size_t)t.file * rows + t.row0 + r) * cols;
		uint32_t carry = 0;
		for (uint32_t x0 = 0; x0 < cols; x0 += 64) {  // wave-uniform bounds: every lane reaches the scan
			const uint32_t x = x0 + lane;
			uint32_t v = 0;
			if (x < cols) {
				if (sizeof(T) == 2) {
					const uint32_t b0 = in[2 * (size_t)x], b1 = in[2 * (size_t)x + 1];
					v = be ? (b0 << 8 | b1) : (b1 << 8 | b0);
				} else {
					v = in[x];
				}
			}
			if (pred) {
				uint32_t total;
				v = carry + wave_excl_scan(v, total) + v;
				carry += total;
			}
			if (x < cols) out[x] = (T)v;
		}
	}
}

// ---- LZW encode --------------------------------------------------------------------------------------------------------

struct BitSink { uint64_t acc; uint32_t nacc, words; uint64_t outcount; };  // outcount: bits since the last Clear, its own included

__device__ __forceinline__ void lzw_put(BitSink &b, uint32_t code, uint32_t w, uint32_t *out, uint32_t cap_words, uint32_t lane)
{
	b.acc = b.acc << w | code;
	b.nacc += w;
	b.outcount += w;
	if (b.nacc >= 32) {
		const uint32_t word = (uint32_t)(b.acc >> (b.nacc - 32));
		if (lane == 0 && b.words < cap_words) out[b.words] = __builtin_bswap32(word);
		b.words++;
		b.nacc -= 32;
	}
}

__device__ __forceinline__ void lzw_clear_table(uint32_t *tab, uint32_t lane)
{
	for (uint32_t k = lane; k < TIFF_LZW_SLOTS; k += 64) tab[k] = 0;
	__syncthreads();
}

__global__ __launch_bounds__(64) void tiff_lzw_encode_kernel(const uint8_t *strips, size_t strip_stride, const uint32_t *in_sizes, uint8_t *outb,
                                                            size_t out_stride, uint32_t *out_sizes)
{
	__shared__ uint32_t tab[TIFF_LZW_SLOTS];
	const uint32_t lane = threadIdx.x, L = in_sizes[blockIdx.x];
	const uint8_t *in = strips + (size_t)blockIdx.x * strip_stride;
	uint32_t *out = (uint32_t *)(outb + (size_t)blockIdx.x * out_stride);
	const uint32_t cap_words = (uint32_t)(out_stride / 4);
	BitSink bs{0, 0, 0, 0};
	uint32_t w = 9, next = 258;
	uint64_t incount = 1, checkpoint = 10000, ratio = 0;  // libtiff's compression-ratio rule (tests/tiff_model.py lzw_codes states it)
	lzw_clear_table(tab, lane);
	lzw_put(bs, LZW_CLEAR, w, out, cap_words, lane);
	uint32_t cur = lane < L ? in[lane] : 0;  // the 64 input bytes from i & ~63 on
	uint32_t omega = (uint32_t)__shfl((int)cur, 0);
	for (uint32_t i = 1; i < L; i++) {
		incount++;
		if ((i & 63) == 0) cur = i + lane < L ? in[i + lane] : 0;
		const uint32_t b = (uint32_t)__shfl((int)cur, (int)(i & 63));
		const uint32_t key = omega << 8 | b;
		uint32_t h = (key * 2654435761u) >> 19;  // 13 bits
		bool found = false;
		for (;;) {
			const uint32_t slot = (h + lane) & (TIFF_LZW_SLOTS - 1), e = tab[slot];
			const uint64_t mm = __ballot((e >> 12) == key && e != 0), em = __ballot(e == 0);
			const int fm = mm ? __ffsll((long long)mm) - 1 : 64, fe = em ? __ffsll((long long)em) - 1 : 64;
			if (fm < fe) {
				omega = (uint32_t)__shfl((int)e, fm) & 0xFFFu;
				found = true;
				break;
			}
			if (fe < 64) {
				if ((int)lane == fe) tab[slot] = key << 12 | next;
				break;
			}
			h += 64;  // 64 taken slots and no match: the probe goes on (the table is never full)
		}
		if (found) continue;
		lzw_put(bs, omega, w, out, cap_words, lane);
		next++;
		bool clear = next == 4094;
		if (!clear) {
			if (next == (1u << w)) {
				w++;
			} else if (incount >= checkpoint) {
				checkpoint = incount + 10000;
				const uint64_t rat = incount <= 0x7FFFFFu ? (incount << 8) / bs.outcount : (bs.outcount >> 8 ? incount / (bs.outcount >> 8) : 0x7FFFFFFFu);
				if (rat <= ratio) clear = true;
				else ratio = rat;
			}
		}
		if (clear) {
			incount = 0; bs.outcount = 0; ratio = 0;
			lzw_put(bs, LZW_CLEAR, w, out, cap_words, lane);
			lzw_clear_table(tab, lane);
			next = 258; w = 9;
		} else {
			__syncthreads();  // the new entry is in LDS before the next probe
		}
		omega = b;
	}
	lzw_put(bs, omega, w, out, cap_words, lane);
	next++;
	if (next == 4094) {
		lzw_put(bs, LZW_CLEAR, w, out, cap_words, lane);
		w = 9;
	} else if (next == (1u << w)) {
		w++;
	}
	lzw_put(bs, LZW_EOI, w, out, cap_words, lane);
	uint32_t size = bs.words * 4;
	if (bs.nacc) {
		const uint32_t word = (uint32_t)(bs.acc << (32 - bs.nacc));
		if (lane == 0 && bs.words < cap_words) out[bs.words] = __builtin_bswap32(word);
		size += (bs.nacc + 7) / 8;
	}
	if (lane == 0) out_sizes[blockIdx.x] = size;
}

// ---- LZW decode --------------------------------------------------------------------------------------------------------

// bits the first k codes after a Clear take
__device__ __forceinline__ uint32_t lzw_bits_of(uint32_t k)
{
	return 9 * k + (k > 254 ? k - 254 : 0) + (k > 766 ? k - 766 : 0) + (k > 1790 ? k - 1790 : 0);
}

__global__ __launch_bounds__(64) void tiff_lzw_decode_kernel(const uint8_t *files, const TiffStrip *strips, uint8_t *decoded, uint32_t *status)
{
	__shared__ uint32_t s_dst[TIFF_LZW_TAB];
	__shared__ uint16_t s_len[TIFF_LZW_TAB];
	const TiffStrip t = strips[blockIdx.x];
	const uint32_t lane = threadIdx.x, want = t.want;
	const uint8_t *in = files + t.src;
	uint8_t *out = decoded + t.dst;
	const uint64_t nbits = (uint64_t)t.len * 8;
	const uint64_t max_iter = nbits / 9 + 2;
	uint64_t P = 0;     // bit position of code jb
	uint32_t jb = 1;    // number of the code lane 0 reads
	uint32_t outpos = 0;
	bool err = true;    // what leaving by the loop bound means
	for (uint64_t iter = 0; iter < max_iter; iter++) {
		const uint32_t j = jb + lane;
		const uint32_t w = 9 + (j > 254) + (j > 766) + (j > 1790);
		const uint64_t pos = P + (lzw_bits_of(j - 1) - lzw_bits_of(jb - 1));
		const bool have = pos + w <= nbits;
		uint32_t code = 0;
		if (have) {
			const uint64_t b0 = pos >> 3;
			uint32_t B = (uint32_t)in[b0] << 16;
			if (b0 + 1 < t.len) B |= (uint32_t)in[b0 + 1] << 8;
			if (b0 + 2 < t.len) B |= (uint32_t)in[b0 + 2];
			code = (B >> (24 - (uint32_t)(pos & 7) - w)) & ((1u << w) - 1u);
		}
		const bool stop = !have || code == LZW_CLEAR || code == LZW_EOI;
		const bool bad = !stop && ((code >= 258 && code > 256 + j) || j > TIFF_LZW_MAX_J);
		const uint64_t sm = __ballot(stop), bm = __ballot(bad);
		const uint32_t F = sm ? (uint32_t)__ffsll((long long)sm) - 1 : 64, X = bm ? (uint32_t)__ffsll((long long)bm) - 1 : 64;
		const uint32_t nv = min(F, X);
		const bool valid = lane < nv;
		// lengths: a literal is 1, a table code one more than the code that defined its entry
		const uint32_t ref = valid && code >= 258 ? code - 257 : 0;  // number of that code; ref < j
		const bool in_group = ref >= jb;
		int ptr = -1;
		uint32_t val = valid ? 1 : 0;
		if (ref) {
			if (in_group) ptr = (int)(ref - jb);
			else val = (uint32_t)s_len[ref] + 1;
		}
#pragma unroll
		for (int r = 0; r < 6; r++) {
			const int p = ptr < 0 ? 0 : ptr;
			const uint32_t pv = (uint32_t)__shfl((int)val, p);
			const int pp = __shfl(ptr, p);
			if (ptr >= 0) { val += pv; ptr = pp; }
		}
		const uint32_t len = val;
		uint32_t total;
		const uint32_t off = wave_excl_scan(len, total);
		// 64-bit sums: a damaged strip may name more than 2^32 bytes
		const uint64_t dst64 = (uint64_t)outpos + off;
		const uint32_t dst = dst64 < want ? (uint32_t)dst64 : want;
		const uint32_t src_g = (uint32_t)__shfl((int)dst, in_group ? (int)(ref - jb) : 0);
		const uint32_t src = ref ? (in_group ? src_g : s_dst[ref]) : 0;
		if (valid && j < TIFF_LZW_TAB) { s_len[j] = (uint16_t)len; s_dst[j] = dst; }
		const uint32_t n = valid ? min(len, want - dst) : 0;  // the last string is cut
		const uint32_t G = outpos;
		const bool late = ref && n && src + n > G;  // reads what this group writes
		if (n && !ref) out[dst] = (uint8_t)code;
		if (n && ref && !late)
			for (uint32_t o = 0; o < n; o++) out[dst + o] = out[src + o];
		uint64_t lm = __ballot(late);
		__syncthreads();
		while (lm) {
			const int q = __ffsll((long long)lm) - 1;
			lm &= lm - 1;
			const uint32_t qs = (uint32_t)__shfl((int)src, q), qd = (uint32_t)__shfl((int)dst, q), qn = (uint32_t)__shfl((int)n, q);
			const uint32_t period = qd - qs;  // >= 1; a byte at or behind qd is the copy's own: KwKwK
			for (uint32_t o = lane; o < qn; o += 64) {
				uint32_t sidx = qs + o;
				if (sidx >= qd) sidx -= period;
				out[qd + o] = out[sidx];
			}
			__syncthreads();
		}
		const uint64_t np = (uint64_t)outpos + total;
		outpos = np < want ? (uint32_t)np : want;
		if (outpos >= want) { err = false; break; }   // the strip's bytes are out: whatever follows is ignored
		if (X < F) break;                              // a code beyond the table
		if (F == 64) {
			P += lzw_bits_of(jb + 63) - lzw_bits_of(jb - 1);
			jb += 64;
			continue;
		}
		const uint32_t fcode = (uint32_t)__shfl((int)code, (int)F), fw = (uint32_t)__shfl((int)w, (int)F);
		const uint32_t fbits = lzw_bits_of(jb + F - 1) - lzw_bits_of(jb - 1);
		const bool fhave = (sm >> F & 1) && P + fbits + fw <= nbits;
		if (!fhave || fcode != LZW_CLEAR) break;       // the data or an EOI ends the strip early
		P += fbits + fw;
		jb = 1;
	}
	// a strip opens with a Clear: the first iteration must have stopped at lane 0 on one (checked by replaying its first code)
	if (t.len < 2 || (((uint32_t)in[0] << 1) | ((uint32_t)in[1] >> 7)) != LZW_CLEAR) err = true;
	if (lane == 0) status[blockIdx.x] = err ? 1u : 0u;
}

// ---- gather and file layout ------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void tiff_gather_kernel(const uint8_t *files, const TiffStrip *strips, const uint64_t *offsets, uint8_t *dst)
{
	const TiffStrip t = strips[blockIdx.x];
	const uint8_t *s = files + t.src;
	uint8_t *d = dst + offsets[blockIdx.x];
	for (uint32_t k = threadIdx.x; k < t.len; k += blockDim.x) d[k] = s[k];
}

__device__ __forceinline__ void put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
__device__ __forceinline__ void put32(uint8_t *p, uint32_t v) { put16(p, v); put16(p + 2, v >> 16); }
__device__ __forceinline__ void put_tag(uint8_t *&p, uint32_t tag, uint32_t type, uint32_t count, uint32_t value)
{
	put16(p, tag); put16(p + 2, type); put32(p + 4, count);
	if (type == 3 && count == 1) { put16(p + 8, value); put16(p + 10, 0); }
	else put32(p + 8, value);
	p += 12;
}

// one workgroup per file: strip offsets by a scan of the sizes, then header, IFD and the two arrays.  libtiff types the byte
// counts of several strips before it knows them (tif_dirwrite.c, WriteAsLong4): SHORT (two of them inline in the entry) when
// ten times a full strip's bytes stay below 65535 -- a coded strip is taken for ten times its rows at worst --, else LONG;
// for uncompressed strips, SHORT when the strip's bytes fit.
__global__ __launch_bounds__(256) void tiff_layout_kernel(TiffPackArgs a)
{
	__shared__ uint32_t scratch[4];
	const uint32_t i = blockIdx.x, spf = a.spf;
	const uint32_t *sizes = a.src_sizes + (size_t)i * spf;
	uint32_t *soff = a.strip_off + (size_t)i * spf;
	uint8_t *f = a.out + (size_t)i * a.out_stride;
	uint32_t base = 8;
	for (uint32_t s0 = 0; s0 < spf; s0 += blockDim.x) {  // uniform bounds: every thread reaches the scan
		const uint32_t s = s0 + threadIdx.x;
		const uint32_t sz = s < spf ? sizes[s] - a.src_skip : 0;
		uint32_t total;
		const uint32_t ex = wg_excl_scan<4>(sz, scratch, total);
		if (s < spf) soff[s] = base + ex;
		base += total;
	}
	__syncthreads();  // soff[] of other threads
	const uint64_t full = (uint64_t)a.rps * a.cols * (a.bits / 8);
	const bool shorts = spf > 1 && (a.compression == 1 ? full <= 0xFFFFu : full < 0xFFFFu / 10);
	const uint32_t csize = shorts ? 2 : 4, inline_counts = csize * spf <= 4;
	const uint32_t ifd = base + (base & 1), ntags = a.predictor == 2 ? 10 : 9;
	const uint32_t counts_at = ifd + 2 + 12 * ntags + 4, offs_at = counts_at + (inline_counts ? 0 : csize * spf);
	if (spf > 1)
		for (uint32_t s = threadIdx.x; s < spf; s += blockDim.x) {
			if (!inline_counts) {
				if (shorts) put16(f + counts_at + 2 * (size_t)s, sizes[s] - a.src_skip);
				else put32(f + counts_at + 4 * (size_t)s, sizes[s] - a.src_skip);
			}
			put32(f + offs_at + 4 * (size_t)s, soff[s]);
		}
	if (threadIdx.x == 0) {
		f[0] = 'I'; f[1] = 'I'; put16(f + 2, 42); put32(f + 4, ifd);
		if (base & 1) f[base] = 0;
		uint8_t *p = f + ifd;
		put16(p, ntags); p += 2;
		put_tag(p, 256, 3, 1, a.cols);
		put_tag(p, 257, 3, 1, a.rows);
		put_tag(p, 258, 3, 1, a.bits);
		put_tag(p, 259, 3, 1, a.compression);
		put_tag(p, 262, 3, 1, 1);
		put_tag(p, 273, 4, spf, spf > 1 ? offs_at : 8);
		put_tag(p, 278, 3, 1, a.rps);
		if (spf == 1) put_tag(p, 279, 4, 1, sizes[0] - a.src_skip);
		else if (inline_counts) put_tag(p, 279, 3, 2, (sizes[0] - a.src_skip) | (sizes[1] - a.src_skip) << 16);  // two SHORTs, little-endian
		else put_tag(p, 279, shorts ? 3 : 4, spf, counts_at);
		put_tag(p, 284, 3, 1, 1);
		if (a.predictor == 2) put_tag(p, 317, 3, 1, 2);
		put32(p, 0);
		a.out_sizes[i] = spf > 1 ? offs_at + 4 * spf : counts_at;
	}
}

// one workgroup per strip: its coded bytes to their place in the file
__global__ __launch_bounds__(256) void tiff_place_kernel(TiffPackArgs a)
{
	const size_t k = blockIdx.x;
	const uint32_t len = a.src_sizes[k] - a.src_skip;
	const uint8_t *s = a.src + k * a.src_stride + a.src_skip;
	uint8_t *d = a.out + (k / a.spf) * a.out_stride + a.strip_off[k];
	for (uint32_t b = threadIdx.x; b < len; b += blockDim.x) d[b] = s[b];
}

}  // namespace

hipError_t launch_tiff_stage(const void *d_images, int n, int rows, int cols, int bps, int predictor, int rps, int spf, uint8_t *d_strips,
                             size_t strip_stride, uint32_t *d_strip_sizes, hipStream_t st)
{
	const dim3 grid((unsigned)((size_t)n * rows)), block(256);
	if (bps == 2)
		hipLaunchKernelGGL(tiff_stage_kernel<uint16_t>, grid, block, 0, st, (const uint16_t *)d_images, (uint32_t)rows, (uint32_t)cols,
		                   (uint32_t)predictor, (uint32_t)rps, (uint32_t)spf, d_strips, strip_stride, d_strip_sizes);
	else
		hipLaunchKernelGGL(tiff_stage_kernel<uint8_t>, grid, block, 0, st, (const uint8_t *)d_images, (uint32_t)rows, (uint32_t)cols,
		                   (uint32_t)predictor, (uint32_t)rps, (uint32_t)spf, d_strips, strip_stride, d_strip_sizes);
	return hipGetLastError();
}

hipError_t launch_tiff_lzw_encode(const uint8_t *d_strips, size_t strip_stride, const uint32_t *d_in_sizes, int nstrips, uint8_t *d_out,
                                  size_t out_stride, uint32_t *d_out_sizes, hipStream_t st)
{
	hipLaunchKernelGGL(tiff_lzw_encode_kernel, dim3((unsigned)nstrips), dim3(64), 0, st, d_strips, strip_stride, d_in_sizes, d_out, out_stride,
	                   d_out_sizes);
	return hipGetLastError();
}

hipError_t launch_tiff_pack(const TiffPackArgs &a, int n, hipStream_t st)
{
	hipLaunchKernelGGL(tiff_layout_kernel, dim3((unsigned)n), dim3(256), 0, st, a);
	hipLaunchKernelGGL(tiff_place_kernel, dim3((unsigned)((size_t)n * a.spf)), dim3(256), 0, st, a);
	return hipGetLastError();
}

hipError_t launch_tiff_gather(const uint8_t *d_files, const TiffStrip *d_strips, uint32_t nstrips, const uint64_t *d_offsets, uint8_t *d_dst,
                              hipStream_t st)
{
	hipLaunchKernelGGL(tiff_gather_kernel, dim3(nstrips), dim3(256), 0, st, d_files, d_strips, d_offsets, d_dst);
	return hipGetLastError();
}

hipError_t launch_tiff_lzw_decode(const uint8_t *d_files, const TiffStrip *d_strips, uint32_t nstrips, uint8_t *d_decoded, uint32_t *d_status,
                                  hipStream_t st)
{
	hipLaunchKernelGGL(tiff_lzw_decode_kernel, dim3(nstrips), dim3(64), 0, st, d_files, d_strips, d_decoded, d_status);
	return hipGetLastError();
}

hipError_t launch_tiff_unpredict(const uint8_t *d_files, const uint8_t *d_decoded, const TiffStrip *d_strips, uint32_t nstrips, int rows,
                                 int cols, int bps, void *d_images, hipStream_t st)
{
	if (bps == 2)
		hipLaunchKernelGGL(tiff_unpredict_kernel<uint16_t>, dim3(nstrips), dim3(256), 0, st, d_files, d_decoded, d_strips, (uint32_t)rows,
		                   (uint32_t)cols, (uint16_t *)d_images);
	else
		hipLaunchKernelGGL(tiff_unpredict_kernel<uint8_t>, dim3(nstrips), dim3(256), 0, st, d_files, d_decoded, d_strips, (uint32_t)rows,
		                   (uint32_t)cols, (uint8_t *)d_images);
	return hipGetLastError();
}

}  // namespace cct
