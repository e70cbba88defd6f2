// JPEG Lossless (ITU-T T.81 process 14: SOF3, Huffman) for one component of precision 2 .. 16: the device side of
// cct_jpegll_encode_batch / cct_jpegll_decode_batch (api_jpeg_lossless.cpp).  tests/jpeg_lossless_model.py is the CPU
// restatement of both directions.
//
// ENCODE (selection value 1 .. 7 for the call, or 0: every frame its cheapest; no point transform).  A sample's difference
// to its prediction, modulo 2^16, falls into one of 17 categories; the frame's Huffman code for the category and the
// category's extra bits make at most 31 bits a sample.  The selection value is a template parameter of kernels 1 and 3.
//   1 hist    differences and a 17-bin histogram per frame, bins replicated 32 times in LDS; flags samples >= 2^P.  With
//             predictor 0 the seven histograms of the seven selection values, from the same read
//   2 table   one lane per frame (per frame and candidate) runs Annex K.2 (merge the two rarest, ties to the larger
//             symbol; limit to 16 bits; drop the reserved code) and leaves BITS, HUFFVAL and the code of every category
//     pick    predictor 0 only, one lane per frame: the candidate with the fewest coded bits, ties to the lowest
//   3 emit    a workgroup per restart interval, 1024 samples a step, 4 per lane: a block scan of the lanes' bit counts
//             places every sample, atomic ORs assemble the bits in LDS, whole words go to the interval's slot of bitbuf
//             and the partial word is carried into the next step; counts the interval's bytes and how many are 0xFF
//   4 layout  one lane per frame sums the interval sizes into file offsets and writes the headers and EOI
//   5 stuff   a workgroup per interval copies the bytes to their place, a 0x00 behind every 0xFF, RSTm in front
// The raster is read twice (1 and 3), with predictor 0 too.
//
// DECODE.  Where a code word starts is known only once every one before it has been read.
//   1 unstuff   a workgroup per frame drops the stuffed zeros, fill bytes and RST markers (a 0xFF is data only when a 0x00
//               follows), notes where every interval starts and checks the RST sequence
//   2 huffman   a workgroup per interval, a lane per subsequence of JPL_SUB bits.  Every lane decodes from its guess of
//               its entry bit to the end of its subsequence; then, a window of 256 subsequences at a time and in order,
//               the landing of the predecessor becomes the entry and lanes whose entry moved decode again, until nothing
//               in the window moves: the window's first entry is right, so by induction all are.  A scan of the sample
//               counts gives every subsequence its place, and a last decode writes the differences.  Samples behind the
//               interval's count (pad bits read as codes) are dropped.
//   3 rows      predictor 1: a workgroup per row sums column 0 of the interval's earlier rows, then scans its row
//     generic   predictors 2 .. 7: a workgroup per interval sweeps the anti-diagonals
// Every index is bounded by (rows, cols) or by a length the host measured, never by file content: see JplEncArgs and the
// comments at each kernel.
#include <algorithm>

#include "cct_internal.h"
#include "wave_device.h"
#include "../../include/compact_hip.h"

namespace cct {
namespace {

// ---- encode ---------------------------------------------------------------------------------------------------------

// T.81 Table H.1 in 32-bit signed arithmetic, >> an arithmetic shift: selection values 4 .. 6 may leave 0 .. 65535, the
// difference is masked to 16 bits behind
__device__ __forceinline__ int jpl_predict(uint32_t ss, int ra, int rb, int rc)
{
	switch (ss) {
	case 1: return ra;
	case 2: return rb;
	case 3: return rc;
	case 4: return ra + rb - rc;
	case 5: return ra + ((rb - rc) >> 1);
	case 6: return rb + ((ra - rc) >> 1);
	default: return (ra + rb) >> 1;
	}
}

// difference of sample g (column c, the i-th of its interval) to its prediction, modulo 2^16.  H.1.2: the interval's first
// sample is predicted by init, the rest of its first row by Ra, column 0 of a later row by Rb, whatever ss says.  ss = 1 is
// the statement it was before the other six came.
template <typename Px>
__device__ __forceinline__ uint32_t jpl_diff(const Px *img, uint32_t g, uint32_t c, uint32_t i, uint32_t cols, uint32_t init, uint32_t ss)
{
	if (ss == 1) {
		const uint32_t pred = i == 0 ? init : (c == 0 ? (uint32_t)img[g - cols] : (uint32_t)img[g - 1]);
		return ((uint32_t)img[g] - pred) & 0xFFFFu;
	}
	int pred;
	if (i < cols) pred = i == 0 ? (int)init : (int)img[g - 1];
	else if (c == 0) pred = (int)img[g - cols];
	else pred = jpl_predict(ss, (int)img[g - 1], (int)img[g - cols], (int)img[g - cols - 1]);
	return (uint32_t)((int)img[g] - pred) & 0xFFFFu;
}

__device__ __forceinline__ uint32_t jpl_category(uint32_t d, uint32_t &extra)
{
	extra = 0;
	if (d == 0) return 0;
	if (d == 0x8000u) return 16;
	const int sd = (int)(int16_t)(uint16_t)d;
	const uint32_t a = (uint32_t)(sd < 0 ? -sd : sd);
	const uint32_t c = 32u - (uint32_t)__clz((int)a);
	extra = (uint32_t)(sd < 0 ? sd - 1 : sd) & ((1u << c) - 1u);
	return c;
}

// SS 1 .. 7: the frame's histogram under that selection value.  SS 0: the seven of them from one read of the raster, Ra, Rb
// and Rc loaded once per sample; NC * 17 bins, each replicated 32 times, 15 232 bytes of LDS for the seven.
template <typename Px, uint32_t SS>
__global__ void __launch_bounds__(256) jpl_hist_kernel(JplEncArgs a, uint32_t bpf)
{
	constexpr uint32_t NC = SS ? 1u : JPL_NCAND;
	__shared__ uint32_t h[NC * 17 * 32];
	__shared__ uint32_t over;
	const uint32_t t = threadIdx.x, frame = blockIdx.x / bpf, b = blockIdx.x % bpf;
	const uint32_t N = a.rows * a.cols, isz = a.rpi * a.cols;
	const Px *img = (const Px *)a.images + (size_t)frame * N;
	for (uint32_t i = t; i < NC * 17 * 32; i += 256) h[i] = 0;
	if (t == 0) over = 0;
	__syncthreads();
	bool ov = false;
	for (uint32_t g = b * 256u + t; g < N; g += bpf * 256u) {
		ov |= ((uint32_t)img[g] >> a.precision) != 0;
		uint32_t extra;
		if (SS) {
			const uint32_t cat = jpl_category(jpl_diff(img, g, g % a.cols, g % isz, a.cols, 1u << (a.precision - 1), SS), extra);
			atomicAdd(&h[cat * 32 + (t & 31u)], 1u);
		} else {
			const uint32_t c = g % a.cols, i = g % isz;
			const int x = (int)img[g];
			if (i < a.cols || c == 0) {  // one prediction for all seven
				const int pred = i == 0 ? (int)(1u << (a.precision - 1)) : (int)img[c == 0 ? g - a.cols : g - 1];
				const uint32_t cat = jpl_category((uint32_t)(x - pred) & 0xFFFFu, extra);
				for (uint32_t k = 0; k < NC; k++) atomicAdd(&h[(k * 17 + cat) * 32 + (t & 31u)], 1u);
			} else {
				const int ra = (int)img[g - 1], rb = (int)img[g - a.cols], rc = (int)img[g - a.cols - 1];
#pragma unroll
				for (uint32_t k = 0; k < NC; k++) {
					const uint32_t cat = jpl_category((uint32_t)(x - jpl_predict(k + 1, ra, rb, rc)) & 0xFFFFu, extra);
					atomicAdd(&h[(k * 17 + cat) * 32 + (t & 31u)], 1u);
				}
			}
		}
	}
	if (ov) atomicOr(&over, 1u);
	__syncthreads();
	if (t < NC * 17) {
		uint32_t s = 0;
		for (uint32_t k = 0; k < 32; k++) s += h[t * 32 + k];
		if (s) atomicAdd(&a.hist[frame * (NC * 17) + t], s);
	}
	if (t == 0 && over) atomicOr(&a.status[frame], JPL_ST_OVERFLOW);
}

// Annex K.2 over the 17 categories and the reserved symbol (index 17, the largest), one lane per table: per frame, or per
// (frame, candidate) of the a.n * a.ncand that predictor 0 weighs.  A fixed predictor is the frame's selection value here.
__global__ void __launch_bounds__(64) jpl_table_kernel(JplEncArgs a)
{
	const uint32_t frame = blockIdx.x * 64u + threadIdx.x;  // the table's index: frame * ncand + candidate
	if (frame >= a.n * a.ncand) return;
	if (a.predictor) a.sel[frame] = a.predictor;
	uint32_t freq[18];
	int codesize[18], others[18];
	for (int i = 0; i < 17; i++) freq[i] = a.hist[frame * 17 + i];
	freq[17] = 1;
	for (int i = 0; i < 18; i++) { codesize[i] = 0; others[i] = -1; }
	for (;;) {
		int c1 = -1, c2 = -1;
		uint32_t v = 0xFFFFFFFFu;
		for (int i = 0; i < 18; i++) if (freq[i] && freq[i] <= v) { v = freq[i]; c1 = i; }
		v = 0xFFFFFFFFu;
		for (int i = 0; i < 18; i++) if (freq[i] && freq[i] <= v && i != c1) { v = freq[i]; c2 = i; }
		if (c2 < 0) break;
		freq[c1] += freq[c2];
		freq[c2] = 0;
		codesize[c1]++;
		while (others[c1] >= 0) { c1 = others[c1]; codesize[c1]++; }
		others[c1] = c2;
		codesize[c2]++;
		while (others[c2] >= 0) { c2 = others[c2]; codesize[c2]++; }
	}
	int bits[33];
	for (int i = 0; i < 33; i++) bits[i] = 0;
	for (int i = 0; i < 18; i++) if (codesize[i]) bits[codesize[i]]++;  // 18 leaves: no code is longer than 17
	for (int i = 32; i > 16; i--)
		while (bits[i] > 0) {
			int j = i - 2;
			while (bits[j] == 0) j--;
			bits[i] -= 2; bits[i - 1]++; bits[j + 1] += 2; bits[j]--;
		}
	int i = 16;
	while (bits[i] == 0) i--;
	bits[i]--;
	JplCode &c = a.codes[frame];
	uint32_t nval = 0;
	for (int ln = 1; ln <= 17; ln++)
		for (int s = 0; s < 17; s++)
			if (codesize[s] == ln) c.huffval[nval++] = (uint8_t)s;  // at most 17 symbols have a size
	c.nval = (uint8_t)nval;
	for (int s = 0; s < 17; s++) { c.size[s] = 0; c.code[s] = 0; }
	uint32_t code = 0, k = 0;
	for (int ln = 1; ln <= 16; ln++) {
		c.bits[ln - 1] = (uint8_t)bits[ln];
		for (int q = 0; q < bits[ln] && k < nval; q++, k++) { c.size[c.huffval[k]] = (uint8_t)ln; c.code[c.huffval[k]] = (uint16_t)code++; }
		code <<= 1;
	}
}

// predictor 0, one lane per frame: the candidate whose table codes its histogram in the fewest bits, the HUFFVAL bytes of
// its DHT counted in (unstuffed bits and no pad bits: an estimate of the file, not its size); ties go to the lowest
// selection value.  The winner's table moves to the frame's first slot, where the emit and layout kernels read it.
__global__ void __launch_bounds__(64) jpl_pick_kernel(JplEncArgs a)
{
	const uint32_t frame = blockIdx.x * 64u + threadIdx.x;
	if (frame >= a.n) return;
	uint32_t best = 0;
	uint64_t best_cost = ~0ull;
	for (uint32_t k = 0; k < JPL_NCAND; k++) {
		const JplCode &c = a.codes[frame * JPL_NCAND + k];
		const uint32_t *hist = a.hist + (size_t)(frame * JPL_NCAND + k) * 17u;
		uint64_t cost = 8u * (uint32_t)c.nval;
		for (uint32_t s = 0; s < 17; s++) cost += (uint64_t)hist[s] * ((uint32_t)c.size[s] + (s < 16 ? s : 0u));
		if (cost < best_cost) { best_cost = cost; best = k; }
	}
	a.sel[frame] = best + 1u;
	if (best) a.codes[frame * JPL_NCAND] = a.codes[frame * JPL_NCAND + best];
}

// nb bits of val at bit p of the LDS words w (bit 0 is the top bit of w[0]); nb <= 31, so two words at most
__device__ __forceinline__ void jpl_put(uint32_t *w, uint32_t p, uint32_t val, uint32_t nb)
{
	const uint64_t v = (uint64_t)val << (64u - nb - (p & 31u));
	atomicOr(&w[p >> 5], (uint32_t)(v >> 32));
	if ((uint32_t)v) atomicOr(&w[(p >> 5) + 1u], (uint32_t)v);
}

__device__ __forceinline__ uint32_t jpl_ff_bytes(uint32_t v, uint32_t nbytes)  // 0xFF among the top nbytes bytes of v
{
	uint32_t n = 0;
	for (uint32_t k = 0; k < nbytes; k++) n += ((v >> (24u - 8u * k)) & 0xFFu) == 0xFFu;
	return n;
}

// A workgroup per interval.  LDS words: a step adds at most 1024 * 31 bits to a carry of at most 31, 993 words and the one
// jpl_put may touch behind.  bitbuf: the interval's slot has a word per sample and its bits fit 31 per sample, so the
// ceil(bits / 32) words written stay inside the slot.  SS 1 .. 7: that selection value; SS 0: the frame's own, sel[frame].
template <typename Px, uint32_t SS>
__global__ void __launch_bounds__(256) jpl_emit_kernel(JplEncArgs a)
{
	__shared__ uint32_t w[JPL_CHUNK + 8];
	__shared__ uint32_t scan[4];  // wg_excl_scan: a word per wave
	__shared__ uint32_t s_ff;
	__shared__ uint8_t l_size[17];
	__shared__ uint16_t l_code[17];
	const uint32_t t = threadIdx.x, frame = blockIdx.x / a.n_int, k = blockIdx.x % a.n_int;
	const uint32_t N = a.rows * a.cols, r0 = k * a.rpi, nrows = min(a.rpi, a.rows - r0), ns = nrows * a.cols, g0 = r0 * a.cols;
	const Px *img = (const Px *)a.images + (size_t)frame * N;
	uint32_t *dst = a.bitbuf + (size_t)frame * N + g0;
	const uint32_t ss = SS ? SS : a.sel[frame];
	const JplCode &code = a.codes[SS ? frame : frame * JPL_NCAND];
	if (t < 17) { l_size[t] = code.size[t]; l_code[t] = code.code[t]; }
	if (t == 0) { s_ff = 0; w[0] = 0; }
	__syncthreads();
	uint32_t carry_bits = 0, words_out = 0, ff = 0, nbytes = 0;
	for (uint32_t base = 0; base < ns; base += JPL_CHUNK) {
		for (uint32_t i = 1 + t; i < JPL_CHUNK + 8; i += 256) w[i] = 0;
		uint32_t val[4], nb[4], sum = 0;
		const uint32_t i0 = base + t * 4u;
		uint32_t c = i0 < ns ? (g0 + i0) % a.cols : 0u;
#pragma unroll
		for (int j = 0; j < 4; j++) {
			val[j] = 0; nb[j] = 0;
			if (i0 + j < ns) {
				uint32_t extra;
				const uint32_t cat = jpl_category(jpl_diff(img, g0 + i0 + j, c, i0 + j, a.cols, 1u << (a.precision - 1), ss), extra);
				const uint32_t nx = cat == 16 ? 0u : cat;
				val[j] = ((uint32_t)l_code[cat] << nx) | extra;
				nb[j] = (uint32_t)l_size[cat] + nx;
				if (++c == a.cols) c = 0;
			}
			sum += nb[j];
		}
		uint32_t total;
		uint32_t p = carry_bits + wg_excl_scan<4>(sum, scan, total);  // its barriers also put the clears before the ORs
#pragma unroll
		for (int j = 0; j < 4; j++) {
			if (nb[j]) jpl_put(w, p, val[j], nb[j]);
			p += nb[j];
		}
		__syncthreads();
		uint32_t tot = carry_bits + total;
		const bool last = base + JPL_CHUNK >= ns;
		if (last && (tot & 7u)) {  // pad the interval to a byte with ones
			if (t == 0) jpl_put(w, tot, (1u << (8u - (tot & 7u))) - 1u, 8u - (tot & 7u));
			tot += 8u - (tot & 7u);
			__syncthreads();
		}
		const uint32_t full = last ? (tot + 31u) >> 5 : tot >> 5;
		for (uint32_t i = t; i < full; i += 256) {
			const uint32_t v = w[i];
			dst[words_out + i] = v;
			ff += jpl_ff_bytes(v, (last && i == full - 1u && (tot & 31u)) ? (tot & 31u) >> 3 : 4u);
		}
		const uint32_t cw = last ? 0u : w[full];
		__syncthreads();
		if (t == 0) w[0] = cw;
		if (last) nbytes = words_out * 4u + (tot >> 3);
		words_out += full;
		carry_bits = tot & 31u;
	}
	if (ff) atomicAdd(&s_ff, ff);
	__syncthreads();
	if (t == 0) { a.ibytes[blockIdx.x] = nbytes; a.iff[blockIdx.x] = s_ff; }
}

__device__ __forceinline__ void jpl_be16(uint8_t *&p, uint32_t v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; }

// one lane per frame: the headers, every interval's offset, EOI and the size.  The offsets sum bytes that bitbuf holds
// (ibytes <= ceil(31 * interval samples / 8), iff <= ibytes) and two per RST, which is how jpl_bound() counts.
__global__ void __launch_bounds__(64) jpl_layout_kernel(JplEncArgs a)
{
	const uint32_t frame = blockIdx.x * 64u + threadIdx.x;
	if (frame >= a.n) return;
	const JplCode &c = a.codes[frame * a.ncand];
	uint8_t *f = a.out + (size_t)frame * a.out_stride, *p = f;
	*p++ = 0xFF; *p++ = 0xD8;
	*p++ = 0xFF; *p++ = 0xC3; jpl_be16(p, 11); *p++ = (uint8_t)a.precision; jpl_be16(p, a.rows); jpl_be16(p, a.cols);
	*p++ = 1; *p++ = 1; *p++ = 0x11; *p++ = 0;
	*p++ = 0xFF; *p++ = 0xC4; jpl_be16(p, 19u + c.nval); *p++ = 0;
	for (int i = 0; i < 16; i++) *p++ = c.bits[i];
	for (uint32_t i = 0; i < c.nval && i < 17; i++) *p++ = c.huffval[i];
	if (a.restart) { *p++ = 0xFF; *p++ = 0xDD; jpl_be16(p, 4); jpl_be16(p, a.rpi * a.cols); }
	*p++ = 0xFF; *p++ = 0xDA; jpl_be16(p, 8); *p++ = 1; *p++ = 1; *p++ = 0; *p++ = (uint8_t)a.sel[frame]; *p++ = 0; *p++ = 0;
	uint32_t off = (uint32_t)(p - f);
	for (uint32_t k = 0; k < a.n_int; k++) {
		if (k) off += 2;
		a.ioff[frame * a.n_int + k] = off;
		off += a.ibytes[frame * a.n_int + k] + a.iff[frame * a.n_int + k];
	}
	f[off] = 0xFF; f[off + 1] = 0xD9;
	a.out_sizes[frame] = a.status[frame] ? 0u : off + 2u;
}

// a workgroup per interval: 1024 bytes a step, a word per lane
__global__ void __launch_bounds__(256) jpl_stuff_kernel(JplEncArgs a)
{
	__shared__ uint32_t scan[4];  // wg_excl_scan: a word per wave
	const uint32_t t = threadIdx.x, frame = blockIdx.x / a.n_int, k = blockIdx.x % a.n_int;
	const uint32_t N = a.rows * a.cols, nbytes = a.ibytes[blockIdx.x];
	const uint32_t *src = a.bitbuf + (size_t)frame * N + k * a.rpi * a.cols;
	uint8_t *dst = a.out + (size_t)frame * a.out_stride + a.ioff[blockIdx.x];
	if (k && t == 0) { dst[-2] = 0xFF; dst[-1] = (uint8_t)(0xD0u + ((k - 1u) & 7u)); }
	uint32_t ff_before = 0;
	for (uint32_t base = 0; base < nbytes; base += 1024) {
		const uint32_t j0 = base + t * 4u, nv = j0 < nbytes ? min(4u, nbytes - j0) : 0u;
		const uint32_t v = nv ? src[j0 >> 2] : 0u;
		uint32_t total;
		uint32_t o = j0 + ff_before + wg_excl_scan<4>(jpl_ff_bytes(v, nv), scan, total);
		for (uint32_t q = 0; q < nv; q++) {
			const uint32_t b = (v >> (24u - 8u * q)) & 0xFFu;
			dst[o++] = (uint8_t)b;
			if (b == 0xFFu) dst[o++] = 0;
		}
		ff_before += total;
	}
}

// ---- decode ---------------------------------------------------------------------------------------------------------

// A workgroup per frame, 2048 bytes a step, 8 per lane.  Reads src[0 .. len]: byte len is the 0xFF of the marker behind the
// scan.  Kept bytes go to ubuf at the frame's own offset, and there are at most len of them.  An interval start is stored
// only at index 1 .. n_int - 1 of the frame's n_int + 1 entries.
__global__ void __launch_bounds__(256) jpl_unstuff_kernel(JplDecArgs a)
{
	__shared__ uint32_t scan[4];  // wg_excl_scan: a word per wave
	__shared__ uint32_t s_bad;
	const uint32_t t = threadIdx.x, fi = blockIdx.x;
	const JplFrame &f = a.frames[fi];
	const uint8_t *src = a.files + f.src;
	uint8_t *dst = a.ubuf + f.src;
	uint32_t *ist = a.istart + f.int0 + fi;
	const uint32_t len = f.len, n_int = f.n_int;
	if (t == 0) s_bad = 0;
	__syncthreads();
	uint32_t kept = 0, rsts = 0, bad = 0;
	for (uint32_t base = 0; base < len; base += 2048) {
		const uint32_t i0 = base + t * 8u, nv = i0 < len ? min(8u, len - i0) : 0u;
		uint32_t by[10];  // bytes i0 - 1 .. i0 + 8
		for (uint32_t q = 0; q < 10; q++) {
			const uint32_t i = i0 + q;  // index + 1
			by[q] = (nv && i >= 1u && i - 1u <= len) ? src[i - 1u] : 0u;
		}
		uint32_t keepm = 0, rstm = 0;
		for (uint32_t q = 0; q < nv; q++) {
			const uint32_t pv = by[q], b = by[q + 1], nx = by[q + 2];
			const bool after_ff = pv == 0xFFu, is_rst = after_ff && b >= 0xD0u && b <= 0xD7u;
			const bool keep = !(b == 0xFFu && nx != 0u) && !(after_ff && (b == 0u || is_rst));
			keepm |= (uint32_t)keep << q;
			rstm |= (uint32_t)is_rst << q;
		}
		uint32_t total;
		const uint32_t ex = wg_excl_scan<4>((uint32_t)__popc(keepm) | (uint32_t)__popc(rstm) << 16, scan, total);
		uint32_t o = kept + (ex & 0xFFFFu), r = rsts + (ex >> 16);
		for (uint32_t q = 0; q < nv; q++) {
			if (keepm >> q & 1u) dst[o++] = (uint8_t)by[q + 1];
			if (rstm >> q & 1u) {
				if (by[q + 1] - 0xD0u != (r & 7u)) bad = 1;
				if (r + 1u < n_int) ist[r + 1u] = o; else bad = 1;
				r++;
			}
		}
		kept += total & 0xFFFFu;
		rsts += total >> 16;
	}
	if (rsts + 1u != n_int) bad = 1;
	if (bad) atomicOr(&s_bad, 1u);
	__syncthreads();
	if (t == 0) {
		ist[0] = 0;
		ist[n_int] = kept;
		if (s_bad) atomicOr(&a.status[fi], JPL_ST_STREAM | JPL_ST_INTERVALS);
	}
}

struct JplLds { int32_t maxcode[17], delta[17]; uint8_t huffval[20]; };

// 32 bits from bit `pos` of p[0 .. nbytes), zeros behind the end
__device__ __forceinline__ uint32_t jpl_peek(const uint8_t *p, uint32_t nbytes, uint32_t pos)
{
	const uint32_t by = pos >> 3;
	uint64_t v = 0;
#pragma unroll
	for (uint32_t j = 0; j < 5; j++) v = v << 8 | (by + j < nbytes ? (uint64_t)p[by + j] : 0ull);
	return (uint32_t)(v >> (8u - (pos & 7u)));
}

// Decodes the samples that start in [start, end) of an interval.  A code outside the table takes 16 bits and counts as a
// sample (so that every pass walks alike); with WRITE it is an error if the sample is one the interval needs, and so is a
// sample that runs past the data.  WRITE stores at out[oidx + i] only for oidx + i < need.
template <bool WRITE>
__device__ __forceinline__ void jpl_run(const JplLds &T, const uint8_t *data, uint32_t nbytes, uint32_t start, uint32_t end, uint32_t &land,
                                        uint32_t &cnt, uint16_t *out, uint32_t oidx, uint32_t need, uint32_t &err, uint32_t *end_bit)
{
	uint32_t pos = start, n = 0;
	while (pos < end) {
		const uint32_t w = jpl_peek(data, nbytes, pos);
		uint32_t ln = 1, d = 0;
		bool found = false;
		for (; ln <= 16; ln++) {
			const int32_t code = (int32_t)(w >> (32u - ln));
			if (code <= T.maxcode[ln]) { found = true; break; }
		}
		if (found) {
			const uint32_t s = T.huffval[(w >> (32u - ln)) + T.delta[ln]];
			if (s == 16) d = 0x8000u;
			else if (s) {
				const uint32_t v = (w << ln) >> (32u - s);
				d = (v < (1u << (s - 1u)) ? v - ((1u << s) - 1u) : v) & 0xFFFFu;
				ln += s;
			}
		} else ln = 16;
		pos += ln;
		if (WRITE && oidx + n < need) {
			if (!found || pos > nbytes * 8u) err = 1;
			out[oidx + n] = (uint16_t)d;
			if (oidx + n == need - 1u) *end_bit = pos;
		}
		n++;
	}
	land = pos;
	cnt = n;
}

// A workgroup per interval.  The interval's subsequence entries are sub0 + floor(8 * start / JPL_SUB) + k onwards:
// ceil(8 * bytes / JPL_SUB) of them, which stay below the next interval's first entry and, summed, below the host's count
// floor(8 * len / JPL_SUB) + n_int.  Differences go to the interval's rows of the frame's slot of diff.
__global__ void __launch_bounds__(256) jpl_huffman_kernel(JplDecArgs a)
{
	__shared__ JplLds T;
	__shared__ uint32_t scan[4];  // wg_excl_scan: a word per wave
	__shared__ uint32_t s_end, s_err;
	const uint32_t t = threadIdx.x, fi = a.int_frame[blockIdx.x];
	const JplFrame &f = a.frames[fi];
	if (a.status[fi] & JPL_ST_INTERVALS) return;  // no interval starts to trust.  Only jpl_unstuff_kernel, a launch earlier, sets this bit: uniform
	const uint32_t k = blockIdx.x - f.int0;
	const uint32_t *ist = a.istart + f.int0 + fi;
	const uint32_t b0 = ist[k], nbytes = ist[k + 1] - b0, nbits = nbytes * 8u;
	const uint8_t *data = a.ubuf + f.src + b0;
	const uint32_t r0 = k * f.rpi, need = min(f.rpi, a.rows - r0) * a.cols;
	uint16_t *out = a.diff + (size_t)f.slot * a.rows * a.cols + (size_t)r0 * a.cols;
	const uint32_t nsub = (nbits + JPL_SUB - 1u) / JPL_SUB;
	const uint32_t sb = f.sub0 + (uint32_t)(((uint64_t)b0 * 8u) / JPL_SUB) + k;
	uint32_t *st = a.sub_start + sb, *la = a.sub_land + sb, *cn = a.sub_cnt + sb;
	if (t < 17) { T.maxcode[t] = f.maxcode[t]; T.delta[t] = f.delta[t]; }
	if (t < 20) T.huffval[t] = f.huffval[t];
	if (t == 0) { s_end = 0xFFFFFFFFu; s_err = 0; }
	__syncthreads();
	uint32_t err = 0, dummy = 0;
	for (uint32_t s = t; s < nsub; s += 256) {
		st[s] = s * JPL_SUB;
		jpl_run<false>(T, data, nbytes, s * JPL_SUB, min((s + 1u) * JPL_SUB, nbits), la[s], cn[s], nullptr, 0, 0, dummy, nullptr);
	}
	// Windows of 256 subsequences, a lane each, in order.  The entry of the window's first subsequence is final (0, or the
	// landing of a subsequence of the window before, which is final).  A round that moves no entry proves the window: every
	// entry equals its predecessor's landing, so by induction all are right.  A round that moves one leaves at least one more
	// subsequence of the window final, so a window takes 256 rounds of one decode per lane at most and the loop as many
	// decodes per lane as the interval has subsequences: linear in the interval even for a stream that never resynchronises.
	for (uint32_t w0 = 0; w0 < nsub;) {
		__syncthreads();
		const uint32_t q = w0 + t;
		bool dirty = false;
		if (q > 0 && q < nsub) {
			const uint32_t e = la[q - 1u];
			if (e != st[q]) { st[q] = e; dirty = true; }
		}
		__syncthreads();
		if (dirty) jpl_run<false>(T, data, nbytes, st[q], min((q + 1u) * JPL_SUB, nbits), la[q], cn[q], nullptr, 0, 0, dummy, nullptr);
		if (!__syncthreads_or(dirty ? 1 : 0)) w0 += 256;
	}
	// every subsequence's place: its samples start at the sum of the counts before it (kept in `la`, no longer needed)
	uint32_t running = 0;
	for (uint32_t base = 0; base < nsub; base += 256) {
		const uint32_t s = base + t, c = s < nsub ? cn[s] : 0u;
		uint32_t total;
		const uint32_t ex = wg_excl_scan<4>(c, scan, total);
		if (s < nsub) la[s] = running + ex;
		running += total;
	}
	__syncthreads();
	for (uint32_t s = t; s < nsub; s += 256) {
		uint32_t l2, c2;
		if (la[s] < need) jpl_run<true>(T, data, nbytes, st[s], min((s + 1u) * JPL_SUB, nbits), l2, c2, out, la[s], need, err, &s_end);
	}
	if (err) atomicOr(&s_err, 1u);
	__syncthreads();
	if (t == 0) {
		// fewer samples than the interval needs, or whole bytes left behind the last one
		if (s_err || running < need || s_end == 0xFFFFFFFFu || (s_end + 7u) >> 3 != nbytes) atomicOr(&a.status[fi], JPL_ST_STREAM);
	}
}

// predictor 1: a workgroup per row of a frame.  x[r][c] = init + (column 0 of the interval's rows above) + d[r][0 .. c].
template <typename Out>
__global__ void __launch_bounds__(256) jpl_rows_kernel(JplDecArgs a)
{
	__shared__ uint32_t scan[4];  // wg_excl_scan: a word per wave
	__shared__ uint32_t s_base;
	const uint32_t t = threadIdx.x, fi = blockIdx.x / a.rows, r = blockIdx.x % a.rows;
	const JplFrame &f = a.frames[fi];
	if (f.ss != 1 || a.status[fi]) return;
	const uint32_t cols = a.cols, rtop = r / f.rpi * f.rpi;
	const uint16_t *d = a.diff + (size_t)f.slot * a.rows * cols;
	Out *out = (Out *)a.images + (size_t)f.slot * a.rows * cols + (size_t)r * cols;
	if (t == 0) s_base = f.init;
	__syncthreads();
	uint32_t part = 0;
	for (uint32_t q = rtop + t; q < r; q += 256) part += d[(size_t)q * cols];
	if (part) atomicAdd(&s_base, part);
	__syncthreads();
	uint32_t running = s_base;
	d += (size_t)r * cols;
	for (uint32_t c0 = 0; c0 < cols; c0 += 1024) {
		const uint32_t i0 = c0 + t * 4u;
		uint32_t v[4], sum = 0;
		for (uint32_t j = 0; j < 4; j++) { v[j] = i0 + j < cols ? (uint32_t)d[i0 + j] : 0u; sum += v[j]; }
		uint32_t total;
		uint32_t x = running + wg_excl_scan<4>(sum, scan, total);
		for (uint32_t j = 0; j < 4; j++) {
			x += v[j];
			if (i0 + j < cols) out[i0 + j] = (Out)((x & 0xFFFFu) << f.pt);
		}
		running += total;
	}
}

// predictors 2 .. 7: a workgroup per interval sweeps the anti-diagonals r + c = const of its rows; what a sample needs (left,
// above, above left) lies on the two diagonals before.  The samples replace the differences in `diff`, before the shift.
template <typename Out>
__global__ void __launch_bounds__(256) jpl_generic_kernel(JplDecArgs a)
{
	const uint32_t t = threadIdx.x, fi = a.int_frame[blockIdx.x];
	const JplFrame &f = a.frames[fi];
	if (f.ss == 1 || a.status[fi]) return;
	const uint32_t k = blockIdx.x - f.int0, cols = a.cols, r0 = k * f.rpi, nrows = min(f.rpi, a.rows - r0);
	uint16_t *x = a.diff + (size_t)f.slot * a.rows * cols + (size_t)r0 * cols;
	Out *out = (Out *)a.images + (size_t)f.slot * a.rows * cols + (size_t)r0 * cols;
	for (uint32_t g = 0; g < nrows + cols - 1u; g++) {
		const uint32_t rlo = g >= cols ? g - cols + 1u : 0u, rhi = min(nrows - 1u, g);
		for (uint32_t r = rlo + t; r <= rhi; r += 256) {
			const uint32_t c = g - r;
			const size_t at = (size_t)r * cols + c;
			int p;
			if (r == 0) p = c == 0 ? (int)f.init : (int)x[at - 1];
			else if (c == 0) p = (int)x[at - cols];
			else {
				const int ra = x[at - 1], rb = x[at - cols], rc = x[at - cols - 1];
				switch (f.ss) {
				case 2: p = rb; break;
				case 3: p = rc; break;
				case 4: p = ra + rb - rc; break;
				case 5: p = ra + ((rb - rc) >> 1); break;
				case 6: p = rb + ((ra - rc) >> 1); break;
				default: p = (ra + rb) >> 1; break;
				}
			}
			const uint32_t v = ((uint32_t)p + (uint32_t)x[at]) & 0xFFFFu;
			x[at] = (uint16_t)v;
			out[at] = (Out)(v << f.pt);
		}
		__syncthreads();
	}
}

// launches 1 .. 3 of the encoder for one selection value (SS 0: the seven candidates and the pick)
template <typename Px, uint32_t SS>
void jpl_encode_front(const JplEncArgs &a, uint32_t bpf, hipStream_t st)
{
	hipLaunchKernelGGL((jpl_hist_kernel<Px, SS>), dim3(a.n * bpf), dim3(256), 0, st, a, bpf);
	hipLaunchKernelGGL(jpl_table_kernel, dim3((a.n * a.ncand + 63u) / 64u), dim3(64), 0, st, a);
	if (SS == 0) hipLaunchKernelGGL(jpl_pick_kernel, dim3((a.n + 63u) / 64u), dim3(64), 0, st, a);
	hipLaunchKernelGGL((jpl_emit_kernel<Px, SS>), dim3(a.n * a.n_int), dim3(256), 0, st, a);
}

template <typename Px>
void jpl_encode_front(const JplEncArgs &a, uint32_t bpf, hipStream_t st)
{
	switch (a.predictor) {
	case 0: jpl_encode_front<Px, 0>(a, bpf, st); break;
	case 1: jpl_encode_front<Px, 1>(a, bpf, st); break;
	case 2: jpl_encode_front<Px, 2>(a, bpf, st); break;
	case 3: jpl_encode_front<Px, 3>(a, bpf, st); break;
	case 4: jpl_encode_front<Px, 4>(a, bpf, st); break;
	case 5: jpl_encode_front<Px, 5>(a, bpf, st); break;
	case 6: jpl_encode_front<Px, 6>(a, bpf, st); break;
	default: jpl_encode_front<Px, 7>(a, bpf, st); break;
	}
}

}  // namespace

hipError_t launch_jpl_encode(const JplEncArgs &a, hipStream_t st)
{
	const uint32_t N = a.rows * a.cols, bpf = std::min(64u, (N + 4095u) / 4096u);
	const dim3 per_frame((a.n + 63u) / 64u), per_int(a.n * a.n_int);
	if (a.predictor > 7u || a.ncand != (a.predictor ? 1u : JPL_NCAND)) return hipErrorInvalidValue;
	if (a.src_bits == 16) jpl_encode_front<uint16_t>(a, bpf, st);
	else jpl_encode_front<uint8_t>(a, bpf, st);
	hipLaunchKernelGGL(jpl_layout_kernel, per_frame, dim3(64), 0, st, a);
	hipLaunchKernelGGL(jpl_stuff_kernel, per_int, dim3(256), 0, st, a);
	return hipGetLastError();
}

hipError_t launch_jpl_decode(const JplDecArgs &a, hipStream_t st)
{
	hipLaunchKernelGGL(jpl_unstuff_kernel, dim3(a.nframes), dim3(256), 0, st, a);
	hipLaunchKernelGGL(jpl_huffman_kernel, dim3(a.total_int), dim3(256), 0, st, a);
	if (a.out_bits == 16) {
		hipLaunchKernelGGL(jpl_rows_kernel<uint16_t>, dim3(a.nframes * a.rows), dim3(256), 0, st, a);
		if (a.any_generic) hipLaunchKernelGGL(jpl_generic_kernel<uint16_t>, dim3(a.total_int), dim3(256), 0, st, a);
	} else {
		hipLaunchKernelGGL(jpl_rows_kernel<uint8_t>, dim3(a.nframes * a.rows), dim3(256), 0, st, a);
		if (a.any_generic) hipLaunchKernelGGL(jpl_generic_kernel<uint8_t>, dim3(a.total_int), dim3(256), 0, st, a);
	}
	return hipGetLastError();
}

}  // namespace cct
