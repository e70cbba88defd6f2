// JPEG-LS lossless (ITU-T T.87: SOF55, NEAR = 0, one component of precision 2 .. 16): the device side of
// cct_jpegls_encode_batch / cct_jpegls_decode_batch (api_jpeg_ls.cpp).  tests/jpeg_ls_model.py is the CPU restatement of both
// directions and the place where the format is written down.
//
// ENCODE.  In the lossless coder the neighbours Ra, Rb, Rc, Rd of a sample are input samples, so everything that does not
// depend on the adaptive state is known for a whole line at once.
//   1 code    one wave per restart interval, the interval's lines in order, 64 samples a step:
//             a  every lane: neighbours, gradients, context and sign, median prediction
//             b  the line's parse from two ballots, "all gradients zero" (a run may start here) and "equals the sample to the
//                left" (a run goes on): a loop over the runs of the step, not over its samples, the same in every lane.  The run
//                state (RUNindex, the two interruption contexts) lives in that loop; it is a chain of its own, apart from the
//                365 regular contexts.  A run's bits and its interruption sample's code land in the interruption sample's lane,
//                the bits of a run to the end of the line in the lane of the last column.
//             c  the regular samples, in order only within a context: until none is pending, the lowest pending lane of every
//                context claims it in LDS (atomicMin), reads (A, B, C, N), finishes the error, k and the code, writes the state
//                back and releases the claim.  A step takes as many rounds as its busiest context has samples.
//             d  a wave scan of the lengths places the codes (up to 64 bits of run, up to 64 of code per lane) in an LDS bit
//                buffer, atomic ORs assemble them
//             e  bit stuffing, wave-wide: 64 bytes at the current bit offset, a ballot for 0xFF, the bytes up to the first one
//                are taken, the next byte is 7 bits wide, again.  All-ones data takes two bytes a round: linear.
//             The stuffed bytes go to the interval's slot of a staging buffer.
//   2 layout  one lane per frame: headers, the offset of every interval, EOI, the size
//   3 place   a workgroup per interval copies its bytes to their place, RSTm in front
//
// DECODE.  A sample's context needs the decoded neighbours: a serial chain per interval by the format's definition.  One lane
// per interval, JLS_DEC_LANES of them a workgroup, each with its own column of the context tables in LDS and a bit reader
// that has the 7-bit rule inline; the neighbours are read back from the raster it writes.  Reads are bounded by the
// interval's bytes (behind them the reader supplies zeros and notes the error), stores by the interval's lines, loops by the
// samples of a line.
#include <algorithm>

#include "cct_internal.h"
#include "wave_device.h"
#include "../../include/compact_hip.h"

namespace cct {
namespace {

// J[i] of T.87 A.7.1.2, four bits each: 0 0 0 0 1 1 1 1 2 2 2 2 3 3 3 3 4 4 5 5 6 6 7 7 8 9 10 11 12 13 14 15
__device__ __forceinline__ uint32_t jls_j(uint32_t i)
{
	const uint64_t lo = 0x3333222211110000ull, hi = 0xFEDCBA9877665544ull;
	return (uint32_t)((i < 16u ? lo : hi) >> (4u * (i & 15u))) & 15u;
}

__device__ __forceinline__ int jls_quant(int d, const JlsParams &p)
{
	if (d <= -p.t3) return -4;
	if (d <= -p.t2) return -3;
	if (d <= -p.t1) return -2;
	if (d < 0) return -1;
	if (d == 0) return 0;
	if (d < p.t1) return 1;
	if (d < p.t2) return 2;
	if (d < p.t3) return 3;
	return 4;
}

// 1 .. 364 and the sign, or 0: run mode
__device__ __forceinline__ int jls_context(int ra, int rb, int rc, int rd, const JlsParams &p, int &sign)
{
	const int q = 81 * jls_quant(rd - rb, p) + 9 * jls_quant(rb - rc, p) + jls_quant(rc - ra, p);
	sign = q < 0 ? -1 : 1;
	return q < 0 ? -q : q;
}

__device__ __forceinline__ int jls_median(int ra, int rb, int rc)
{
	const int mn = min(ra, rb), mx = max(ra, rb);
	return rc >= mx ? mn : rc <= mn ? mx : ra + rb - rc;
}

// the regular contexts' update (A.6): B and N after the error e, C corrected
__device__ __forceinline__ void jls_update(uint32_t &A, int &B, int &C, int &N, int e, int reset)
{
	B += e;
	A += (uint32_t)(e < 0 ? -e : e);
	if (N == reset) {
		A >>= 1;
		N >>= 1;
		B = B >= 0 ? B >> 1 : -((1 - B) >> 1);
	}
	N++;
	if (B <= -N) {
		B += N;
		if (C > -128) C--;
		if (B <= -N) B = -N + 1;
	} else if (B > 0) {
		B -= N;
		if (C < 127) C++;
		if (B > 0) B = 0;
	}
}

// ---- encode ---------------------------------------------------------------------------------------------------------

// the writer's RANGE is a power of two
__device__ __forceinline__ int jls_reduce(int e, const JlsParams &p)
{
	e = (int)((uint32_t)e & (p.range - 1u));
	return e >= (int)(p.range >> 1) ? e - (int)p.range : e;
}

// Golomb(m, k, limit): k <= 16, so the value fits 17 bits and the length is at most limit - qbpp - 1 + k < 64 or limit
__device__ __forceinline__ void jls_golomb(uint32_t m, uint32_t k, uint32_t limit, const JlsParams &p, uint64_t &val, uint32_t &len)
{
	const uint32_t hi = m >> k, esc = limit - p.qbpp - 1u;
	if (hi < esc) {
		val = (1ull << k) | (m & ((1u << k) - 1u));
		len = hi + 1u + k;
	} else {
		val = (1ull << p.qbpp) | ((m - 1u) & ((1u << p.qbpp) - 1u));
		len = limit;
	}
}

// len bits (1 .. 64) of val at bit pos of the LDS words w (bit 0 is the top bit of w[0]): three words at most
__device__ __forceinline__ void jls_put(uint32_t *w, uint32_t pos, uint64_t val, uint32_t len)
{
	const uint64_t top = val << (64u - len);
	const uint32_t sh = pos & 31u, i = pos >> 5;
	const uint32_t a0 = (uint32_t)((top >> 32) >> sh), a1 = (uint32_t)(top >> sh), a2 = sh ? (uint32_t)(top << (32u - sh)) : 0u;
	if (a0) atomicOr(&w[i], a0);
	if (a1) atomicOr(&w[i + 1u], a1);
	if (a2) atomicOr(&w[i + 2u], a2);
}

// wd bits (1 .. 8) from bit o of w
__device__ __forceinline__ uint32_t jls_bits(const uint32_t *w, uint32_t o, uint32_t wd)
{
	const uint64_t v = (uint64_t)w[o >> 5] << 32 | w[(o >> 5) + 1u];
	return (uint32_t)(v >> (64u - wd - (o & 31u))) & ((1u << wd) - 1u);
}

__device__ __forceinline__ uint64_t jls_lanes(uint32_t lo, uint32_t hi)  // lanes [lo, hi), lo <= 63, hi <= 64
{
	return (hi >= 64u ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
}

// One wave per interval.  LDS: the contexts as two words each, (A) and (N | B << 8 | C << 16) -- N <= 64, -64 < B <= 0 and
// -128 <= C <= 127 once a sample is done --, the claims, and the bit buffer of a step: a carry of fewer than 8 bits and 64
// lanes of at most 128 bits are 8199 bits, 257 words; jls_put touches two words behind the one a code starts in (JLS_STEP_WORDS).
// Every store to the staging slot is checked against istride; the slot is sized by jls_interval_bound().
template <typename Px>
__global__ void __launch_bounds__(64) jls_code_kernel(JlsEncArgs a)
{
	__shared__ uint32_t cA[365], cS[365], claim[365];
	__shared__ uint32_t w[JLS_STEP_WORDS];
	const uint32_t lane = threadIdx.x, frame = blockIdx.x / a.n_int, ki = blockIdx.x % a.n_int;
	const JlsParams &p = a.par;
	const uint32_t cols = a.cols, r0 = ki * a.rpi, nrows = min(a.rpi, a.rows - r0);
	const Px *img = (const Px *)a.images + (size_t)frame * a.rows * cols + (size_t)r0 * cols;
	uint8_t *dst = a.stage + (size_t)blockIdx.x * a.istride;
	for (uint32_t i = lane; i < 365u; i += 64u) { cA[i] = p.a0; cS[i] = 1u; claim[i] = 0xFFFFFFFFu; }
	for (uint32_t i = lane; i < JLS_STEP_WORDS; i += 64u) w[i] = 0;
	__syncthreads();
	// the run chain, the same in every lane: the interruption contexts 365 (RItype 0) and 366, and RUNindex
	uint32_t rA0 = p.a0, rA1 = p.a0, rN0 = 1, rN1 = 1, rNn0 = 0, rNn1 = 0, runindex = 0;
	uint32_t carry = 0, op = 0;  // bits waiting at the start of w; bytes written
	bool seven = false;          // the last byte written is 0xFF: the next one carries 7 bits
	bool over = false, bound_hit = false;
	for (uint32_t r = 0; r < nrows; r++) {
		const Px *cur = img + (size_t)r * cols, *abv = cur - cols;
		const int rc0 = r >= 2u ? (int)abv[-(ptrdiff_t)cols] : 0;  // Rc of column 0: the first sample two lines up
		bool in_run = false;
		uint32_t run_len = 0;
		for (uint32_t c0 = 0; c0 < cols; c0 += 64u) {
			const uint32_t c = c0 + lane, nv = min(64u, cols - c0);
			const bool valid = lane < nv;
			int x = 0, ra = 0, rb = 0, rc = 0, rd = 0;
			if (valid) {
				x = (int)cur[c];
				if (r) {
					rb = (int)abv[c];
					rd = (int)abv[min(c + 1u, cols - 1u)];
					rc = c ? (int)abv[c - 1u] : rc0;
				}
				ra = c ? (int)cur[c - 1u] : rb;
				over |= ((uint32_t)x >> a.precision) != 0;
			}
			int sign;
			const int q = jls_context(ra, rb, rc, rd, p, sign);
			const uint64_t zmask = __ballot(valid && q == 0), eqmask = __ballot(valid && x == ra);
			uint64_t pre = 0, code = 0, regmask = 0;
			uint32_t plen = 0, clen = 0;
			// b: the parse.  ppos: the first lane not yet assigned
			for (uint32_t ppos = 0; ppos < nv;) {
				if (!in_run) {
					const uint64_t zz = zmask >> ppos << ppos;
					const uint32_t s = zz ? (uint32_t)__ffsll((long long)zz) - 1u : nv;
					regmask |= jls_lanes(ppos, s);
					if (s >= nv) break;
					in_run = true;
					run_len = 0;
					ppos = s;
				}
				const uint64_t ne = ~eqmask >> ppos << ppos;  // lanes behind the line's end never equal: t <= nv unless nv is 64
				const uint32_t t = ne ? (uint32_t)__ffsll((long long)ne) - 1u : 64u;
				run_len += min(t, nv) - ppos;
				const bool eol = t >= nv && c0 + nv == cols;
				if (t >= nv && !eol) break;  // the run goes on in the next step
				in_run = false;
				uint64_t rp = 0;
				uint32_t rl = 0, cnt = run_len;  // run_len <= 65535: 32 ones at most
				while (cnt >= (1u << jls_j(runindex))) {
					rp = rp << 1 | 1u;
					rl++;
					cnt -= 1u << jls_j(runindex);
					if (runindex < 31u) runindex++;
				}
				if (eol) {
					if (cnt) { rp = rp << 1 | 1u; rl++; }
					if (lane == nv - 1u) { pre = rp; plen = rl; }
					break;
				}
				const int xt = __shfl(x, (int)t), rat = __shfl(ra, (int)t), rbt = __shfl(rb, (int)t);
				const uint32_t jr = jls_j(runindex);
				rp = (rp << 1) << jr | cnt;
				rl += 1u + jr;
				const bool rit = rat == rbt;
				int e = xt - (rit ? rat : rbt);
				if (!rit && rat > rbt) e = -e;
				e = jls_reduce(e, p);
				uint32_t A = rit ? rA1 : rA0, N = rit ? rN1 : rN0, Nn = rit ? rNn1 : rNn0;
				const uint32_t temp = rit ? A + (N >> 1) : A;
				uint32_t k = 0;
				while (k < 16u && (N << k) < temp) k++;
				const bool map = (k == 0 && e > 0 && 2u * Nn < N) || (e < 0 && 2u * Nn >= N) || (e < 0 && k != 0);
				const uint32_t em = 2u * (uint32_t)(e < 0 ? -e : e) - (rit ? 1u : 0u) - (map ? 1u : 0u);
				uint64_t cv;
				uint32_t cl;
				jls_golomb(em, k, p.limit - jr - 1u, p, cv, cl);
				if (lane == t) { pre = rp; plen = rl; code = cv; clen = cl; }
				if (e < 0) Nn++;
				A += (em + 1u - (rit ? 1u : 0u)) >> 1;
				if (N == p.reset) { A >>= 1; N >>= 1; Nn >>= 1; }
				N++;
				if (rit) { rA1 = A; rN1 = N; rNn1 = Nn; } else { rA0 = A; rN0 = N; rNn0 = Nn; }
				if (runindex) runindex--;
				ppos = t + 1u;
			}
			// c: the regular samples
			bool pending = (regmask >> lane & 1ull) != 0;
			const int pxm = jls_median(ra, rb, rc);
			while (__ballot(pending)) {
				if (pending) atomicMin(&claim[q], lane);
				__syncthreads();
				if (pending && claim[q] == lane) {
					uint32_t A = cA[q];
					const uint32_t s = cS[q];
					int N = (int)(s & 0xFFu), B = (int)(int8_t)(s >> 8), C = (int)(int8_t)(s >> 16);
					const int px = min(max(pxm + sign * C, 0), (int)p.maxval);
					const int e = jls_reduce((x - px) * sign, p);
					uint32_t k = 0;
					while (k < 16u && ((uint32_t)N << k) < A) k++;
					const uint32_t m = (k == 0 && 2 * B <= -N) ? (uint32_t)(e >= 0 ? 2 * e + 1 : -2 * (e + 1)) : (uint32_t)(e >= 0 ? 2 * e : -2 * e - 1);
					jls_golomb(m, k, p.limit, p, code, clen);
					jls_update(A, B, C, N, e, (int)p.reset);
					cA[q] = A;
					cS[q] = (uint32_t)N | ((uint32_t)B & 0xFFu) << 8 | ((uint32_t)C & 0xFFu) << 16;
					claim[q] = 0xFFFFFFFFu;
					pending = false;
				}
				__syncthreads();
			}
			// d: place the bits
			uint32_t total;
			uint32_t pos = carry + wave_excl_scan(plen + clen, total);
			if (plen) jls_put(w, pos, pre, plen);
			if (clen) jls_put(w, pos + plen, code, clen);
			__syncthreads();
			const uint32_t tot = carry + total;
			const bool last = r == nrows - 1u && c0 + 64u >= cols;
			// e: whole bytes out (at the interval's end the rest too, padded with the zeros behind it in w)
			uint32_t rpos = 0;
			for (;;) {
				const uint32_t wd = (seven && lane == 0) ? 7u : 8u;
				const uint32_t o = rpos + 8u * lane - ((seven && lane) ? 1u : 0u);
				const bool have = last ? o < tot : o + wd <= tot;
				const uint32_t b = have ? jls_bits(w, o, wd) : 0u;
				const uint64_t hm = __ballot(have), fm = __ballot(have && b == 0xFFu);
				if (!hm) break;
				const uint32_t nh = (uint32_t)__popcll(hm);  // the lanes that have a byte are the first nh
				const uint32_t first = fm ? (uint32_t)__ffsll((long long)fm) - 1u : 64u, take = min(nh, first + 1u);
				if (lane < take) {
					if ((size_t)op + lane < a.istride) dst[op + lane] = (uint8_t)b;
					else bound_hit = true;
				}
				op += take;
				rpos += 8u * take - (seven ? 1u : 0u);
				seven = first < nh;
			}
			if (!last) {
				const uint32_t left = tot - rpos;  // fewer than 8
				const uint32_t cv = left ? jls_bits(w, rpos, left) : 0u;
				__syncthreads();
				for (uint32_t i = lane; i < (tot >> 5) + 3u && i < JLS_STEP_WORDS; i += 64u) w[i] = 0;
				__syncthreads();
				if (lane == 0 && left) w[0] = cv << (32u - left);
				__syncthreads();
				carry = left;
			}
		}
	}
	if (seven) {
		if (lane == 0) {
			if ((size_t)op < a.istride) dst[op] = 0;
			else bound_hit = true;
		}
		op++;
	}
	if (lane == 0) a.ibytes[blockIdx.x] = op;
	if (over) atomicOr(&a.status[frame], JLS_ST_OVERFLOW);
	if (bound_hit) atomicOr(&a.status[frame], JLS_ST_BOUND);
}

__device__ __forceinline__ void jls_be16(uint8_t *&p, uint32_t v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; }

// one lane per frame: the headers (31 bytes at most, JLS_HDR_MAX), every interval's offset, EOI and the size.  A file that
// would pass out_stride is not written behind its headers and gets JLS_ST_BOUND.
__global__ void __launch_bounds__(64) jls_layout_kernel(JlsEncArgs a)
{
	const uint32_t frame = blockIdx.x * 64u + threadIdx.x;
	if (frame >= a.n) return;
	uint8_t *f = a.out + (size_t)frame * a.out_stride, *p = f;
	*p++ = 0xFF; *p++ = 0xD8;
	*p++ = 0xFF; *p++ = 0xF7; jls_be16(p, 11); *p++ = (uint8_t)a.precision; jls_be16(p, a.rows); jls_be16(p, a.cols);
	*p++ = 1; *p++ = 1; *p++ = 0x11; *p++ = 0;
	if (a.restart) { *p++ = 0xFF; *p++ = 0xDD; jls_be16(p, 4); jls_be16(p, a.restart); }
	*p++ = 0xFF; *p++ = 0xDA; jls_be16(p, 8); *p++ = 1; *p++ = 1; *p++ = 0; *p++ = 0; *p++ = 0; *p++ = 0;
	uint64_t off = (uint64_t)(p - f);
	for (uint32_t k = 0; k < a.n_int; k++) {
		if (k) off += 2;
		a.ioff[frame * a.n_int + k] = (uint32_t)min(off, (uint64_t)0xFFFFFFFFu);
		off += a.ibytes[frame * a.n_int + k];
	}
	if (off + 2u > a.out_stride) a.status[frame] |= JLS_ST_BOUND;  // only the code kernel, a launch earlier, writes this word too
	else { f[off] = 0xFF; f[off + 1] = 0xD9; }
	a.out_sizes[frame] = a.status[frame] ? 0u : (uint32_t)off + 2u;
}

// a workgroup per interval.  The layout kernel has checked that the frame's last interval ends inside out_stride.
__global__ void __launch_bounds__(256) jls_place_kernel(JlsEncArgs a)
{
	const uint32_t t = threadIdx.x, frame = blockIdx.x / a.n_int, k = blockIdx.x % a.n_int;
	if (a.status[frame]) return;
	const uint32_t nbytes = a.ibytes[blockIdx.x];
	const uint8_t *src = a.stage + (size_t)blockIdx.x * a.istride;
	uint8_t *dst = a.out + (size_t)frame * a.out_stride + a.ioff[blockIdx.x];
	if (k && t == 0) { dst[-2] = 0xFF; dst[-1] = (uint8_t)(0xD0u + ((k - 1u) & 7u)); }
	for (uint32_t i = t; i < nbytes; i += 256u) dst[i] = src[i];
}

// ---- decode ---------------------------------------------------------------------------------------------------------

// The interval's bytes p[0 .. end) as bits, most significant first; the byte behind a 0xFF gives its low 7.  acc holds nbits
// bits from its top down, `valid` of them from the data: behind the data the reader supplies zeros, and a read that takes
// one of those sets err.
struct JlsReader {
	const uint8_t *p;
	uint32_t pos, end;
	uint64_t acc;
	int nbits, valid;
	bool prev_ff, err;
	__device__ __forceinline__ void fill()
	{
		while (nbits <= 56) {
			uint32_t b = 0, wd = 8;
			if (pos < end) {
				const uint32_t raw = p[pos++];
				wd = prev_ff ? 7u : 8u;
				b = raw & ((1u << wd) - 1u);
				prev_ff = raw == 0xFFu;
				valid += (int)wd;
			}
			acc |= (uint64_t)b << (64 - nbits - (int)wd);
			nbits += (int)wd;
		}
	}
	__device__ __forceinline__ void consume(uint32_t n)  // n <= 47
	{
		acc <<= n;
		nbits -= (int)n;
		valid -= (int)n;
		if (valid < 0) err = true;
	}
	__device__ __forceinline__ uint32_t value(uint32_t n)  // n <= 31
	{
		fill();
		const uint32_t v = n ? (uint32_t)(acc >> (64u - n)) : 0u;
		consume(n);
		return v;
	}
	// zeros up to the next one, which is consumed; stops at `most` (<= 47) zeros, the bit behind them not consumed
	__device__ __forceinline__ uint32_t zeros(uint32_t most)
	{
		fill();
		const uint32_t z = acc ? (uint32_t)__clzll((long long)acc) : 64u;
		if (z >= most) { consume(most); return most; }
		consume(z + 1u);
		return z;
	}
	// the bytes of which a bit was read, one more if the last of them is 0xFF: anything but `end` is an error
	__device__ __forceinline__ void finish()
	{
		uint32_t t = pos;
		int v = valid;
		while (t > 0) {
			const int wd = (t >= 2u && p[t - 2u] == 0xFFu) ? 7 : 8;
			if (v < wd) break;
			v -= wd;
			t--;
		}
		if (t > 0 && p[t - 1u] == 0xFFu) t++;
		if (t != end) err = true;
	}
};

// M of a Golomb code with parameter k (< 32) under `limit`; a value above 2^qbpp is an error (no coder writes one)
__device__ __forceinline__ uint32_t jls_read_golomb(JlsReader &rd, uint32_t k, uint32_t limit, const JlsParams &p)
{
	const uint32_t esc = limit - p.qbpp - 1u;
	const uint32_t z = rd.zeros(esc);
	if (z < esc) {
		const uint64_t m = (uint64_t)z << k | rd.value(k);
		if (m > (1ull << p.qbpp)) { rd.err = true; return 0; }
		return (uint32_t)m;
	}
	if (!rd.value(1)) rd.err = true;
	return rd.value(p.qbpp) + 1u;
}

__device__ __forceinline__ int jls_fix(int rx, const JlsParams &p)
{
	if (rx < 0) rx += (int)p.range;
	else if (rx > (int)p.maxval) rx -= (int)p.range;
	return min(max(rx, 0), (int)p.maxval);
}

// A lane per interval; no lane waits for another.  LDS: lane l owns entry q * JLS_DEC_LANES + l of the tables; with an LSE
// segment N reaches 65535 and A 2^31, so a context takes three words here.  Every sample of the interval's lines is stored
// exactly once unless the data is in error, and nothing else is: c < cols guards every store, r < nrows every line.
template <typename Out>
__global__ void __launch_bounds__(JLS_DEC_LANES) jls_decode_kernel(JlsDecArgs a)
{
	constexpr uint32_t L = JLS_DEC_LANES;
	__shared__ uint32_t cA[367 * L], cNC[367 * L];  // cNC: N << 8 | (C & 0xFF)
	__shared__ int32_t cB[365 * L];
	const uint32_t l = threadIdx.x, ii = blockIdx.x * L + l;
	if (ii >= a.total_int) return;
	const JlsInterval iv = a.intervals[ii];
	const JlsParams p = a.frames[iv.frame].par;
	const uint32_t cols = a.cols;
	Out *out = (Out *)a.images + (size_t)a.frames[iv.frame].slot * a.rows * cols + (size_t)iv.row0 * cols;
	for (uint32_t q = 0; q < 367u; q++) { cA[q * L + l] = p.a0; cNC[q * L + l] = 1u << 8; }
	for (uint32_t q = 0; q < 365u; q++) cB[q * L + l] = 0;
	uint32_t nn0 = 0, nn1 = 0, runindex = 0;
	JlsReader rd{a.files + iv.src, 0, iv.len, 0, 0, 0, false, false};
	for (uint32_t r = 0; r < iv.nrows && !rd.err; r++) {
		Out *cur = out + (size_t)r * cols;
		const Out *abv = cur - cols;
		const int rc0 = r >= 2u ? (int)abv[-(ptrdiff_t)cols] : 0;
		int ra = r ? (int)abv[0] : 0;
		uint32_t c = 0;
		while (c < cols && !rd.err) {
			int rb = r ? (int)abv[c] : 0;
			const int rc = c ? (r ? (int)abv[c - 1u] : 0) : rc0, rdd = r ? (int)abv[min(c + 1u, cols - 1u)] : 0;
			int sign;
			const int q = jls_context(ra, rb, rc, rdd, p, sign);
			if (q) {
				uint32_t A = cA[q * L + l];
				const uint32_t nc = cNC[q * L + l];
				int N = (int)(nc >> 8), C = (int)(int8_t)nc, B = cB[q * L + l];
				const int px = min(max(jls_median(ra, rb, rc) + sign * C, 0), (int)p.maxval);
				uint32_t k = 0;
				while (k < 31u && ((uint64_t)N << k) < A) k++;
				const int m = (int)jls_read_golomb(rd, k, p.limit, p);
				int e;
				if (k == 0 && 2 * B <= -N) e = (m & 1) ? (m - 1) >> 1 : -(m >> 1) - 1;
				else e = (m & 1) ? -((m + 1) >> 1) : m >> 1;
				jls_update(A, B, C, N, e, (int)p.reset);
				cA[q * L + l] = A;
				cNC[q * L + l] = (uint32_t)N << 8 | ((uint32_t)C & 0xFFu);
				cB[q * L + l] = B;
				ra = jls_fix(px + sign * e, p);
				cur[c++] = (Out)ra;
				continue;
			}
			// run mode: every 1 bit moves c on by at least one sample, so the loop is bounded by the line
			bool ended = false;
			while (rd.value(1)) {
				const uint32_t seg = 1u << jls_j(runindex), n = min(seg, cols - c);
				for (uint32_t i = 0; i < n; i++) cur[c + i] = (Out)ra;
				c += n;
				if (n == seg && runindex < 31u) runindex++;
				if (c >= cols) { ended = true; break; }
			}
			if (ended || rd.err) break;
			const uint32_t jr = jls_j(runindex), n = rd.value(jr);
			if (c + n >= cols) { rd.err = true; break; }  // the run passes the end of the line
			for (uint32_t i = 0; i < n; i++) cur[c + i] = (Out)ra;
			c += n;
			rb = r ? (int)abv[c] : 0;
			const uint32_t rit = ra == rb ? 1u : 0u, qi = (365u + rit) * L + l;
			uint32_t A = cA[qi], N = cNC[qi] >> 8, Nn = rit ? nn1 : nn0;
			const uint32_t temp = rit ? A + (N >> 1) : A;
			uint32_t k = 0;
			while (k < 31u && ((uint64_t)N << k) < temp) k++;
			const uint32_t em = jls_read_golomb(rd, k, p.limit - jr - 1u, p), t = em + rit;
			int e = (int)((t + 1u) >> 1);
			if (e && (t & 1u) == ((k != 0 || 2u * Nn >= N) ? 1u : 0u)) e = -e;
			if (e < 0) Nn++;
			A += (em + 1u - rit) >> 1;
			if (N == p.reset) { A >>= 1; N >>= 1; Nn >>= 1; }
			N++;
			cA[qi] = A;
			cNC[qi] = N << 8;
			if (rit) nn1 = Nn; else nn0 = Nn;
			if (runindex) runindex--;
			if (!rit && ra > rb) e = -e;
			ra = jls_fix((rit ? ra : rb) + e, p);
			cur[c++] = (Out)ra;
		}
	}
	if (!rd.err) rd.finish();
	if (rd.err) atomicOr(&a.status[iv.frame], JLS_ST_STREAM);
}

}  // namespace

hipError_t launch_jls_encode(const JlsEncArgs &a, hipStream_t st)
{
	const dim3 per_frame((a.n + 63u) / 64u), per_int(a.n * a.n_int);
	if (a.src_bits == 16) hipLaunchKernelGGL(jls_code_kernel<uint16_t>, per_int, dim3(64), 0, st, a);
	else hipLaunchKernelGGL(jls_code_kernel<uint8_t>, per_int, dim3(64), 0, st, a);
	hipLaunchKernelGGL(jls_layout_kernel, per_frame, dim3(64), 0, st, a);
	hipLaunchKernelGGL(jls_place_kernel, per_int, dim3(256), 0, st, a);
	return hipGetLastError();
}

hipError_t launch_jls_decode(const JlsDecArgs &a, hipStream_t st)
{
	const dim3 grid((a.total_int + JLS_DEC_LANES - 1u) / JLS_DEC_LANES);
	if (a.out_bits == 16) hipLaunchKernelGGL(jls_decode_kernel<uint16_t>, grid, dim3(JLS_DEC_LANES), 0, st, a);
	else hipLaunchKernelGGL(jls_decode_kernel<uint8_t>, grid, dim3(JLS_DEC_LANES), 0, st, a);
	return hipGetLastError();
}

}  // namespace cct
