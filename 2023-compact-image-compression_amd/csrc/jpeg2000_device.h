// Device functions and constants shared by the JPEG 2000 encoder (jpeg2000_kernels.hip) and decoder (jpeg2000_decode_kernels.hip):
// the MQ state table, the Tier-1 sample word and its contexts (Annex D), the set-up of a code-block's tables in LDS, the two
// halves of "this sample became significant" around the coders' own sign decision, and the shape of a tag tree, as
// tests/jpeg2000_model.py holds them for both Python models.  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <hip/hip_runtime.h>

namespace cct {
namespace {

// T.800 Table C.2: Qe | NMPS << 16 | NLPS << 22 | SWITCH << 28
#define J2K_Q(qe, nm, nl, sw) ((uint32_t)(qe) | (uint32_t)(nm) << 16 | (uint32_t)(nl) << 22 | (uint32_t)(sw) << 28)
__device__ const uint32_t J2K_MQ_TABLE[47] = {
	J2K_Q(0x5601, 1, 1, 1), J2K_Q(0x3401, 2, 6, 0), J2K_Q(0x1801, 3, 9, 0), J2K_Q(0x0AC1, 4, 12, 0), J2K_Q(0x0521, 5, 29, 0), J2K_Q(0x0221, 38, 33, 0),
	J2K_Q(0x5601, 7, 6, 1), J2K_Q(0x5401, 8, 14, 0), J2K_Q(0x4801, 9, 14, 0), J2K_Q(0x3801, 10, 14, 0), J2K_Q(0x3001, 11, 17, 0), J2K_Q(0x2401, 12, 18, 0),
	J2K_Q(0x1C01, 13, 20, 0), J2K_Q(0x1601, 29, 21, 0), J2K_Q(0x5601, 15, 14, 1), J2K_Q(0x5401, 16, 14, 0), J2K_Q(0x5101, 17, 15, 0), J2K_Q(0x4801, 18, 16, 0),
	J2K_Q(0x3801, 19, 17, 0), J2K_Q(0x3401, 20, 18, 0), J2K_Q(0x3001, 21, 19, 0), J2K_Q(0x2801, 22, 19, 0), J2K_Q(0x2401, 23, 20, 0), J2K_Q(0x2201, 24, 21, 0),
	J2K_Q(0x1C01, 25, 22, 0), J2K_Q(0x1801, 26, 23, 0), J2K_Q(0x1601, 27, 24, 0), J2K_Q(0x1401, 28, 25, 0), J2K_Q(0x1201, 29, 26, 0), J2K_Q(0x1101, 30, 27, 0),
	J2K_Q(0x0AC1, 31, 28, 0), J2K_Q(0x09C1, 32, 29, 0), J2K_Q(0x08A1, 33, 30, 0), J2K_Q(0x0521, 34, 31, 0), J2K_Q(0x0441, 35, 32, 0), J2K_Q(0x02A1, 36, 33, 0),
	J2K_Q(0x0221, 37, 34, 0), J2K_Q(0x0141, 38, 35, 0), J2K_Q(0x0111, 39, 36, 0), J2K_Q(0x0085, 40, 37, 0), J2K_Q(0x0049, 41, 38, 0), J2K_Q(0x0025, 42, 39, 0),
	J2K_Q(0x0015, 43, 40, 0), J2K_Q(0x0009, 44, 41, 0), J2K_Q(0x0005, 45, 42, 0), J2K_Q(0x0001, 45, 43, 0), J2K_Q(0x5601, 46, 46, 0),
};
#undef J2K_Q

// the word of a sample: which of its eight neighbours are significant, its own state, its magnitude (19 bits at most)
constexpr uint32_t T1_N = 1u, T1_S = 2u, T1_W = 4u, T1_E = 8u, T1_NW = 16u, T1_NE = 32u, T1_SW = 64u, T1_SE = 128u, T1_NBR = 255u;
constexpr uint32_t T1_SIG = 1u << 8, T1_NEG = 1u << 9, T1_VISIT = 1u << 10, T1_REFINED = 1u << 11, T1_MAG_SHIFT = 12;
constexpr uint32_t CTX_SIGN = 9, CTX_MAG = 14, CTX_RL = 17, CTX_UNI = 18, N_CTX = 19;

// Table D.1 from the neighbour bits of a state word
__device__ __forceinline__ uint32_t zc_context(uint32_t orient, uint32_t f)
{
	uint32_t hn = ((f >> 2) & 1) + ((f >> 3) & 1), vn = (f & 1) + ((f >> 1) & 1);
	const uint32_t dn = ((f >> 4) & 1) + ((f >> 5) & 1) + ((f >> 6) & 1) + ((f >> 7) & 1);
	if (orient == 1) { const uint32_t t = hn; hn = vn; vn = t; }
	if (orient == 3) {
		const uint32_t hv = hn + vn;
		if (dn >= 3) return 8;
		if (dn == 2) return hv >= 1 ? 7 : 6;
		if (dn == 1) return hv >= 2 ? 5 : 3 + hv;
		return hv >= 2 ? 2 : hv;
	}
	if (hn == 2) return 8;
	if (hn == 1) return vn >= 1 ? 7 : (dn >= 1 ? 6 : 5);
	if (vn == 2) return 4;
	if (vn == 1) return 3;
	return dn >= 2 ? 2 : dn;
}

// Table D.3 from (signs N S W E) << 4 | (significant N S W E): context | flip << 7
__device__ __forceinline__ uint32_t sc_context(uint32_t k)
{
	auto contrib = [&](uint32_t bit) { return !((k >> bit) & 1) ? 0 : ((k >> (4 + bit)) & 1) ? -1 : 1; };
	int vc = std::max(-1, std::min(1, contrib(0) + contrib(1))), hc = std::max(-1, std::min(1, contrib(2) + contrib(3)));
	uint32_t flip = 0;
	if (hc < 0 || (hc == 0 && vc < 0)) { hc = -hc; vc = -vc; flip = 1; }
	return (CTX_SIGN + (uint32_t)(hc ? 3 + vc : vc)) | flip << 7;
}

// what a pass codes: an insignificant sample with a significant neighbour; a significant sample not visited in this plane
__device__ __forceinline__ uint32_t spp_candidate(uint32_t f) { return (uint32_t)(!(f & T1_SIG) && (f & T1_NBR)); }
__device__ __forceinline__ uint32_t mrp_candidate(uint32_t f) { return (uint32_t)((f & (T1_SIG | T1_VISIT)) == T1_SIG); }

// The tables of a code-block in LDS, filled by the lanes of its wave (a barrier follows at the caller): D.1 for the subband's
// orientation and D.3 as bytes, the 47 MQ states, and the contexts in their initial states (D.7, MPS 0).
__device__ __forceinline__ void t1_load_tables(uint32_t lane, uint32_t orient, uint32_t *s_table, uint32_t *s_ctx, uint8_t *s_zc, uint8_t *s_sc)
{
	for (uint32_t i = lane; i < 256; i += 64) { s_zc[i] = (uint8_t)zc_context(orient, i); s_sc[i] = (uint8_t)sc_context(i); }
	if (lane < 47) s_table[lane] = J2K_MQ_TABLE[lane];
	if (lane < N_CTX) s_ctx[lane] = J2K_MQ_TABLE[lane == 0 ? 4 : lane == CTX_RL ? 3 : lane == CTX_UNI ? 46 : 0];
}

// A sample becomes significant: its sign is coded in the context s_sc[] holds for this key of the four neighbour words ..
__device__ __forceinline__ uint32_t t1_sign_key(uint32_t n, uint32_t s, uint32_t wl, uint32_t e)
{
	return ((n >> 8) & 1) | ((s >> 8) & 1) << 1 | ((wl >> 8) & 1) << 2 | ((e >> 8) & 1) << 3 | ((n >> 9) & 1) << 4 | ((s >> 9) & 1) << 5 |
	       ((wl >> 9) & 1) << 6 | ((e >> 9) & 1) << 7;
}
// .. and then sample i of the block (rows of FW words) tells its eight neighbours; n, s, wl, e are the four words read for the key
__device__ __forceinline__ void t1_tell_neighbours(uint32_t *s_w, uint32_t i, uint32_t FW, uint32_t n, uint32_t s, uint32_t wl, uint32_t e)
{
	s_w[i - FW] = n | T1_S; s_w[i + FW] = s | T1_N; s_w[i - 1] = wl | T1_E; s_w[i + 1] = e | T1_W;
	s_w[i - FW - 1] |= T1_SE; s_w[i - FW + 1] |= T1_SW;
	s_w[i + FW - 1] |= T1_NE; s_w[i + FW + 1] |= T1_NW;
}

// B.10.2: level 0 holds the ncw x nch leaves, every further level half of it rounded up, down to 1 x 1 or to LEVELS levels
template <uint32_t LEVELS>
struct TagTreeShape {
	uint32_t nlev, off[LEVELS], lw[LEVELS];
	__device__ void shape(uint32_t ncw, uint32_t nch)
	{
		uint32_t pw = ncw, ph = nch, o = 0;
		nlev = 0;
		for (;;) {
			off[nlev] = o; lw[nlev] = pw;
			nlev++;
			if ((pw == 1 && ph == 1) || nlev == LEVELS) break;
			o += pw * ph; pw = (pw + 1) / 2; ph = (ph + 1) / 2;
		}
	}
	__device__ __forceinline__ uint32_t node(int lv, uint32_t x, uint32_t y) const { return off[lv] + (y >> lv) * lw[lv] + (x >> lv); }  // above leaf (x, y)
};

__device__ __forceinline__ uint32_t bit_length(uint32_t v) { return v ? 32u - (uint32_t)__clz((int)v) : 0u; }

}  // namespace
}  // namespace cct
