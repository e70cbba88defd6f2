// What the three CompaCT stage-(i) encoders (encode_kernels.hip, encode_tiles.hip, encode_stream.hip) must agree on byte for
// byte: the three predicates that define the token format, the packed 16-bit subtract they are evaluated on, and the list of
// difficult blocks.  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "cct_internal.h"

namespace cct {
namespace {

// LDS pointers carry their address space in the type: a generic pointer would turn every access
// into a flat_* instruction, whose completion forces vmcnt(0) and drains the prefetch ring.
#define LDS(T) __attribute__((address_space(3))) T

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// ---- the token format ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool tok_two(int dlt) { return (uint32_t)(dlt + 63) > 127u; }      // two-byte token: outside [-63, 64], core.py:316
__device__ __forceinline__ bool seg_large(int dlt) { return (uint32_t)(dlt + 64) > 128u; }    // |delta| > 64, cluster.py:37-38
__device__ __forceinline__ bool out_of_q7(int dlt) { return (uint32_t)(dlt + 2047) > 4095u; } // outside [-2047, 2048], SURVEY App. A Q7

// per-half a - b of two packed 16-bit pairs (v_pk_sub)
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b)
{
	return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b)));
}

// difficult-block list: first ENC_LIST_CAP records in LDS, the rest in the HBM workspace
struct DiffList {
	LDS(uint32_t) *l_idx; LDS(uint8_t) *l_cur; LDS(uint64_t) *l_mask;
	uint32_t *g_idx; uint8_t *g_cur; uint64_t *g_mask;
	__device__ __forceinline__ void set(uint32_t e, uint32_t idx, uint32_t cur) const
	{
		if (e < ENC_LIST_CAP) { l_idx[e] = idx; l_cur[e] = (uint8_t)cur; }
		else { g_idx[e - ENC_LIST_CAP] = idx; g_cur[e - ENC_LIST_CAP] = (uint8_t)cur; }
	}
	__device__ __forceinline__ uint32_t idx(uint32_t e) const
	{
		uint32_t v;
		if (e < ENC_LIST_CAP) v = l_idx[e]; else v = g_idx[e - ENC_LIST_CAP];
		return v;
	}
	__device__ __forceinline__ uint32_t cur(uint32_t e) const
	{
		uint32_t v;
		if (e < ENC_LIST_CAP) v = l_cur[e]; else v = g_cur[e - ENC_LIST_CAP];
		return v;
	}
	__device__ __forceinline__ uint64_t mask(uint32_t e) const
	{
		uint64_t v;
		if (e < ENC_LIST_CAP) v = l_mask[e]; else v = g_mask[e - ENC_LIST_CAP];
		return v;
	}
	__device__ __forceinline__ void set_mask(uint32_t e, uint64_t m) const
	{
		if (e < ENC_LIST_CAP) l_mask[e] = m; else g_mask[e - ENC_LIST_CAP] = m;
	}
};

}  // namespace
}  // namespace cct
