// Device functions shared by the PNG writer (png_kernels.hip) and the PNG reader (png_read_kernels.hip): the Paeth predictor
// and the workgroup CRC-32 (segment CRCs combined with multmodp).  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace cct {
namespace {

// PNG spec 9.4: ties go to a, then b, then c
__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c)
{
	const int p = (int)a + (int)b - (int)c;
	const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
	return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// zlib crc32.c multmodp: a * b modulo the CRC-32 polynomial, bit-reflected (bit 31 = x^0).  a must not be 0.
__device__ uint32_t multmodp(uint32_t a, uint32_t b)
{
	uint32_t m = 1u << 31, p = 0;
	for (;;) {
		if (a & m) {
			p ^= b;
			if ((a & (m - 1u)) == 0) break;
		}
		m >>= 1;
		b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
	}
	return p;
}

// x^(8 n) modulo the polynomial: the operator that appends n zero bytes to a raw CRC register
__device__ uint32_t x8n_mod(uint32_t n)
{
	uint32_t p = 1u << 31, sq = 1u << 23;  // x^0, x^8
	while (n) {
		if (n & 1u) p = multmodp(sq, p);
		sq = multmodp(sq, sq);
		n >>= 1;
	}
	return p;
}

// entry `tid` of the byte-wise CRC-32 table (256 lanes fill it; a barrier follows at the caller)
__device__ __forceinline__ void crc32_table_entry(uint32_t *table, int tid)
{
	uint32_t c = (uint32_t)tid;
#pragma unroll
	for (int i = 0; i < 8; i++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
	table[tid] = c;
}

// CRC-32 of the T bytes byte_at(0 .. T - 1) by one workgroup of 256 lanes; lane 0 returns it.  The bytes are cut into 256
// segments of equal length `seg`, aligned to the end (the first segment starts with up to 255 virtual zero bytes, which leave
// a raw CRC register at 0), so every lane's raw table CRC moves to its place by a power of two of the one-segment operator
// x^(8 seg): a tree of 8 levels, each level one squaring of the operator (crc32_combine for equal lengths).  table: filled
// and published by the caller; wave_crc: 4 words of LDS.  256 * seg must fit 32 bits: T <= 2^32 - 256.
template <class F>
__device__ __forceinline__ uint32_t crc32_workgroup(uint32_t T, const uint32_t *table, uint32_t *wave_crc, F byte_at)
{
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t seg = (T + 255) / 256, pad = 256 * seg - T;
	uint32_t reg = 0;
	const uint32_t v0 = (uint32_t)tid * seg, v1 = v0 + seg;
	for (uint32_t v = max(v0, pad); v < v1; v++) {
		const uint32_t j = v - pad;
		if (j == 0) reg = 0xFFFFFFFFu;  // CRC-32's initial register, in front of the first real byte
		const uint32_t b = byte_at(j);
		reg = table[(reg ^ b) & 255u] ^ (reg >> 8);
	}
	uint32_t P = x8n_mod(seg);  // one segment
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t right = (uint32_t)__shfl_down((int)reg, d, 64);
		if ((lane & (2 * d - 1)) == 0) reg = multmodp(P, reg) ^ right;
		P = multmodp(P, P);
	}
	if (lane == 0) wave_crc[wave] = reg;
	__syncthreads();
	uint32_t r = 0;
	if (tid == 0) {  // P = x^(8 * 64 seg): one wave's segments
		r = wave_crc[0];
		for (int w = 1; w < 4; w++) r = multmodp(P, r) ^ wave_crc[w];
		r ^= 0xFFFFFFFFu;
	}
	return r;
}

}  // namespace
}  // namespace cct
