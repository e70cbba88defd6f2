// Lane-level plumbing shared by every kernel file: the DPP move and its control words, additive scans over a wave and over a
// workgroup, xor-butterfly reduces, the one-lane shift and the LDS-only barrier.  Each translation unit gets its own copy
// (anonymous namespace).
//
// EVERY LANE OF THE WAVE MUST REACH A CALL.  A DPP move reads the source lane's register whether or not that lane is enabled
// for the instruction, and leaves a disabled destination lane alone: under a lane-divergent branch a scan sums stale
// registers (the row_bcast steps read lanes 15, 31 and 47 of every wave) and the total comes from a lane 63 that never took
// part.  A wave-uniform branch (`if (wave == 0)`, a loop whose bounds are the same for the whole wave) is fine.
//
// DPP, not LDS permute (ds_bpermute, which is what __shfl* compiles to): a DPP move is a modifier on a VALU instruction, so a
// scan step is one v_add with VALU latency; a permute is an LDS instruction per step that shares the queue (and lgkmcnt) with
// the kernel's real LDS traffic.  The host emulators under tools/debug compile the .hip files with a C++ compiler and a
// stand-in hip_runtime.h that has __shfl* but no DPP builtin: off the device the scans fall back to the __shfl_up loop.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

// the HIP compiler (both of its passes parse the kernels) against a C++ compiler with the emulators' stand-in runtime
#if defined(__HIP__)
#define CCT_WAVE_DPP 1
#else
#define CCT_WAVE_DPP 0
#endif

namespace cct {
namespace {

// workgroup barrier that orders LDS traffic only: __syncthreads() also drains vmcnt, which would serialise the global loads
// and stores in flight with the barrier
__device__ __forceinline__ void lds_barrier()
{
#if CCT_WAVE_DPP
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#else
	__syncthreads();
#endif
}

// ---- xor-butterfly reduces: every lane gets the result ----------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
	return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
		v += ((uint64_t)hi << 32) | lo;
	}
	return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
	return v;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d);
	return v;
}

#if CCT_WAVE_DPP
// ---- DPP move ------------------------------------------------------------------------------------------------------------
// A lane whose source lies outside the wave (or outside its row, for the row_* controls), or whose row ROW_MASK leaves out,
// reads `old`.
constexpr int DPP_QUAD_SWAP1 = 0xB1;                                                          // quad_perm [1,0,3,2]: lane i <- lane i^1
constexpr int DPP_QUAD_EVEN = 0xA0;                                                           // quad_perm [0,0,2,2]: lane i <- lane i&~1
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;  // lane i <- lane i-n of its row of 16
constexpr int DPP_WAVE_SHR1 = 0x138;                                                          // lane i <- lane i-1 across the whole wave
constexpr int DPP_ROW_BCAST15 = 0x142;                                                        // lane 15 of a row -> every lane of the next row
constexpr int DPP_ROW_BCAST31 = 0x143;                                                        // lane 31 -> every lane of rows 2 and 3
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ uint32_t dpp_move(uint32_t v, uint32_t old = 0)
{
	return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xF, false);
}
#endif

// v of the lane below; lane 0 takes `fill`
__device__ __forceinline__ uint32_t wave_shift_up(uint32_t v, uint32_t fill)
{
#if CCT_WAVE_DPP
	return dpp_move<DPP_WAVE_SHR1>(v, fill);
#else
	const uint32_t o = (uint32_t)__shfl_up((int)v, 1);
	return (threadIdx.x & 63) ? o : fill;
#endif
}

// ---- additive scans --------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
#if CCT_WAVE_DPP
	v += dpp_move<DPP_ROW_SHR1>(v);
	v += dpp_move<DPP_ROW_SHR2>(v);
	v += dpp_move<DPP_ROW_SHR4>(v);
	v += dpp_move<DPP_ROW_SHR8>(v);
	v += dpp_move<DPP_ROW_BCAST15, 0xA>(v);  // into rows 1 and 3
	v += dpp_move<DPP_ROW_BCAST31, 0xC>(v);  // into rows 2 and 3
#else
	const int lane = threadIdx.x & 63;
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = (uint32_t)__shfl_up((int)v, d);
		if (lane >= d) v += o;
	}
#endif
	return v;
}

// exclusive scan over the wave; the wave's sum (lane 63) in `total`
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t &total)
{
	const uint32_t inc = wave_incl_scan(v);
#if CCT_WAVE_DPP
	total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
#else
	total = (uint32_t)__shfl((int)inc, 63);
#endif
	return inc - v;
}

// 64-bit inclusive scan (file offsets past 2^32): both halves move, the add is done in 64 bits.  The permute loop on the device
// too: a test of seconds cannot reach past 2^32, so its one user (dfl_pack_offsets_kernel) keeps the instructions it always had
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v)
{
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
#if CCT_WAVE_DPP
		const uint64_t o = __shfl_up((unsigned long long)v, d);
#else
		const uint64_t o = (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d) << 32 | (uint32_t)__shfl_up((int)(uint32_t)v, d);
#endif
		if (lane >= d) v += o;
	}
	return v;
}

// Exclusive scan of v over the workgroup (threads in tid order); total returned in `total`.  blockDim.x is a multiple of 64,
// `scratch` needs blockDim.x / 64 words of LDS, and the call contains two barriers: the one place that turns wave sums into
// a workgroup prefix.
// NW: the number of waves where the kernel fixes it (the loop over the wave sums is then unrolled), 0: read from blockDim.
template <int NW = 0, typename T>
__device__ __forceinline__ T wg_excl_scan(T v, T *scratch, T &total)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = NW ? NW : (int)(blockDim.x >> 6);
	const T inc = wave_incl_scan(v);
	if (lane == 63) scratch[wave] = inc;
	__syncthreads();
	T base = 0, tot = 0;
	for (int w = 0; w < nw; w++) {
		const T x = scratch[w];
		if (w < wave) base += x;
		tot += x;
	}
	__syncthreads();
	total = tot;
	return base + inc - v;
}

}  // namespace
}  // namespace cct
