// host emulation shim: one std::thread per GPU thread, blocks run one after another
#pragma once
#include <pthread.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>
typedef int hipError_t; typedef void *hipStream_t; typedef void *hipEvent_t;
constexpr hipError_t hipSuccess = 0;
constexpr hipError_t hipErrorInvalidValue = 1;
struct uint2 { uint32_t x, y; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
struct alignas(16) uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
extern thread_local dim3 threadIdx, blockIdx, blockDim;
struct BlockCtx { pthread_barrier_t bar; pthread_barrier_t wbar[16]; uint64_t wslot[16][64]; int orflag[2]; int phase; };
extern BlockCtx *g_blk;
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __constant__ static const
#define __launch_bounds__(...)
using std::min; using std::max;
static inline void __syncthreads() { pthread_barrier_wait(&g_blk->bar); }
static inline int __syncthreads_or(int v)
{
	static thread_local int ph = 0;
	int *f = &g_blk->orflag[ph & 1];
	if (v) __atomic_store_n(f, 1, __ATOMIC_SEQ_CST);
	pthread_barrier_wait(&g_blk->bar);
	int r = __atomic_load_n(f, __ATOMIC_SEQ_CST);
	pthread_barrier_wait(&g_blk->bar);
	if (threadIdx.x == 0) g_blk->orflag[ph & 1] = 0;
	pthread_barrier_wait(&g_blk->bar);
	return r;
}
static inline uint64_t wave_xchg(uint64_t v, int src)  // every lane of the wave must call
{
	const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
	g_blk->wslot[w][l] = v;
	pthread_barrier_wait(&g_blk->wbar[w]);
	uint64_t r = (src >= 0 && src < 64) ? g_blk->wslot[w][src] : v;
	pthread_barrier_wait(&g_blk->wbar[w]);
	return r;
}
static inline int __shfl(int v, int src, int = 64) { return (int)wave_xchg((uint32_t)v, src & 63); }
static inline int __shfl_up(int v, int d, int = 64) { int l = threadIdx.x & 63; return (int)wave_xchg((uint32_t)v, l - d >= 0 ? l - d : -1); }
static inline int __shfl_down(int v, int d, int = 64) { int l = threadIdx.x & 63; return (int)wave_xchg((uint32_t)v, l + d < 64 ? l + d : -1); }
static inline uint64_t __ballot(bool b)
{
	const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
	g_blk->wslot[w][l] = b;
	pthread_barrier_wait(&g_blk->wbar[w]);
	uint64_t r = 0;
	for (int k = 0; k < 64; k++) r |= (uint64_t)(g_blk->wslot[w][k] & 1) << k;
	pthread_barrier_wait(&g_blk->wbar[w]);
	return r;
}
static inline int __shfl_xor(int v, int m, int = 64) { return (int)wave_xchg((uint32_t)v, (int)(threadIdx.x & 63) ^ m); }
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t atomicOr(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t atomicMax(uint32_t *p, uint32_t v)
{
	uint32_t o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
	while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
	return o;
}
static inline int __clz(int x) { return x ? __builtin_clz((unsigned)x) : 32; }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline uint32_t __brev(uint32_t x)
{
	x = (x >> 16) | (x << 16);
	x = ((x & 0xFF00FF00u) >> 8) | ((x & 0x00FF00FFu) << 8);
	x = ((x & 0xF0F0F0F0u) >> 4) | ((x & 0x0F0F0F0Fu) << 4);
	x = ((x & 0xCCCCCCCCu) >> 2) | ((x & 0x33333333u) << 2);
	return ((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1);
}
static inline long long clock64() { return 0; }  // the emulation measures nothing
static inline int __clzll(long long x) { return x ? __builtin_clzll((unsigned long long)x) : 64; }
static inline int __ffsll(long long x) { return __builtin_ffsll(x); }
static inline hipError_t hipGetLastError() { return 0; }
// the host side of the runtime, for launch functions that name it; an emulator that plays the host side itself (allocations
// with poisoned tails, events: j2k_dec_host_emu) defines EMU_OWN_HOST_RUNTIME before it includes this file
#ifndef EMU_OWN_HOST_RUNTIME
enum { hipMemcpyHostToDevice, hipMemcpyDeviceToHost };
enum { hipFuncAttributeMaxDynamicSharedMemorySize };
static inline hipError_t hipFuncSetAttribute(const void *, int, int) { return hipSuccess; }
static inline hipError_t hipMalloc(void **p, size_t n) { *p = malloc(n ? n : 1); return *p ? hipSuccess : 1; }
template <class T> static inline hipError_t hipMalloc(T **p, size_t n) { return hipMalloc((void **)p, n); }
static inline hipError_t hipFree(void *p) { free(p); return hipSuccess; }
static inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
#endif
template <class K, class... A>
void emu_launch(K kernel, dim3 grid, dim3 block, A... args)
{
	// the threads of a launch play its blocks one after another, a barrier between two blocks (a block's __shared__ statics are
	// the next one's as well): threads are made once per launch, not once per block
	BlockCtx ctx{};
	pthread_barrier_init(&ctx.bar, nullptr, block.x);
	for (unsigned w = 0; w < (block.x + 63) / 64; w++) pthread_barrier_init(&ctx.wbar[w], nullptr, std::min(64u, block.x - 64 * w));
	g_blk = &ctx;
	std::vector<std::thread> th;
	for (unsigned t = 0; t < block.x; t++)
		th.emplace_back([=]() {
			threadIdx = dim3(t); blockDim = block;
			for (unsigned b = 0; b < grid.x; b++) {
				blockIdx = dim3(b);
				kernel(args...);
				pthread_barrier_wait(&g_blk->bar);
			}
		});
	for (auto &x : th) x.join();
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch(k, g, b, __VA_ARGS__)
