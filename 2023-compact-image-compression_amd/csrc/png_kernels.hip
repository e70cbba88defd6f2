// Device PNG writer for 16-bit grayscale slices, byte-identical to Pillow's PNG encoder (PngImagePlugin + ZipEncode.c) at
// compress_level 4 .. 9: the 16-bit preview the reference writes through imageio (src/codec/core.py:522-538) and the PNG
// column of its corpus comparison (lib/png.py:25-31).  Three stages (api.cpp cct_png_encode_batch):
//   filter   png_filter_kernel: one wave per row.  Samples are (v << shift) & 0xFFFF, big-endian, so bpp = 2, and row -1 is
//            zeros.  Pillow's choice: the cost of a filtered row is the sum of min(v, 256 - v) over its bytes (the filter
//            byte not counted); None first, then Up, Sub and Paeth, each tried only while the best cost is > 0 and taken
//            only when strictly cheaper (Average needs optimize=True, which is not offered).  Filter byte + filtered row
//            land in the DEFLATE pass's input.  png_filter8_kernel: the same for the 8-bit files of cct_png_encode8_batch
//            (bpp = 1), whose samples are uint8 rasters or uint16 rasters mapped through a window on load.
//   deflate  the device DEFLATE at memLevel 9 / Z_FILTERED (deflate_kernels.hip), or host libz
//   pack     png_pack_kernel: signature, IHDR, the zlib stream cut into IDAT chunks of max(65536, 4*cols) bytes (the
//            bufsize of Pillow's ImageFile._save; the last one shorter) and IEND, every chunk with its CRC-32
#include <hip/hip_runtime.h>

#include "cct_internal.h"
#include "wave_device.h"
#include "png_device.h"

namespace cct {
namespace {

// ZipEncode.c: the distance of a filtered byte from zero
__device__ __forceinline__ uint32_t png_cost(uint32_t v)
{
	v &= 255u;
	return v < 128u ? v : 256u - v;
}

// filter type f (0 None, 1 Sub, 2 Up, 4 Paeth) of byte x with left a, up b, up-left c
__device__ __forceinline__ uint32_t png_filter_byte(int f, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
	const uint32_t pred = f == 1 ? a : f == 2 ? b : f == 4 ? paeth(a, b, c) : 0u;
	return (x - pred) & 255u;
}

constexpr int FILTER_ROWS = 4;  // rows (waves) per workgroup

// Rows are independent: wave w of workgroup (x, s) filters row 4x + w of slice s.  A row is read twice (costs, then the chosen
// filter); the second pass finds it in the cache.  A pixel costs at most 256, so a lane's sums stay below 2^32 for any row
// the DEFLATE pass takes (cols < 2^29, cols / 64 pixels per lane); the wave adds them in 64 bits.
__global__ void __launch_bounds__(256) png_filter_kernel(const uint16_t *img, int rows, int cols, int shift, uint8_t *out,
                                                         size_t out_stride)
{
	const int s = blockIdx.y, r = (int)blockIdx.x * FILTER_ROWS + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (r >= rows) return;
	const uint16_t *cur = img + ((size_t)s * rows + r) * (size_t)cols;
	const bool has_up = r > 0;
	const uint16_t *up = has_up ? cur - cols : cur;
	uint8_t *o = out + (size_t)s * out_stride + (size_t)r * (1 + 2 * (size_t)cols);
	auto smp = [&](uint16_t v) { return ((uint32_t)v << shift) & 0xFFFFu; };
	auto load = [&](int c, uint32_t &x, uint32_t &a, uint32_t &b, uint32_t &d) {
		x = smp(cur[c]);
		a = c ? smp(cur[c - 1]) : 0u;
		b = has_up ? smp(up[c]) : 0u;
		d = has_up && c ? smp(up[c - 1]) : 0u;
	};
	uint32_t c_none = 0, c_sub = 0, c_up = 0, c_paeth = 0;
	for (int c = lane; c < cols; c += 64) {
		uint32_t x, a, b, d;
		load(c, x, a, b, d);
#pragma unroll
		for (int k = 0; k < 2; k++) {  // high byte, then low byte; byte i's left neighbour is byte i - 2: the same byte of pixel c - 1
			const uint32_t sh = 8u - 8u * (uint32_t)k;
			const uint32_t xb = (x >> sh) & 255u, ab = (a >> sh) & 255u, bb = (b >> sh) & 255u, db = (d >> sh) & 255u;
			c_none += png_cost(xb);
			c_sub += png_cost(xb - ab);
			c_up += png_cost(xb - bb);
			c_paeth += png_cost(xb - paeth(ab, bb, db));
		}
	}
	const uint64_t s_none = wave_sum((uint64_t)c_none), s_sub = wave_sum((uint64_t)c_sub), s_up = wave_sum((uint64_t)c_up), s_paeth = wave_sum((uint64_t)c_paeth);  // 64-bit sums
	uint64_t best = s_none;
	int f = 0;
	if (best > 0 && s_up < best) { best = s_up; f = 2; }
	if (best > 0 && s_sub < best) { best = s_sub; f = 1; }
	if (best > 0 && s_paeth < best) { best = s_paeth; f = 4; }
	if (lane == 0) o[0] = (uint8_t)f;
	for (int c = lane; c < cols; c += 64) {
		uint32_t x, a, b, d;
		load(c, x, a, b, d);
		o[1 + 2 * (size_t)c] = (uint8_t)png_filter_byte(f, x >> 8, a >> 8, b >> 8, d >> 8);
		o[2 + 2 * (size_t)c] = (uint8_t)png_filter_byte(f, x & 255u, a & 255u, b & 255u, d & 255u);
	}
}

// The 8-bit writer's filter (cct_png_encode8_batch): the samples are bytes, so bpp = 1 and the left neighbour is the previous
// pixel.  A uint16 raster is mapped to bytes through the window as it is loaded (no 8-bit raster exists in memory); a uint8
// raster takes the same path with the window (0, 255), which is the identity.  Pillow's costs, order and rule are those of
// png_filter_kernel above.
// The map y = ((clamp(v, lo, hi) - lo) * 510 + w) / (2 w), w = hi - lo, in integers: the numerator is below 2^25 (511 w,
// w < 2^16), and for 0 <= n < 2^25 and a divisor d with l = ceil(log2 d), floor(n / d) = (n * ceil(2^(25 + l) / d)) >> (25 + l)
// exactly (Granlund and Montgomery 1994, theorem 4.2); the multiplier is below 2^27, so the product fits 64 bits.
// launch_png_filter8 computes multiplier and shift on the host.
struct PngWindow {
	uint32_t lo, hi, w, mul, shift;
};

constexpr int FILTER8_PX = 8;  // pixels per lane per step: one 16-byte load of uint16 samples, one 8-byte store of filtered bytes

// One wave per row as above; lane l takes pixels [8 (l + 64 i), 8 (l + 64 i) + 8) in step i.  The group of a lane starts at any
// address (a row starts at r * cols samples and its output at r * (1 + cols) + 1 bytes): whole groups are moved with
// __builtin_memcpy, which gfx950 turns into one load or store at any alignment (deflate_kernels.hip compares matches the same
// way); the last, partial group of a row goes pixel by pixel.  Nothing outside [0, cols) of the two rows is read.  A pixel
// costs at most 128, so a lane's sums stay below 2^32 for any row the DEFLATE pass takes; the wave adds them in 64 bits.
template <class T>
__global__ void __launch_bounds__(256) png_filter8_kernel(const T *img, int rows, int cols, PngWindow win, uint8_t *out,
                                                          size_t out_stride)
{
	const int s = blockIdx.y, r = (int)blockIdx.x * FILTER_ROWS + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (r >= rows) return;
	const T *cur = img + ((size_t)s * rows + r) * (size_t)cols;
	const bool has_up = r > 0;
	const T *up = has_up ? cur - cols : cur;
	uint8_t *o = out + (size_t)s * out_stride + (size_t)r * (1 + (size_t)cols);
	auto smp = [&](uint32_t v) {
		const uint32_t c = min(max(v, win.lo), win.hi);
		return (uint32_t)(((uint64_t)((c - win.lo) * 510u + win.w) * win.mul) >> win.shift);
	};
	// y[0] = sample c0 - 1 of `row` (0 in front of the row), y[1 + i] = sample c0 + i for i < nv
	auto load = [&](const T *row, int c0, int nv, uint32_t (&y)[1 + FILTER8_PX]) {
		constexpr int PER_WORD = 4 / (int)sizeof(T);  // samples in a 32-bit word, the lowest address in the low bits
		uint32_t raw[FILTER8_PX];
		if (nv == FILTER8_PX) {
			uint32_t words[FILTER8_PX / PER_WORD];
			__builtin_memcpy(words, row + c0, sizeof(words));
#pragma unroll
			for (int i = 0; i < FILTER8_PX; i++) raw[i] = (words[i / PER_WORD] >> (8 * (int)sizeof(T) * (i % PER_WORD))) & (T)~(T)0;
		} else {
#pragma unroll
			for (int i = 0; i < FILTER8_PX; i++) raw[i] = i < nv ? (uint32_t)row[c0 + i] : 0u;
		}
		y[0] = c0 ? smp(row[c0 - 1]) : 0u;
#pragma unroll
		for (int i = 0; i < FILTER8_PX; i++) y[1 + i] = smp(raw[i]);
	};
	auto load_both = [&](int c0, int nv, uint32_t (&x)[1 + FILTER8_PX], uint32_t (&b)[1 + FILTER8_PX]) {
		load(cur, c0, nv, x);
		if (has_up) {
			load(up, c0, nv, b);
		} else {
#pragma unroll
			for (int i = 0; i <= FILTER8_PX; i++) b[i] = 0u;
		}
	};
	uint32_t c_none = 0, c_sub = 0, c_up = 0, c_paeth = 0;
	for (int c0 = lane * FILTER8_PX; c0 < cols; c0 += 64 * FILTER8_PX) {
		const int nv = min(FILTER8_PX, cols - c0);
		uint32_t x[1 + FILTER8_PX], b[1 + FILTER8_PX];
		load_both(c0, nv, x, b);
#pragma unroll
		for (int i = 0; i < FILTER8_PX; i++) {
			if (i < nv) {
				c_none += png_cost(x[1 + i]);
				c_sub += png_cost(x[1 + i] - x[i]);
				c_up += png_cost(x[1 + i] - b[1 + i]);
				c_paeth += png_cost(x[1 + i] - paeth(x[i], b[1 + i], b[i]));
			}
		}
	}
	const uint64_t s_none = wave_sum((uint64_t)c_none), s_sub = wave_sum((uint64_t)c_sub), s_up = wave_sum((uint64_t)c_up), s_paeth = wave_sum((uint64_t)c_paeth);  // 64-bit sums
	uint64_t best = s_none;
	int f = 0;
	if (best > 0 && s_up < best) { best = s_up; f = 2; }
	if (best > 0 && s_sub < best) { best = s_sub; f = 1; }
	if (best > 0 && s_paeth < best) { best = s_paeth; f = 4; }
	if (lane == 0) o[0] = (uint8_t)f;
	for (int c0 = lane * FILTER8_PX; c0 < cols; c0 += 64 * FILTER8_PX) {
		const int nv = min(FILTER8_PX, cols - c0);
		uint32_t x[1 + FILTER8_PX], b[1 + FILTER8_PX];
		load_both(c0, nv, x, b);
		uint32_t q[FILTER8_PX];
#pragma unroll
		for (int i = 0; i < FILTER8_PX; i++) q[i] = png_filter_byte(f, x[1 + i], x[i], b[1 + i], b[i]);
		uint8_t *dst = o + 1 + (size_t)c0;
		if (nv == FILTER8_PX) {
			const uint32_t words[2] = {q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24), q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24)};
			__builtin_memcpy(dst, words, sizeof(words));
		} else {
#pragma unroll
			for (int i = 0; i < FILTER8_PX; i++)
				if (i < nv) dst[i] = (uint8_t)q[i];
		}
	}
}

__constant__ uint8_t c_png_sig[8] = {0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A};
__constant__ uint8_t c_png_iend[12] = {0, 0, 0, 0, 0x49, 0x45, 0x4E, 0x44, 0xAE, 0x42, 0x60, 0x82};
__constant__ uint8_t c_idat[4] = {0x49, 0x44, 0x41, 0x54};

// One workgroup per (chunk k, slice s): copies the chunk's bytes of the zlib stream behind its length and type and appends
// the CRC-32 of type + data.  The CRC: the 4 + len bytes are cut into 256 segments of equal length `seg`, aligned to the end
// (the first segment starts with up to 255 virtual zero bytes, which leave a raw CRC register at 0), so every lane's raw
// table CRC moves to its place by a power of two of the one-segment operator x^(8 seg): a tree of 8 levels, each level one
// squaring of the operator (crc32_combine for equal lengths); crc32_workgroup (png_device.h) is the same scheme as a function,
// which the reader uses (calling it here moved this kernel's instructions about).  Chunk 0 also writes the signature and IHDR; the last chunk
// IEND and the file size.
__global__ void __launch_bounds__(256) png_pack_kernel(PngPackArgs a)
{
	__shared__ uint32_t table[256];
	__shared__ uint32_t wave_crc[4];
	const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t k = blockIdx.x;
	const uint32_t Z = a.src_sizes[s] - a.src_skip, C = a.chunk;
	const uint32_t nch = (Z + C - 1) / C;
	if (k >= nch) return;
	const uint8_t *src = a.src + (size_t)s * a.src_stride + a.src_skip + (size_t)k * C;
	uint8_t *out = a.out + (size_t)s * a.out_stride;
	const uint32_t len = min(C, Z - k * C);
	const size_t o = 33 + (size_t)k * ((size_t)C + 12);
	{
		uint32_t c = (uint32_t)tid;
#pragma unroll
		for (int i = 0; i < 8; i++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
		table[tid] = c;
	}
	if (k == 0 && tid < 33) out[tid] = tid < 8 ? c_png_sig[tid] : a.ihdr[tid - 8];
	if (tid < 8) out[o + tid] = tid < 4 ? (uint8_t)(len >> (24 - 8 * tid)) : c_idat[tid - 4];
	for (uint32_t j = (uint32_t)tid; j < len; j += 256) out[o + 8 + j] = src[j];
	if (k == nch - 1) {
		const size_t e = 33 + (size_t)Z + 12 * (size_t)nch;
		if (tid < 12) out[e + tid] = c_png_iend[tid];
		if (tid == 0) a.out_sizes[s] = (uint32_t)(e + 12);
	}
	__syncthreads();
	const uint32_t T = 4 + len, seg = (T + 255) / 256, pad = 256 * seg - T;
	uint32_t reg = 0;
	const uint32_t v0 = (uint32_t)tid * seg, v1 = v0 + seg;
	for (uint32_t v = max(v0, pad); v < v1; v++) {
		const uint32_t j = v - pad;
		if (j == 0) reg = 0xFFFFFFFFu;  // CRC-32's initial register, in front of the first real byte
		const uint32_t b = j < 4 ? c_idat[j] : src[j - 4];
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
	if (tid == 0) {  // P = x^(8 * 64 seg): one wave's segments
		uint32_t r = wave_crc[0];
		for (int w = 1; w < 4; w++) r = multmodp(P, r) ^ wave_crc[w];
		const uint32_t crc = r ^ 0xFFFFFFFFu;
		uint8_t *q = out + o + 8 + len;
		q[0] = (uint8_t)(crc >> 24); q[1] = (uint8_t)(crc >> 16); q[2] = (uint8_t)(crc >> 8); q[3] = (uint8_t)crc;
	}
}

}  // namespace

hipError_t launch_png_filter(const uint16_t *d_img, int n, int rows, int cols, int shift, uint8_t *d_out, size_t out_stride,
                             hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	hipLaunchKernelGGL(png_filter_kernel, dim3((rows + FILTER_ROWS - 1) / FILTER_ROWS, n), dim3(64 * FILTER_ROWS), 0, st, d_img,
	                   rows, cols, shift, d_out, out_stride);
	return hipGetLastError();
}

hipError_t launch_png_filter8(const void *d_img, int src_bits, int n, int rows, int cols, int lo, int hi, uint8_t *d_out,
                              size_t out_stride, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	PngWindow win{};
	win.lo = (uint32_t)lo; win.hi = (uint32_t)hi; win.w = win.hi - win.lo;
	const uint32_t d = 2u * win.w;
	uint32_t l = 1;
	while ((1u << l) < d) l++;
	win.shift = 25u + l;
	win.mul = (uint32_t)((((uint64_t)1 << win.shift) + d - 1) / d);
	const dim3 grid((rows + FILTER_ROWS - 1) / FILTER_ROWS, n), block(64 * FILTER_ROWS);
	if (src_bits == 16)
		hipLaunchKernelGGL(png_filter8_kernel<uint16_t>, grid, block, 0, st, (const uint16_t *)d_img, rows, cols, win, d_out, out_stride);
	else
		hipLaunchKernelGGL(png_filter8_kernel<uint8_t>, grid, block, 0, st, (const uint8_t *)d_img, rows, cols, win, d_out, out_stride);
	return hipGetLastError();
}

hipError_t launch_png_pack(const PngPackArgs &a, int n, uint32_t max_chunks, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	hipLaunchKernelGGL(png_pack_kernel, dim3(max_chunks, n), dim3(256), 0, st, a);
	return hipGetLastError();
}

}  // namespace cct
