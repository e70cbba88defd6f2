// Device PNG reader for 8- and 16-bit grayscale files (api.cpp cct_png_read_batch), the inverse of png_kernels.hip and of the
// reference's png_to_array (lib/png.py).  The host walks the chunk heads and builds the chunk table; then
//   unpack    png_unpack_kernel: one workgroup per chunk checks the chunk's CRC-32 and, for IDAT, copies the data to its place
//             in the file's zlib stream
//   inflate   inflate_kernels.hip, unchanged, on the gathered streams
//   unfilter  png_unfilter_kernel: filter byte + filtered row -> uint16 samples >> shift
// Every address below is computed from values of the host's table (PngChunk) or from the shape the caller passed; file
// content is only ever compared (CRC), copied (IDAT) or used as a selector among the five filter types.
#include <hip/hip_runtime.h>

#include "cct_internal.h"
#include "png_device.h"

#ifndef CCT_PNG_DYNAMIC_LDS  // the host emulation (tools/debug/inflate_host_emu) supplies the launch's bytes its own way
#define CCT_PNG_DYNAMIC_LDS(name) extern __shared__ __attribute__((aligned(16))) uint8_t name[]
#endif

namespace cct {
namespace {

// The copy runs first and coalesced: whole dwords of the destination, each put together from the two aligned source dwords
// that hold its bytes (the second one may reach into the chunk's CRC field, never beyond it), and single bytes at both ends.
// The CRC pass, where lane i walks segment i, then finds the chunk in the cache; it loads aligned dwords as well, one per four
// bytes of its segment (the first and the last may reach up to 3 bytes outside the chunk, inside the 256-byte aligned upload
// and its 16 bytes of padding).
__global__ void __launch_bounds__(256) png_unpack_kernel(PngUnpackArgs a)
{
	__shared__ uint32_t table[256];
	__shared__ uint32_t wave_crc[4];
	const int tid = threadIdx.x;
	const PngChunk c = a.chunks[blockIdx.x];
	const uint8_t *__restrict__ src = a.files + c.src;  // type, data, CRC
	const uint32_t len = c.len;
	crc32_table_entry(table, tid);
	if (c.file & PNG_CHUNK_IDAT) {
		uint8_t *__restrict__ dst = a.streams + c.dst;
		const uint8_t *__restrict__ data = src + 4;
		const uint32_t head = min(len, (uint32_t)(4u - ((uintptr_t)dst & 3u)) & 3u), nw = (len - head) >> 2, tail = head + 4 * nw;
		if ((uint32_t)tid < head) dst[tid] = data[tid];
		if ((uint32_t)tid < len - tail) dst[tail + tid] = data[tail + tid];
		uint32_t *__restrict__ dw = reinterpret_cast<uint32_t *>(dst + head);
		const uintptr_t s1 = (uintptr_t)(data + head);
		const uint32_t sh = (uint32_t)(s1 & 3u) * 8u;
		const uint32_t *__restrict__ sw = reinterpret_cast<const uint32_t *>(s1 & ~(uintptr_t)3);
		if (sh == 0) {
#pragma unroll 8
			for (uint32_t w = (uint32_t)tid; w < nw; w += 256) dw[w] = sw[w];
		} else {
#pragma unroll 8
			for (uint32_t w = (uint32_t)tid; w < nw; w += 256) dw[w] = (sw[w] >> sh) | (sw[w + 1] << (32u - sh));
		}
	}
	__syncthreads();
	const uint32_t *word = reinterpret_cast<const uint32_t *>((uintptr_t)src & ~(uintptr_t)3);
	const uint32_t off = (uint32_t)((uintptr_t)src & 3u);
	uint32_t cur = 0, cur_w = 0xFFFFFFFFu;
	const uint32_t crc = crc32_workgroup(4 + len, table, wave_crc, [&](uint32_t j) -> uint32_t {
		const uint32_t w = (j + off) >> 2;
		if (w != cur_w) { cur = word[w]; cur_w = w; }
		return (cur >> (((j + off) & 3u) * 8u)) & 255u;
	});
	if (tid == 0) {
		const uint8_t *q = src + 4 + (size_t)len;
		const uint32_t stored = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
		if (crc != stored) atomicOr(&a.status[c.file & ~PNG_CHUNK_IDAT], PNG_ST_CRC);
	}
}

// ---- unfilter ------------------------------------------------------------------------------------------------------------
// Byte (r, i) of a row needs bytes (r, i - bpp), (r - 1, i) and (r - 1, i - bpp) (Average, Paeth), so a pixel needs its left,
// upper and upper-left neighbours.  A wave takes a band of 64 rows, lane j row j, as a skewed wavefront: at step t lane j
// reconstructs pixel t - j.  Its left neighbour is its own previous result; the pixel above is what lane j - 1 produced at step
// t - 1 (one __shfl_up: a one-lane neighbour read, not one of the scans of wave_device.h), the upper-left one what it produced at
// step t - 2, i.e. the previous "above".  Lane 0 reads the row above the band.  Outside 0 <= t - j < cols a lane produces 0, which is what row and column -1 are.
//
// Input and output go through LDS in tiles of 64 columns.  Superstep s (steps 64 s .. 64 s + 63) touches pixels
// 64 s - 63 .. 64 s + 63, tiles s - 1 and s of a ring of two; it loads tile s first (row by row, the lanes across the columns),
// reconstructs in place, and then tile s - 1 is complete in every row and leaves as uint16, again row by row.  A band
// of `cols` columns takes NT + 1 supersteps, NT = ceil(cols / 64).
//
// The last row of a band is the row above the next band.  Its reconstructed bytes go back in place into the inflated rows
// (the workspace is the library's own), from where the next band loads them into row 64 of its tiles.
//
// Waves per image: the workgroup's waves take the bands round-robin and run their supersteps in lockstep, three barriers per
// global superstep (load | reconstruct | store).  Band b + 1 needs tile s of band b's last row when it loads its tile s;
// band b stores that tile at the end of its superstep s + 1.  So band b + 1 runs two supersteps behind band b, and a wave's
// next band starts when its previous one has ended: band b starts at global superstep
//     (b / NW) * max(NT + 1, 2 NW) + 2 (b % NW).
constexpr int UF_PITCH = 262;  // bytes per LDS row: 128 two-byte pixels + 6.  Lane j reads pixel t - j at byte 260 j + 2 t: bank 65 j + t / 2
constexpr int UF_WAVE_LDS = 65 * UF_PITCH + 2;  // 64 rows of the band and the row above; a multiple of 4

__device__ __forceinline__ uint32_t unfilter_byte(uint32_t f, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
	const uint32_t pred = f == 1 ? a : f == 2 ? b : f == 3 ? (a + b) >> 1 : f == 4 ? paeth(a, b, c) : 0u;
	return (x + pred) & 255u;
}

template <int BPP>
__device__ __forceinline__ uint32_t lds_px(const uint8_t *row, int x)
{
	if (BPP == 2) return *reinterpret_cast<const uint16_t *>(row + 2 * (x & 127));
	return row[x & 127];
}
template <int BPP>
__device__ __forceinline__ void lds_px_set(uint8_t *row, int x, uint32_t v)
{
	if (BPP == 2) *reinterpret_cast<uint16_t *>(row + 2 * (x & 127)) = (uint16_t)v;
	else row[x & 127] = (uint8_t)v;
}
// a pixel's bytes in file order from the low byte up: byte 0 of a 16-bit sample is its high byte
template <int BPP>
__device__ __forceinline__ uint32_t px_load(const uint8_t *p)
{
	return BPP == 2 ? (uint32_t)p[0] | ((uint32_t)p[1] << 8) : (uint32_t)p[0];
}

template <int BPP>
__device__ void unfilter_image(const PngUnfilterArgs &a, int img, uint8_t *lds)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = blockDim.x >> 6;
	const int rows = a.nrows, cols = a.cols, shift = a.shift;
	const size_t pitch = 1 + (size_t)cols * BPP;
	uint8_t *in = a.rows + (size_t)img * a.rows_stride;
	uint16_t *out = a.images + (size_t)img * rows * cols;
	uint8_t *L = lds + wave * UF_WAVE_LDS, *Lrow = L + lane * UF_PITCH, *Ltop = L + 64 * UF_PITCH;
	const int NT = (cols + 63) >> 6, S = NT + 1, nbands = (rows + 63) >> 6;
	const long long period = max(S, 2 * NW);
	const long long G = (long long)((nbands - 1) / NW) * period + 2 * ((nbands - 1) % NW) + S;
	int b = wave;
	long long start = 2 * wave;
	uint32_t f = 0, left = 0, up_prev = 0, mine = 0;
	bool bad = false;
	for (long long g = 0; g < G; g++) {
		const bool active = b < nbands && g >= start && g < start + S;  // wave-uniform
		const int s = (int)(g - start), r0 = b * 64, nr = min(64, rows - r0);
		const bool row_ok = active && lane < nr;
		if (active) {  // load tile s
			if (s == 0) {
				f = row_ok ? in[(size_t)(r0 + lane) * pitch] : 0u;
				if (f > 4u) { bad = true; f = 0; }
				left = up_prev = mine = 0;
			}
			const int x = s * 64 + lane;
			if (s < NT && x < cols) {
				const uint8_t *col = in + 1 + (size_t)x * BPP;
				const uint32_t top = r0 ? px_load<BPP>(col + (size_t)(r0 - 1) * pitch) : 0u;
				for (int q = 0; q < nr; q += 32) {  // 32 rows' loads in flight, then their LDS stores
					uint32_t v[32];
#pragma unroll
					for (int k = 0; k < 32; k++) v[k] = q + k < nr ? px_load<BPP>(col + (size_t)(r0 + q + k) * pitch) : 0u;
#pragma unroll
					for (int k = 0; k < 32; k++)
						if (q + k < nr) lds_px_set<BPP>(L + (q + k) * UF_PITCH, x, v[k]);
				}
				lds_px_set<BPP>(Ltop, x, top);
			}
		}
		__syncthreads();
		if (active) {
			for (int k = 0; k < 64; k++) {
				const int t = s * 64 + k, x = t - lane;
				uint32_t up = (uint32_t)__shfl_up((int)mine, 1, 64);
				if (lane == 0) up = t < cols ? lds_px<BPP>(Ltop, t) : 0u;
				uint32_t o = 0;
				if (row_ok && x >= 0 && x < cols) {
					const uint32_t v = lds_px<BPP>(Lrow, x);
					o = unfilter_byte(f, v & 255u, left & 255u, up & 255u, up_prev & 255u);
					if (BPP == 2) o |= unfilter_byte(f, v >> 8, left >> 8, up >> 8, up_prev >> 8) << 8;
					lds_px_set<BPP>(Lrow, x, o);
					left = o;
				}
				up_prev = up;
				mine = o;
			}
		}
		__syncthreads();
		if (active) {
			if (s >= 1) {  // tile s - 1 is complete
				const int x = (s - 1) * 64 + lane;
				if (x < cols) {
					for (int rr = 0; rr < nr; rr++) {
						const uint32_t v = lds_px<BPP>(L + rr * UF_PITCH, x);
						const uint32_t smp = BPP == 2 ? ((v & 255u) << 8) | (v >> 8) : v;
						out[(size_t)(r0 + rr) * cols + x] = (uint16_t)(smp >> shift);
					}
					if (r0 + 64 < rows) {  // a band follows
						const uint32_t v = lds_px<BPP>(L + 63 * UF_PITCH, x);
						uint8_t *p = in + (size_t)(r0 + 63) * pitch + 1 + (size_t)x * BPP;
						p[0] = (uint8_t)v;
						if (BPP == 2) p[1] = (uint8_t)(v >> 8);
					}
				}
			}
			if (s == S - 1) {
				b += NW;
				start = (long long)(b / NW) * period + 2 * (b % NW);
			}
		}
		__syncthreads();
	}
	if (bad) atomicOr(&a.status[img], PNG_ST_FILTER);
}

// One workgroup per image.  A file that has failed so far, or whose stream did not inflate to exactly its rows, is left alone.
__global__ void __launch_bounds__(512) png_unfilter_kernel(PngUnfilterArgs a)
{
	CCT_PNG_DYNAMIC_LDS(uf_lds);
	const int img = blockIdx.x;
	const uint32_t bpp = a.bpp[img] == 1 ? 1u : 2u;
	const uint32_t want = (uint32_t)a.nrows * (1u + (uint32_t)a.cols * bpp);
	if (a.status[img] || a.zstatus[img] || a.row_sizes[img] != want) return;
	if (bpp == 2) unfilter_image<2>(a, img, uf_lds);
	else unfilter_image<1>(a, img, uf_lds);
}

}  // namespace

hipError_t launch_png_unpack(const PngUnpackArgs &a, uint32_t n_chunks, hipStream_t st)
{
	if (n_chunks == 0) return hipSuccess;
	hipLaunchKernelGGL(png_unpack_kernel, dim3(n_chunks), dim3(256), 0, st, a);
	return hipGetLastError();
}

hipError_t launch_png_unfilter(const PngUnfilterArgs &a, int n, int waves, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	if (waves != 1 && waves != 2 && waves != 4 && waves != 8) waves = PNG_UNFILTER_WAVES;
	const size_t lds = (size_t)waves * UF_WAVE_LDS;
	hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(png_unfilter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(64 * waves), lds, st, a);
	return hipGetLastError();
}

}  // namespace cct
