// The JPEG 2000 decoder on the host, for checks that need no GPU: csrc/jpeg2000_decode_kernels.hip and csrc/api_jpeg2000.cpp
// compile unchanged with g++ and run under AddressSanitizer / UBSan.  The shim of ../rle_host_emu stands in for the kernel
// side of the HIP runtime (a std::thread per GPU thread, the blocks of a launch one after another); this file adds the host
// side the entry point uses (allocations, copies, events) and the library's context.  So cct_j2k_decode_batch itself runs:
// the marker walk, the layout, the passes, the kernels.  drive.py compares it with tests/jpeg2000_decode_model.py.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I../rle_host_emu -x c++ emu.cpp -o emu -lpthread && python drive.py
// Bounds: a device allocation is a malloc of its own, and what DevBuf::ensure adds on top of the bytes the caller asked for is
// poisoned, so AddressSanitizer reports the first byte behind every buffer; the LDS of a launch is a malloc of exactly the
// launch's bytes.  Slow (a thread per lane): small shapes.  It checks the algorithm and the bounds, not the timing.
#define EMU_OWN_HOST_RUNTIME  // the host side of the runtime is this file's (below), not the shim's
#include "emu_common.h"
#include <sanitizer/asan_interface.h>
static uint32_t *g_dyn_lds;
#define J2K_DEC_DYNAMIC_LDS(name) uint32_t *name = g_dyn_lds
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) (g_dyn_lds = (uint32_t *)malloc((sh) ? (sh) : 1), emu_launch(k, g, b, __VA_ARGS__), free(g_dyn_lds))

// ---- the host side of the runtime ----
enum { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipHostMallocDefault };
static size_t asked(size_t want)  // DevBuf::ensure(bytes) allocates bytes + bytes / 8 + 4096
{
	size_t b = want > 4096 ? (want - 4096) * 8 / 9 : 0;
	while (b + b / 8 + 4096 < want) b++;
	while (b && b + b / 8 + 4096 > want) b--;
	return b;
}
static hipError_t hipMalloc(void **p, size_t want)
{
	*p = malloc(want);
	memset(*p, 0xEE, want);
	ASAN_POISON_MEMORY_REGION((char *)*p + asked(want), want - asked(want));
	return *p ? hipSuccess : 1;
}
static hipError_t hipHostMalloc(void **p, size_t n, int) { *p = malloc(n); return hipSuccess; }
static hipError_t hipFree(void *p) { free(p); return hipSuccess; }
static hipError_t hipHostFree(void *p) { free(p); return hipSuccess; }
static hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
static hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
static hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
static hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)1; return hipSuccess; }
static hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
static hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0; return hipSuccess; }
static hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
static const char *hipGetErrorString(hipError_t) { return "emulated"; }

#include "../../../2023-compact-image-compression_amd/csrc/jpeg2000_decode_kernels.hip"
#include "../../../2023-compact-image-compression_amd/csrc/api_jpeg2000.cpp"

// ---- the library's context ----
namespace cct {
QuiesceLock g_quiesce;
thread_local int tl_api_depth;
std::mutex g_mu;
static char g_err[512];
int fail(int code, const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); return code; }
int ensure_ctx(int) { return CCT_OK; }
hipStream_t main_stream() { return nullptr; }
int lease_decode_slot(DecLease &l) { l.stream = nullptr; l.slot = 0; return CCT_OK; }
void set_last_kernel_ms(bool, float) {}
hipError_t launch_j2k_encode(const J2kArgs &, hipStream_t) { return hipSuccess; }  // the encoder has an emulation of its own
}  // namespace cct

// emu rows cols bits shift in.bin out.bin; in.bin: u32 n, n + 1 u64 offsets, the files; out.bin: i32 rc, n u32 statuses, n rasters
int main(int argc, char **argv)
{
	if (argc != 7) { printf("usage\n"); return 2; }
	const int rows = atoi(argv[1]), cols = atoi(argv[2]), bits = atoi(argv[3]), shift = atoi(argv[4]);
	std::ifstream in(argv[5], std::ios::binary);
	std::vector<uint8_t> d((std::istreambuf_iterator<char>(in)), {});
	uint32_t n;
	memcpy(&n, d.data(), 4);
	std::vector<uint64_t> offs(n + 1);
	memcpy(offs.data(), d.data() + 4, (n + 1) * 8);
	const size_t blob_at = 4 + (n + 1) * 8, blob_len = d.size() - blob_at, img_bytes = (size_t)n * rows * cols * (bits / 8);
	uint8_t *blob = (uint8_t *)malloc(blob_len ? blob_len : 1);  // mallocs of their own: the sanitizer sees their ends
	memcpy(blob, d.data() + blob_at, blob_len);
	uint8_t *images = (uint8_t *)malloc(img_bytes ? img_bytes : 1);
	memset(images, 0xEE, img_bytes);
	std::vector<uint32_t> status(n, 0xEEEEEEEEu);
	const int rc = cct_j2k_decode_batch(blob, offs.data(), (int)n, rows, cols, bits, shift, images, 0, (size_t)n * rows * cols, status.data());
	std::ofstream out(argv[6], std::ios::binary);
	out.write((const char *)&rc, 4);
	out.write((const char *)status.data(), n * 4);
	out.write((const char *)images, img_bytes);
	free(images); free(blob);
	cct::j2k_release();
	return 0;
}
