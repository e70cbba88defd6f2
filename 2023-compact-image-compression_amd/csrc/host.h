// Host-side declarations shared by the translation units of libcompact_hip.so (api.cpp: context, encode, decode;
// api_comm.cpp: RCCL all-gather; api_packbits.cpp: PackBits utility; api_dicom_rle.cpp: DICOM RLE codec; api_jpeg_lossless.cpp: JPEG Lossless codec; api_jpeg_ls.cpp: JPEG-LS codec; api_jpeg2000.cpp: JPEG 2000 codec; api_tiff.cpp: TIFF writer and reader),
// and the scaffold every batch entry point is built from: StreamDrain, EventPair, Workspace, the decode slot lease, and the
// copies of a pass (rasters_to_device, files_to_host, good_rasters_to_host).  Not part of the C ABI.
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <condition_variable>
#include <mutex>
#include <optional>

#include <hip/hip_runtime.h>

#include "../../include/compact_hip.h"

namespace cct {

// last error of the calling thread (cct_last_error); returns `code` so that `return fail(...)` reads well
int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                          \
	do {                                                                                         \
		hipError_t e_ = (expr);                                                                    \
		if (e_ != hipSuccess)                                                                      \
			return ::cct::fail(CCT_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));         \
	} while (0)

// Runtime operations that are rare and heavy -- stream capture and graph instantiation / destruction, the per-shape table
// builds (device allocations plus SYNCHRONOUS copies), workspace growth, stream creation -- never run next to another call of
// the library: every entry point that drives the device holds `g_quiesce` shared from the moment it owns its slot (ApiCall), and
// those operations give it up and take it exclusively (exclusive_section).  Order: slot mutex, then g_quiesce; a thread waiting
// for a slot holds neither, and nobody waits for g_mu while it counts as a call in flight.
// Why: round 2 saw two concurrent encode calls hang inside the runtime about once in ten runs, one of them capturing its graphs
// for the first time.  Round 3 ran the suspects side by side without a lock (tools/debug/capture_vs_free.cpp,
// profiles/r03_capture_vs_free.log): allocations, frees, pinned allocations and stream creation next to an open capture neither
// stalled nor failed; a SYNCHRONOUS hipMemcpy (default stream) did -- hipStreamEndCapture then reports "capturing stream has
// unjoined work" and the runtime dies.  The library's synchronous copies are the table builds (get_tables), which a second
// thread could reach while the first one captured; they are inside the exclusive section now, and no steady-state path copies
// synchronously any more.
struct QuiesceLock {  // shared / exclusive with priority for the exclusive side (glibc's rwlock prefers readers: with three
	std::mutex m;        // threads issuing calls back to back an exclusive section could wait for a long time)
	std::condition_variable cv;
	int readers = 0, writers_waiting = 0;
	bool writer = false;
	void lock_shared() { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !writer && writers_waiting == 0; }); readers++; }
	void unlock_shared() { std::unique_lock<std::mutex> l(m); if (--readers == 0) cv.notify_all(); }
	void lock() { std::unique_lock<std::mutex> l(m); writers_waiting++; cv.wait(l, [&] { return !writer && readers == 0; }); writers_waiting--; writer = true; }
	void unlock() { std::unique_lock<std::mutex> l(m); writer = false; cv.notify_all(); }
};
extern QuiesceLock g_quiesce;
extern thread_local int tl_api_depth;
struct ApiCall {
	ApiCall() { if (tl_api_depth++ == 0) g_quiesce.lock_shared(); }
	~ApiCall() { if (--tl_api_depth == 0) g_quiesce.unlock_shared(); }
	ApiCall(const ApiCall &) = delete;
	ApiCall &operator=(const ApiCall &) = delete;
};
template <class F>
auto exclusive_section(F f) -> decltype(f())
{
	const bool shared = tl_api_depth > 0;
	if (shared) g_quiesce.unlock_shared();
	g_quiesce.lock();
	struct Back { bool shared; ~Back() { g_quiesce.unlock(); if (shared) g_quiesce.lock_shared(); } } back{shared};
	return f();
}

struct DevBuf {  // grow-only device (or pinned host) buffer
	void *p = nullptr;
	size_t cap = 0;
	bool pinned_host = false;
	int ensure(size_t bytes)
	{
		if (bytes <= cap) return CCT_OK;
		return exclusive_section([&]() -> int {
			release();
			const size_t want = bytes + bytes / 8 + 4096;
			hipError_t e = pinned_host ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
			if (e != hipSuccess) { p = nullptr; cap = 0; return fail(CCT_E_NOMEM, "allocation of %zu bytes failed: %s", want, hipGetErrorString(e)); }
			cap = want;
			return CCT_OK;
		});
	}
	// hipFree / hipHostFree wait for the whole device: callers run them inside an exclusive section (ensure() does) or with
	// every stream of the library drained (cct_shutdown)
	void release()
	{
		if (p) { if (pinned_host) (void)hipHostFree(p); else (void)hipFree(p); }
		p = nullptr; cap = 0;
	}
};

extern std::mutex g_mu;          // device context, main stream (and with it encode slot 0), every plumbing call
int ensure_ctx(int device = -1); // binds the device on first use (call with g_mu held); CCT_E_DEVICE in a child forked after that
hipStream_t main_stream();       // valid once ensure_ctx() has succeeded
int bound_device();
bool forked_after_init();        // this process is a fork() child of the one that initialised the device
void comm_release();             // cct_shutdown: drop the communicator and its buffers (api_comm.cpp)

// ---- the scaffold of a batch entry point ----
// Asynchronous copies that target locals (std::vector on the stack frame) or caller memory must have landed before an
// error return unwinds the frame: declare one of these AFTER those locals; it drains the stream unless disarmed.
struct StreamDrain {
	hipStream_t s; bool armed = true;
	explicit StreamDrain(hipStream_t st) : s(st) {}
	~StreamDrain() { if (armed) (void)hipStreamSynchronize(s); }
	void disarm() { armed = false; }
};

// Timing events around the kernels of a pass, created on first use: begin, end, and once the stream is synchronised add_ms.
struct EventPair {
	hipEvent_t e0 = nullptr, e1 = nullptr;
	int begin(hipStream_t st)
	{
		if (!e0) HIP_TRY(hipEventCreate(&e0));
		if (!e1) HIP_TRY(hipEventCreate(&e1));
		HIP_TRY(hipEventRecord(e0, st));
		return CCT_OK;
	}
	int end(hipStream_t st) { HIP_TRY(hipEventRecord(e1, st)); return CCT_OK; }
	int add_ms(float &sum) { float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, e0, e1)); sum += ms; return CCT_OK; }
	void release() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); e0 = e1 = nullptr; }
};

// What a codec outside api.cpp keeps per slot: N grow-only buffers, which an enum of the codec names, and its timing events.
template <int N>
struct Workspace {
	DevBuf buf[N];
	EventPair ev;
	void release() { for (DevBuf &b : buf) b.release(); ev.release(); }  // cct_shutdown, every stream drained
};

// A decode slot taken for one call, as every decode-side entry point takes one: its lock, the call's share of g_quiesce
// (given up before the lock: members go in reverse order), its stream and its index (DecSlot in api.cpp; a codec outside
// api.cpp keeps a workspace of its own per slot).
constexpr int DEC_SLOTS = 2;
struct DecLease { std::unique_lock<std::mutex> lk; std::optional<ApiCall> in_call; hipStream_t stream = nullptr; int slot = 0; };
int lease_decode_slot(DecLease &l);
void set_last_kernel_ms(bool encode, float ms);  // cct_last_timings [0] / [4] of the calling thread
void dicom_rle_release();        // cct_shutdown: workspaces and events of api_dicom_rle.cpp
void jpegll_release();           // cct_shutdown: workspaces and events of api_jpeg_lossless.cpp
void jpegls_release();           // cct_shutdown: workspaces and events of api_jpeg_ls.cpp
void j2k_release();              // cct_shutdown: workspaces and events of api_jpeg2000.cpp
void tiff_release();             // cct_shutdown: workspaces and events of api_tiff.cpp
// The DEFLATE pass of encode slot 0 for a codec outside api.cpp.  The caller holds g_mu, counts as a call (ApiCall) and has
// bound the device: n strings of d_in_sizes[i] bytes at d_in + i * in_stride (deflate_in_stride of the longest, the padding
// zero) -> zlib streams of `level` (4 .. 9), default strategy, memLevel 8, on the main stream.  Stream i starts 13 bytes
// into *d_out + i * out_stride (deflate_out_stride); (*d_out_sizes)[i] counts those 13 bytes too.  Both belong to the slot.
int deflate_on_main(const uint8_t *d_in, size_t in_stride, const uint32_t *d_in_sizes, int n, size_t out_stride, int level,
                    const uint8_t **d_out, const uint32_t **d_out_sizes);
int inflate_lanes_for_call();    // launch_inflate's `lanes` as cct_zlib_decompress_batch picks them (option "inflate_lanes")

// h_offsets[0 .. n] of an archive must not decrease; `noun` is what the caller's message calls an entry ("frame", "file")
inline int check_offsets(const uint64_t *h_offsets, int n, const char *noun)
{
	for (int i = 0; i < n; i++)
		if (h_offsets[i + 1] < h_offsets[i]) return fail(CCT_E_ARG, "%s offsets must not decrease", noun);
	return CCT_OK;
}

// The rasters of one pass, rasters c0 .. c0 + nc - 1 of img_bytes each: on the device already, they stay where they are;
// from the host they are copied into `buf`, grown to hold them.  *d_img: where the pass's first raster is on the device.
inline int rasters_to_device(const void *images, int images_on_device, int c0, int nc, size_t img_bytes, DevBuf &buf, hipStream_t st,
                             const void **d_img)
{
	*d_img = (const uint8_t *)images + (size_t)c0 * img_bytes;
	if (images_on_device) return CCT_OK;
	if (int rc = buf.ensure((size_t)nc * img_bytes)) return rc;
	HIP_TRY(hipMemcpyAsync(buf.p, *d_img, (size_t)nc * img_bytes, hipMemcpyHostToDevice, st));
	*d_img = buf.p;
	return CCT_OK;
}

// The files of one pass back to the caller, once their sizes are on the host: file i is h_sizes[i] bytes at
// d_files + i * d_stride + skip and goes to h_out + i * out_stride; a size of 0 copies nothing.  A size above `limit` is
// the device's mistake and refuses the call ("<noun> <index0 + i>: size .. beyond its <limit_name>").  The copies have landed on return.
inline int files_to_host(uint8_t *h_out, size_t out_stride, const uint32_t *h_sizes, int nc, const void *d_files, size_t d_stride,
                         size_t skip, size_t limit, const char *noun, int index0, const char *limit_name, hipStream_t st)
{
	for (int i = 0; i < nc; i++) {
		if (h_sizes[i] > limit) return fail(CCT_E_DEVICE, "%s %d: size %u beyond its %s", noun, index0 + i, h_sizes[i], limit_name);
		if (h_sizes[i])
			HIP_TRY(hipMemcpyAsync(h_out + (size_t)i * out_stride, (const uint8_t *)d_files + (size_t)i * d_stride + skip, h_sizes[i],
			                       hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(hipStreamSynchronize(st));
	return CCT_OK;
}

// The rasters of one pass (frames c0 .. c1 - 1 of the batch, frame_bytes each, the first at d_img) back to the caller's
// `images`, the good ones only and in runs: a refused frame (h_status not CCT_OK) leaves its slot in host memory alone.
inline int good_rasters_to_host(void *images, const uint8_t *d_img, size_t frame_bytes, const uint32_t *h_status, int c0, int c1,
                                hipStream_t st)
{
	for (int i = c0; i < c1;) {
		if (h_status[i] != CCT_OK) { i++; continue; }
		int j = i + 1;
		while (j < c1 && h_status[j] == CCT_OK) j++;
		HIP_TRY(hipMemcpyAsync((uint8_t *)images + (size_t)i * frame_bytes, d_img + (size_t)(i - c0) * frame_bytes,
		                       (size_t)(j - i) * frame_bytes, hipMemcpyDeviceToHost, st));
		i = j;
	}
	HIP_TRY(hipStreamSynchronize(st));
	return CCT_OK;
}

}  // namespace cct
