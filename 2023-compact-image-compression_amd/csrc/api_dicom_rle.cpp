// DICOM RLE Lossless frames behind the C ABI: host side of dicom_rle_kernels.hip.  Encode takes the encode slot (g_mu, the
// main stream), decode a decode slot (lease_decode_slot); passes, copies and timing are the scaffold of host.h.  The
// workspaces are this file's own, one for the encode slot and one per decode slot.  The host parses the 64-byte frame
// headers; everything behind the header is the device's.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "cct_internal.h"
#include "host.h"

using namespace cct;

namespace {

constexpr size_t RLE_MAX_PIXELS = (size_t)1 << 26;   // rows * cols: a 16-bit frame of that many stays below 2^28 + 64 bytes
constexpr size_t RLE_PASS_BYTES = (size_t)512 << 20;  // frames on the device at a time (one frame at least)

enum { E_IMG, E_ROWINFO, E_OUT, E_SIZES, E_NBUF };
enum { D_FRAMES, D_SEGS, D_TABLE, D_TINFO, D_SHORT_SEG, D_IMG, D_NBUF };
Workspace<E_NBUF> g_enc_ws;             // under g_mu
Workspace<D_NBUF> g_dec_ws[DEC_SLOTS];  // under the slot's lock

int check_shape(int n, int rows, int cols, int bits)
{
	if (bits != 8 && bits != 16) return fail(CCT_E_ARG, "DICOM RLE: %d bits allocated: 8 or 16", bits);
	if (rows < 1 || cols < 1) return fail(CCT_E_ARG, "DICOM RLE shape %d x %d: rows and cols must be >= 1", rows, cols);
	if ((size_t)rows * (size_t)cols > RLE_MAX_PIXELS)
		return fail(CCT_E_ARG, "DICOM RLE shape %d x %d: more than %zu pixels", rows, cols, RLE_MAX_PIXELS);
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	return CCT_OK;
}

uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// header of one frame -> its segments' (offset, length), or CCT_E_STREAM
int parse_frame(const uint8_t *f, size_t len, int nseg, uint32_t seg_off[2], uint32_t seg_len[2])
{
	if (len < 64 || len > 0xFFFFFFFFull) return CCT_E_STREAM;
	if (le32(f) != (uint32_t)nseg) return CCT_E_STREAM;
	for (int k = 0; k < nseg; k++) seg_off[k] = le32(f + 4 + 4 * k);
	if (seg_off[0] != 64) return CCT_E_STREAM;
	for (int k = 0; k < nseg; k++) {
		if (seg_off[k] > len) return CCT_E_STREAM;
		if (k && seg_off[k] <= seg_off[k - 1]) return CCT_E_STREAM;
	}
	for (int k = 0; k < nseg; k++) {
		seg_len[k] = (k + 1 < nseg ? seg_off[k + 1] : (uint32_t)len) - seg_off[k];
		if (seg_len[k] == 0) return CCT_E_STREAM;  // an empty segment yields nothing
	}
	return CCT_OK;
}

}  // namespace

void cct::dicom_rle_release()
{
	g_enc_ws.release();
	for (auto &w : g_dec_ws) w.release();
}

extern "C" {

size_t cct_dicom_rle_bound(int rows, int cols, int bits)
{
	if ((bits != 8 && bits != 16) || rows < 1 || cols < 1 || (size_t)rows * (size_t)cols > RLE_MAX_PIXELS) return 0;
	return 64 + (size_t)(bits / 8) * 2 * (size_t)rows * (size_t)cols;  // a byte costs two at worst (a row of one, a remainder of one)
}

int cct_dicom_rle_encode_batch(const void *images, int images_on_device, int n, int rows, int cols, int bits, uint8_t *h_out,
                               size_t out_stride, uint32_t *h_out_sizes)
{
	int rc = check_shape(n, rows, cols, bits);
	if (rc) return rc;
	const size_t bound = cct_dicom_rle_bound(rows, cols, bits);
	if (out_stride < bound) return fail(CCT_E_CAP, "out_stride %zu too small (need cct_dicom_rle_bound = %zu)", out_stride, bound);
	if (n > 0 && (!images || !h_out || !h_out_sizes)) return fail(CCT_E_ARG, "null argument");
	if (n == 0) return CCT_OK;
	std::lock_guard<std::mutex> lk(g_mu);
	ApiCall in_call;
	if ((rc = ensure_ctx())) return rc;
	hipStream_t st = main_stream();
	DevBuf *W = g_enc_ws.buf;
	EventPair &ev = g_enc_ws.ev;
	const int planes = bits / 8;
	const size_t N = (size_t)rows * cols, img_bytes = N * planes, dstride = (bound + 3) & ~(size_t)3;  // the header is written in words
	const int per_pass = (int)std::max<size_t>(1, RLE_PASS_BYTES / dstride);
	float ms_sum = 0;
	StreamDrain drain(st);  // copies into caller memory land before any return
	for (int c0 = 0; c0 < n; c0 += per_pass) {
		const int nc = std::min(per_pass, n - c0);
		const void *d_img;
		if ((rc = rasters_to_device(images, images_on_device, c0, nc, img_bytes, W[E_IMG], st, &d_img))) return rc;
		if ((rc = W[E_ROWINFO].ensure((size_t)nc * planes * rows * 4))) return rc;
		if ((rc = W[E_OUT].ensure((size_t)nc * dstride))) return rc;
		if ((rc = W[E_SIZES].ensure((size_t)nc * 4))) return rc;
		if ((rc = ev.begin(st))) return rc;
		HIP_TRY(launch_dicom_rle_encode(d_img, nc, rows, cols, planes, (uint32_t *)W[E_ROWINFO].p, (uint8_t *)W[E_OUT].p, dstride, (uint32_t *)W[E_SIZES].p, st));
		if ((rc = ev.end(st))) return rc;
		HIP_TRY(hipMemcpyAsync(h_out_sizes + c0, W[E_SIZES].p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		if ((rc = ev.add_ms(ms_sum))) return rc;
		if ((rc = files_to_host(h_out + (size_t)c0 * out_stride, out_stride, h_out_sizes + c0, nc, W[E_OUT].p, dstride, 0, dstride, "frame", c0, "bound", st)))
			return rc;
	}
	set_last_kernel_ms(true, ms_sum);
	return CCT_OK;
}

int cct_dicom_rle_decode_batch(const uint8_t *h_frames, const uint64_t *h_offsets, int n, int rows, int cols, int bits, void *images,
                               int images_on_device, size_t images_cap_px, uint32_t *h_status)
{
	int rc = check_shape(n, rows, cols, bits);
	if (rc) return rc;
	const size_t N = (size_t)rows * cols;
	if (images_cap_px / N < (size_t)n) return fail(CCT_E_CAP, "output holds %zu pixels, need %zu", images_cap_px, (size_t)n * N);
	if (n > 0 && (!h_frames || !h_offsets || !images || !h_status)) return fail(CCT_E_ARG, "null argument");
	if ((rc = check_offsets(h_offsets, n, "frame"))) return rc;
	if (n == 0) return CCT_OK;
	DecLease L;
	if ((rc = lease_decode_slot(L))) return rc;
	hipStream_t st = L.stream;
	DevBuf *W = g_dec_ws[L.slot].buf;
	EventPair &ev = g_dec_ws[L.slot].ev;
	const int nseg_frame = bits / 8;
	const size_t px_bytes = (size_t)nseg_frame;
	float ms_sum = 0;
	std::vector<RleSegment> segs;
	std::vector<int> seg_frame;
	std::vector<uint32_t> short_seg;
	StreamDrain drain(st);  // declared after the vectors the copies land in
	for (int c0 = 0; c0 < n;) {
		// a pass: frames c0 .. c1 - 1, RLE_PASS_BYTES of them at most
		int c1 = c0 + 1;
		while (c1 < n && h_offsets[c1 + 1] - h_offsets[c0] <= RLE_PASS_BYTES && (size_t)(c1 + 1 - c0) * N * px_bytes <= 2 * RLE_PASS_BYTES) c1++;
		const uint64_t a0 = h_offsets[c0], a1 = h_offsets[c1];
		segs.clear(); seg_frame.clear();
		uint64_t ntiles = 0;
		for (int i = c0; i < c1; i++) {
			uint32_t so[2] = {0, 0}, sl[2] = {0, 0};
			h_status[i] = (uint32_t)parse_frame(h_frames + h_offsets[i], (size_t)(h_offsets[i + 1] - h_offsets[i]), nseg_frame, so, sl);
			if (h_status[i] != CCT_OK) continue;
			for (int k = 0; k < nseg_frame; k++) {
				RleSegment s{};
				s.src = h_offsets[i] - a0 + so[k];
				s.dst = (size_t)(i - c0) * N * px_bytes + (size_t)(nseg_frame - 1 - k);  // little-endian pixels: segment 0 is the high byte
				s.len = sl[k];
				s.tile0 = (uint32_t)ntiles;
				ntiles += ((uint64_t)sl[k] + RLE_TILE - 1) / RLE_TILE;
				segs.push_back(s); seg_frame.push_back(i);
			}
		}
		if (!segs.empty()) {
			if (ntiles > 0x7FFFFFFFull) return fail(CCT_E_ARG, "DICOM RLE: too many coded bytes in one pass");
			const size_t abytes = (size_t)(a1 - a0), nseg = segs.size();
			uint8_t *d_img = images_on_device ? (uint8_t *)images + (size_t)c0 * N * px_bytes : nullptr;
			if (!images_on_device) {
				if ((rc = W[D_IMG].ensure((size_t)(c1 - c0) * N * px_bytes))) return rc;
				d_img = (uint8_t *)W[D_IMG].p;
			}
			if ((rc = W[D_FRAMES].ensure(abytes + 16))) return rc;
			if ((rc = W[D_SEGS].ensure(nseg * sizeof(RleSegment)))) return rc;
			if ((rc = W[D_TABLE].ensure((size_t)ntiles * RLE_ENTRIES * 4))) return rc;
			if ((rc = W[D_TINFO].ensure((size_t)ntiles * sizeof(uint2)))) return rc;
			if ((rc = W[D_SHORT_SEG].ensure(nseg * 4))) return rc;
			HIP_TRY(hipMemcpyAsync(W[D_FRAMES].p, h_frames + a0, abytes, hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(W[D_SEGS].p, segs.data(), nseg * sizeof(RleSegment), hipMemcpyHostToDevice, st));
			RleDecodeArgs a{};
			a.frames = (const uint8_t *)W[D_FRAMES].p; a.segs = (const RleSegment *)W[D_SEGS].p;
			a.nseg = (uint32_t)nseg; a.ntiles = (uint32_t)ntiles;
			a.want = (uint32_t)N; a.step = (uint32_t)px_bytes;
			a.table = (uint32_t *)W[D_TABLE].p; a.tinfo = (uint2 *)W[D_TINFO].p; a.short_seg = (uint32_t *)W[D_SHORT_SEG].p;
			a.images = d_img;
			if ((rc = ev.begin(st))) return rc;
			HIP_TRY(launch_dicom_rle_decode(a, st));
			if ((rc = ev.end(st))) return rc;
			short_seg.assign(nseg, 0);
			HIP_TRY(hipMemcpyAsync(short_seg.data(), W[D_SHORT_SEG].p, nseg * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			if ((rc = ev.add_ms(ms_sum))) return rc;
			for (size_t s = 0; s < nseg; s++)
				if (short_seg[s]) h_status[seg_frame[s]] = CCT_E_STREAM;
			if (!images_on_device && (rc = good_rasters_to_host(images, d_img, N * px_bytes, h_status, c0, c1, st))) return rc;
		}
		c0 = c1;
	}
	set_last_kernel_ms(false, ms_sum);
	for (int i = 0; i < n; i++)
		if (h_status[i] != CCT_OK) return fail((int)h_status[i], "frame %d: not a DICOM RLE frame of this shape, or a segment that ends short", i);
	return CCT_OK;
}

}  // extern "C"
