// JPEG-LS lossless (T.87) files behind the C ABI: host side of jpeg_ls_kernels.hip.  Encode takes the encode slot (g_mu, the
// main stream), decode a decode slot (lease_decode_slot); passes, copies and timing are the scaffold of host.h.  The
// workspaces are this file's own, one for the encode slot and one per decode slot.  The host walks the header segments of
// every file, decides every structural refusal before anything is uploaded, and finds the markers inside the scan (0xFF and a
// byte >= 0x80): the device sees the byte range of every restart interval and the scan's coding parameters.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "cct_internal.h"
#include "host.h"

using namespace cct;

namespace {

constexpr size_t JLS_MAX_PIXELS = (size_t)1 << 26;
constexpr size_t JLS_PASS_BYTES = (size_t)512 << 20;  // device bytes of the frames of one pass (one frame at least)

enum { E_IMG, E_STAGE, E_INTS, E_OUT, E_SIZES, E_STATUS, E_NBUF };
enum { D_FILES, D_FRAMES, D_INTERVALS, D_STATUS, D_IMG, D_NBUF };
Workspace<E_NBUF> g_enc_ws;             // under g_mu
Workspace<D_NBUF> g_dec_ws[DEC_SLOTS];  // under the slot's lock

bool shape_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && rows <= 65535 && cols <= 65535 && (size_t)rows * (size_t)cols <= JLS_MAX_PIXELS; }

int check_shape(int n, int rows, int cols)
{
	if (!shape_ok(rows, cols))
		return fail(CCT_E_ARG, "JPEG-LS shape %d x %d: rows and cols 1 .. 65535, at most %zu pixels", rows, cols, JLS_MAX_PIXELS);
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	return CCT_OK;
}

uint32_t be16(const uint8_t *p) { return (uint32_t)p[0] << 8 | (uint32_t)p[1]; }

// T.87 C.2.4.1.1: the value is replaced by lo when it leaves [lo, hi], not saturated
int clamp_t(int i, int lo, int hi) { return (i > hi || i < lo) ? lo : i; }

uint32_t bit_length(uint32_t v) { uint32_t n = 0; while (v) { n++; v >>= 1; } return n; }

// The coding parameters of a scan of precision P: the defaults, or what an LSE segment of id 1 states (0: the default).
// false for values T.87 does not allow.
bool jls_params(int P, uint32_t maxval, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t reset, JlsParams &o)
{
	const uint32_t top = (1u << P) - 1u;
	if (maxval == 0) maxval = top;
	if (maxval > top) return false;
	const int mv = (int)maxval;
	int d1, d2, d3;
	if (mv >= 128) {
		const int f = (std::min(mv, 4095) + 128) >> 8;
		d1 = clamp_t(f + 2, 1, mv); d2 = clamp_t(4 * f + 3, d1, mv); d3 = clamp_t(17 * f + 4, d2, mv);
	} else {
		const int f = 256 / (mv + 1);
		d1 = clamp_t(std::max(2, 3 / f), 1, mv); d2 = clamp_t(std::max(3, 7 / f), d1, mv); d3 = clamp_t(std::max(4, 21 / f), d2, mv);
	}
	o.maxval = maxval;
	o.t1 = t1 ? (int)t1 : d1; o.t2 = t2 ? (int)t2 : d2; o.t3 = t3 ? (int)t3 : d3;
	o.reset = reset ? reset : 64u;
	o.range = maxval + 1u;
	o.qbpp = bit_length(o.range - 1u);
	const uint32_t bpp = std::max(2u, bit_length(maxval));
	o.limit = 2u * (bpp + std::max(8u, bpp));
	o.a0 = std::max(2u, (o.range + 32u) >> 6);
	return 1 <= o.t1 && o.t1 <= o.t2 && o.t2 <= o.t3 && o.t3 <= mv && o.reset >= 3 && o.reset <= std::max(255u, maxval);
}

struct Parsed {
	int P = 0, Y = 0, X = 0;
	uint32_t ri = 0;  // lines per restart interval, 0: none
	JlsParams par{};
	std::vector<std::pair<size_t, size_t>> intervals;  // [start, end) of every interval's bytes in the file
	bool rst_ok = true;                                 // the RST markers count 0, 1, .. 7, 0, ..
};

// The marker walk (tests/jpeg_ls_model.py parse()): CCT_OK or CCT_E_JPEGLS.  Every read is checked against len first.
int parse_file(const uint8_t *f, size_t len, Parsed &o)
{
	if (len < 4 || f[0] != 0xFF || f[1] != 0xD8) return CCT_E_JPEGLS;
	size_t pos = 2;
	bool sof = false, have_lse = false;
	int comp_id = 0;
	uint32_t lse[5] = {0, 0, 0, 0, 0};
	for (;;) {
		if (pos + 4 > len || f[pos] != 0xFF) return CCT_E_JPEGLS;
		const int m = f[pos + 1];
		if (m == 0xD8 || m == 0xD9 || m == 0x01 || m == 0xFF || m == 0x00 || (m >= 0xD0 && m <= 0xD7)) return CCT_E_JPEGLS;
		const size_t ln = be16(f + pos + 2);
		if (ln < 2 || pos + 2 + ln > len) return CCT_E_JPEGLS;
		const uint8_t *seg = f + pos + 4;
		const size_t sl = ln - 2;
		pos += 2 + ln;
		if (m == 0xF7) {
			if (sof || sl < 6 || sl != 6 + 3 * (size_t)seg[5]) return CCT_E_JPEGLS;
			o.P = seg[0]; o.Y = (int)be16(seg + 1); o.X = (int)be16(seg + 3);
			if (seg[5] != 1 || o.Y == 0 || o.X == 0 || o.P < 2 || o.P > 16) return CCT_E_JPEGLS;
			comp_id = seg[6];
			sof = true;
		} else if ((m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) || m == 0xF9) {
			return CCT_E_JPEGLS;  // another SOF type
		} else if (m == 0xF8) {
			if (sl != 11 || seg[0] != 1) return CCT_E_JPEGLS;  // ids 2 .. 4: mapping tables, oversize image dimensions
			for (int k = 0; k < 5; k++) lse[k] = be16(seg + 1 + 2 * k);
			have_lse = true;
		} else if (m == 0xDD) {
			if (sl < 2 || sl > 4) return CCT_E_JPEGLS;
			o.ri = 0;
			for (size_t k = 0; k < sl; k++) o.ri = o.ri << 8 | seg[k];
		} else if (m == 0xDC) {
			return CCT_E_JPEGLS;  // DNL
		} else if (m == 0xDA) {
			// one component, no mapping table, NEAR 0, ILV 0, no point transform
			if (!sof || sl != 6 || seg[0] != 1 || seg[1] != comp_id || seg[2] != 0 || seg[3] != 0 || seg[4] != 0 || seg[5] != 0) return CCT_E_JPEGLS;
			break;
		}  // APPn, COM and whatever else carries a length: skipped
	}
	if (!jls_params(o.P, have_lse ? lse[0] : 0, lse[1], lse[2], lse[3], lse[4], o.par)) return CCT_E_JPEGLS;
	size_t start = pos;
	for (size_t i = pos;;) {
		const uint8_t *q = i < len ? (const uint8_t *)memchr(f + i, 0xFF, len - i) : nullptr;
		if (!q || (size_t)(q - f) + 1 >= len) return CCT_E_JPEGLS;  // no EOI
		const size_t j = (size_t)(q - f);
		const int nx = f[j + 1];
		if (nx < 0x80) i = j + 2;
		else if (nx >= 0xD0 && nx <= 0xD7) {
			if ((size_t)(nx - 0xD0) != (o.intervals.size() & 7)) o.rst_ok = false;
			o.intervals.emplace_back(start, j);
			start = i = j + 2;
		} else if (nx == 0xD9) { o.intervals.emplace_back(start, j); break; }
		else return CCT_E_JPEGLS;  // any other marker inside the scan
	}
	return CCT_OK;
}

const char *refusal(int code)
{
	return code == CCT_E_JPEGLS  ? "not a JPEG-LS file this reader takes"
	       : code == CCT_E_MIXED ? "the frame's shape or precision is not the call's"
	                             : "scan data: it ends early or is left over, a wrong RST, a run past the end of a line, a value outside the range";
}

}  // namespace

void cct::jpegls_release()
{
	g_enc_ws.release();
	for (auto &w : g_dec_ws) w.release();
}

extern "C" {

// jls_interval_bound() (cct_internal.h) for every interval, two bytes of RST in front of all but the first, the headers and
// EOI within JLS_HDR_MAX + 2.
size_t cct_jpegls_bound(int rows, int cols, int restart_rows)
{
	if (!shape_ok(rows, cols) || restart_rows < 0 || restart_rows > 65535) return 0;
	const size_t rpi = restart_rows && restart_rows < rows ? (size_t)restart_rows : (size_t)rows, n_int = ((size_t)rows + rpi - 1) / rpi;
	return JLS_HDR_MAX + 2 + n_int * (jls_interval_bound(rpi, (size_t)cols) + 2);
}

int cct_jpegls_info(const uint8_t *h_file, size_t len, int *rows, int *cols, int *precision)
{
	if (!h_file || !rows || !cols || !precision) return fail(CCT_E_ARG, "null argument");
	Parsed p;
	const int rc = parse_file(h_file, len, p);
	if (rc) return fail(rc, "%s", refusal(rc));
	*rows = p.Y; *cols = p.X; *precision = p.P;
	return CCT_OK;
}

int cct_jpegls_encode_batch(const void *images, int images_on_device, int n, int rows, int cols, int src_bits, int precision, int restart_rows,
                            uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes, uint32_t *h_status)
{
	int rc = check_shape(n, rows, cols);
	if (rc) return rc;
	if (src_bits != 8 && src_bits != 16) return fail(CCT_E_ARG, "JPEG-LS: samples of %d bits: 8 or 16", src_bits);
	if (precision < 2 || precision > src_bits) return fail(CCT_E_ARG, "JPEG-LS: precision %d: 2 .. %d", precision, src_bits);
	if (restart_rows < 0 || restart_rows > 65535) return fail(CCT_E_ARG, "JPEG-LS: restart interval of %d lines: 0 .. 65535", restart_rows);
	const size_t bound = cct_jpegls_bound(rows, cols, restart_rows);
	if (out_stride < bound) return fail(CCT_E_CAP, "out_stride %zu too small (need cct_jpegls_bound = %zu)", out_stride, bound);
	if (n > 0 && (!images || !h_out || !h_out_sizes || !h_status)) return fail(CCT_E_ARG, "null argument");
	if (n == 0) return CCT_OK;
	std::lock_guard<std::mutex> lk(g_mu);
	ApiCall in_call;
	if ((rc = ensure_ctx())) return rc;
	hipStream_t st = main_stream();
	DevBuf *W = g_enc_ws.buf;
	EventPair &ev = g_enc_ws.ev;
	const size_t N = (size_t)rows * cols, img_bytes = N * (src_bits / 8), dstride = (bound + 3) & ~(size_t)3;
	const uint32_t rpi = restart_rows && restart_rows < rows ? (uint32_t)restart_rows : (uint32_t)rows, n_int = ((uint32_t)rows + rpi - 1) / rpi;
	const size_t istride = (jls_interval_bound(rpi, (size_t)cols) + 3) & ~(size_t)3;
	const int per_pass = (int)std::max<size_t>(1, JLS_PASS_BYTES / (dstride + n_int * istride));
	JlsParams par{};
	jls_params(precision, 0, 0, 0, 0, 0, par);
	float ms_sum = 0;
	std::vector<uint32_t> status;
	StreamDrain drain(st);  // copies into caller memory land before any return
	for (int c0 = 0; c0 < n; c0 += per_pass) {
		const int nc = std::min(per_pass, n - c0);
		const void *d_img;
		if ((rc = rasters_to_device(images, images_on_device, c0, nc, img_bytes, W[E_IMG], st, &d_img))) return rc;
		if ((rc = W[E_STAGE].ensure((size_t)nc * n_int * istride))) return rc;
		if ((rc = W[E_INTS].ensure((size_t)nc * n_int * 2 * 4))) return rc;
		if ((rc = W[E_OUT].ensure((size_t)nc * dstride))) return rc;
		if ((rc = W[E_SIZES].ensure((size_t)nc * 4))) return rc;
		if ((rc = W[E_STATUS].ensure((size_t)nc * 4))) return rc;
		JlsEncArgs a{};
		a.images = d_img; a.src_bits = (uint32_t)src_bits; a.n = (uint32_t)nc; a.rows = (uint32_t)rows; a.cols = (uint32_t)cols;
		a.precision = (uint32_t)precision; a.rpi = rpi; a.n_int = n_int; a.restart = (uint32_t)restart_rows;
		a.par = par;
		a.status = (uint32_t *)W[E_STATUS].p;
		a.stage = (uint8_t *)W[E_STAGE].p; a.istride = istride;
		a.ibytes = (uint32_t *)W[E_INTS].p; a.ioff = a.ibytes + (size_t)nc * n_int;
		a.out = (uint8_t *)W[E_OUT].p; a.out_stride = dstride; a.out_sizes = (uint32_t *)W[E_SIZES].p;
		if ((rc = ev.begin(st))) return rc;
		HIP_TRY(hipMemsetAsync(W[E_STATUS].p, 0, (size_t)nc * 4, st));
		HIP_TRY(launch_jls_encode(a, st));
		if ((rc = ev.end(st))) return rc;
		status.assign(nc, 0);
		HIP_TRY(hipMemcpyAsync(h_out_sizes + c0, W[E_SIZES].p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(status.data(), a.status, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		if ((rc = ev.add_ms(ms_sum))) return rc;
		for (int i = 0; i < nc; i++) {
			if (status[i] & JLS_ST_BOUND) return fail(CCT_E_DEVICE, "frame %d: the file left cct_jpegls_bound", c0 + i);
			h_status[c0 + i] = status[i] ? CCT_E_OVERFLOW : CCT_OK;
		}
		if ((rc = files_to_host(h_out + (size_t)c0 * out_stride, out_stride, h_out_sizes + c0, nc, W[E_OUT].p, dstride, 0, bound, "frame", c0, "bound", st)))
			return rc;
	}
	set_last_kernel_ms(true, ms_sum);
	for (int i = 0; i < n; i++)
		if (h_status[i] != CCT_OK) return fail((int)h_status[i], "frame %d: a sample does not fit the precision of %d bits", i, precision);
	return CCT_OK;
}

int cct_jpegls_decode_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int rows, int cols, int bits, void *images,
                            int images_on_device, size_t images_cap_px, uint32_t *h_status)
{
	int rc = check_shape(n, rows, cols);
	if (rc) return rc;
	if (bits != 8 && bits != 16) return fail(CCT_E_ARG, "JPEG-LS: %d bits allocated: 8 or 16", bits);
	const size_t N = (size_t)rows * cols, px_bytes = (size_t)bits / 8;
	if (images_cap_px / N < (size_t)n) return fail(CCT_E_CAP, "output holds %zu pixels, need %zu", images_cap_px, (size_t)n * N);
	if (n > 0 && (!h_files || !h_offsets || !images || !h_status)) return fail(CCT_E_ARG, "null argument");
	if ((rc = check_offsets(h_offsets, n, "file"))) return rc;
	if (n == 0) return CCT_OK;
	// the marker walk: every refusal that needs no decoding is decided here, before the device is touched
	std::vector<Parsed> parsed(n);
	for (int i = 0; i < n; i++) {
		const size_t len = (size_t)(h_offsets[i + 1] - h_offsets[i]);
		Parsed &p = parsed[i];
		int r = len > 0xFFFFFFFFull ? CCT_E_JPEGLS : parse_file(h_files + h_offsets[i], len, p);
		if (r == CCT_OK && (p.Y != rows || p.X != cols || p.P > bits)) r = CCT_E_MIXED;
		if (r == CCT_OK) {
			const uint32_t rpi = p.ri && p.ri < (uint32_t)rows ? p.ri : (uint32_t)rows, n_int = ((uint32_t)rows + rpi - 1) / rpi;
			if (p.intervals.size() != n_int || !p.rst_ok) r = CCT_E_STREAM;  // a wrong RST count or sequence
		}
		h_status[i] = (uint32_t)r;
	}
	if (std::all_of(h_status, h_status + n, [](uint32_t s) { return s != CCT_OK; }))  // nothing to send: no device needed
		return fail((int)h_status[0], "frame 0: %s", refusal((int)h_status[0]));
	DecLease L;
	if ((rc = lease_decode_slot(L))) return rc;
	hipStream_t st = L.stream;
	DevBuf *W = g_dec_ws[L.slot].buf;
	EventPair &ev = g_dec_ws[L.slot].ev;
	float ms_sum = 0;
	std::vector<JlsFrame> frames;
	std::vector<JlsInterval> ints;
	std::vector<uint32_t> status;
	std::vector<int> frame_of;
	StreamDrain drain(st);  // declared after the vectors the copies land in
	for (int c0 = 0; c0 < n;) {
		int c1 = c0 + 1;
		while (c1 < n && h_offsets[c1 + 1] - h_offsets[c0] <= JLS_PASS_BYTES / 4 && (size_t)(c1 + 1 - c0) * N * px_bytes <= JLS_PASS_BYTES) c1++;
		const uint64_t a0 = h_offsets[c0], a1 = h_offsets[c1];
		frames.clear(); ints.clear(); frame_of.clear();
		for (int i = c0; i < c1; i++) {
			if (h_status[i] != CCT_OK) continue;
			const Parsed &p = parsed[i];
			const uint32_t rpi = p.ri && p.ri < (uint32_t)rows ? p.ri : (uint32_t)rows;
			for (size_t k = 0; k < p.intervals.size(); k++) {
				JlsInterval v{};
				v.src = h_offsets[i] - a0 + p.intervals[k].first;
				v.len = (uint32_t)(p.intervals[k].second - p.intervals[k].first);
				v.frame = (uint32_t)frames.size();
				v.row0 = (uint32_t)k * rpi;
				v.nrows = std::min(rpi, (uint32_t)rows - v.row0);
				ints.push_back(v);
			}
			frames.push_back(JlsFrame{(uint32_t)(i - c0), p.par});
			frame_of.push_back(i);
		}
		if (!frames.empty()) {
			const size_t abytes = (size_t)(a1 - a0), nf = frames.size(), ni = ints.size();
			uint8_t *d_img = images_on_device ? (uint8_t *)images + (size_t)c0 * N * px_bytes : nullptr;
			if (!images_on_device) {
				if ((rc = W[D_IMG].ensure((size_t)(c1 - c0) * N * px_bytes))) return rc;
				d_img = (uint8_t *)W[D_IMG].p;
			}
			if ((rc = W[D_FILES].ensure(abytes + 16))) return rc;
			if ((rc = W[D_FRAMES].ensure(nf * sizeof(JlsFrame)))) return rc;
			if ((rc = W[D_INTERVALS].ensure(ni * sizeof(JlsInterval)))) return rc;
			if ((rc = W[D_STATUS].ensure(nf * 4))) return rc;
			HIP_TRY(hipMemcpyAsync(W[D_FILES].p, h_files + a0, abytes, hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(W[D_FRAMES].p, frames.data(), nf * sizeof(JlsFrame), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(W[D_INTERVALS].p, ints.data(), ni * sizeof(JlsInterval), hipMemcpyHostToDevice, st));
			JlsDecArgs a{};
			a.files = (const uint8_t *)W[D_FILES].p; a.frames = (const JlsFrame *)W[D_FRAMES].p; a.nframes = (uint32_t)nf;
			a.intervals = (const JlsInterval *)W[D_INTERVALS].p; a.total_int = (uint32_t)ni;
			a.rows = (uint32_t)rows; a.cols = (uint32_t)cols; a.out_bits = (uint32_t)bits;
			a.status = (uint32_t *)W[D_STATUS].p; a.images = d_img;
			if ((rc = ev.begin(st))) return rc;
			HIP_TRY(hipMemsetAsync(W[D_STATUS].p, 0, nf * 4, st));
			HIP_TRY(launch_jls_decode(a, st));
			if ((rc = ev.end(st))) return rc;
			status.assign(nf, 0);
			HIP_TRY(hipMemcpyAsync(status.data(), W[D_STATUS].p, nf * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			if ((rc = ev.add_ms(ms_sum))) return rc;
			for (size_t k = 0; k < nf; k++)
				if (status[k]) h_status[frame_of[k]] = CCT_E_STREAM;
			if (!images_on_device && (rc = good_rasters_to_host(images, d_img, N * px_bytes, h_status, c0, c1, st))) return rc;
		}
		c0 = c1;
	}
	set_last_kernel_ms(false, ms_sum);
	for (int i = 0; i < n; i++)
		if (h_status[i] != CCT_OK) return fail((int)h_status[i], "frame %d: %s", i, refusal((int)h_status[i]));
	return CCT_OK;
}

}  // extern "C"
