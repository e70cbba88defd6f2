// JPEG Lossless (SOF3) frames behind the C ABI: host side of jpeg_lossless_kernels.hip.  Encode takes the encode slot (g_mu,
// the main stream), decode a decode slot (lease_decode_slot); passes, copies and timing are the scaffold of host.h.  The
// workspaces are this file's own, one for the encode slot and one per decode slot.  The host walks the markers of every file
// and decides every structural refusal before anything is uploaded; the device sees the entropy-coded segment, the decoding
// table and the scan parameters.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "cct_internal.h"
#include "host.h"

using namespace cct;

namespace {

constexpr size_t JPL_MAX_PIXELS = (size_t)1 << 26;
constexpr size_t JPL_PASS_BYTES = (size_t)512 << 20;  // device bytes of the frames of one pass (one frame at least)

enum { E_IMG, E_HIST, E_CODES, E_BITBUF, E_INTS, E_OUT, E_SIZES, E_NBUF };
enum { D_FILES, D_FRAMES, D_INT_FRAME, D_UBUF, D_ISTART, D_SUB, D_DIFF, D_STATUS, D_IMG, D_NBUF };
Workspace<E_NBUF> g_enc_ws;             // under g_mu
Workspace<D_NBUF> g_dec_ws[DEC_SLOTS];  // under the slot's lock

bool shape_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && rows <= 65535 && cols <= 65535 && (size_t)rows * (size_t)cols <= JPL_MAX_PIXELS; }

int check_shape(int n, int rows, int cols)
{
	if (!shape_ok(rows, cols))
		return fail(CCT_E_ARG, "JPEG Lossless shape %d x %d: rows and cols 1 .. 65535, at most %zu pixels", rows, cols, JPL_MAX_PIXELS);
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	return CCT_OK;
}

uint32_t be16(const uint8_t *p) { return (uint32_t)p[0] << 8 | (uint32_t)p[1]; }

struct Table { uint8_t bits[16]; uint8_t vals[17]; int nval; bool defined = false; };
struct Parsed {
	int P = 0, Y = 0, X = 0, ri = 0, ss = 0, pt = 0;
	Table table;
	size_t s0 = 0, s1 = 0;  // the entropy-coded segment: [s0, s1), f[s1] is the 0xFF of EOI
};

// The marker walk (tests/jpeg_lossless_model.py parse()): CCT_OK or CCT_E_JPEG.  Every read is checked against len first.
int parse_file(const uint8_t *f, size_t len, Parsed &o)
{
	if (len < 4 || f[0] != 0xFF || f[1] != 0xD8) return CCT_E_JPEG;
	size_t pos = 2;
	bool sof = false;
	int comp_id = 0;
	Table tables[4];
	for (;;) {
		if (pos + 4 > len || f[pos] != 0xFF) return CCT_E_JPEG;
		const int m = f[pos + 1];
		if (m == 0xD8 || m == 0xD9 || m == 0x01 || m == 0xFF || m == 0x00 || (m >= 0xD0 && m <= 0xD7)) return CCT_E_JPEG;
		const size_t ln = be16(f + pos + 2);
		if (ln < 2 || pos + 2 + ln > len) return CCT_E_JPEG;
		const uint8_t *seg = f + pos + 4;
		size_t sl = ln - 2;
		pos += 2 + ln;
		if (m == 0xC3) {
			if (sof || sl < 6 || sl != 6 + 3 * (size_t)seg[5]) return CCT_E_JPEG;
			o.P = seg[0]; o.Y = (int)be16(seg + 1); o.X = (int)be16(seg + 3);
			if (seg[5] != 1 || o.Y == 0 || o.X == 0 || o.P < 2 || o.P > 16) return CCT_E_JPEG;
			comp_id = seg[6];
			sof = true;
		} else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
			return CCT_E_JPEG;  // another SOF type
		} else if (m == 0xC4) {
			while (sl) {
				if (sl < 17) return CCT_E_JPEG;
				size_t cnt = 0;
				uint32_t kraft = 0;
				for (int l = 1; l <= 16; l++) { cnt += seg[l]; kraft += (uint32_t)seg[l] << (16 - l); }
				if (sl < 17 + cnt) return CCT_E_JPEG;
				if (seg[0] > 3 || cnt > 17 || kraft > 65536u) return CCT_E_JPEG;  // class 0, ids 0 .. 3; 17 symbols at most
				Table &t = tables[seg[0]];
				memcpy(t.bits, seg + 1, 16);
				for (size_t k = 0; k < cnt; k++) { if (seg[17 + k] > 16) return CCT_E_JPEG; t.vals[k] = seg[17 + k]; }
				t.nval = (int)cnt;
				t.defined = true;
				seg += 17 + cnt; sl -= 17 + cnt;
			}
		} else if (m == 0xDD) {
			if (sl != 2) return CCT_E_JPEG;
			o.ri = (int)be16(seg);
		} else if (m == 0xDC) {
			return CCT_E_JPEG;  // DNL
		} else if (m == 0xDA) {
			if (!sof || sl != 6 || seg[0] != 1 || seg[1] != comp_id) return CCT_E_JPEG;
			const int td = seg[2] >> 4;
			o.ss = seg[3]; o.pt = seg[5] & 15;
			if (o.ss < 1 || o.ss > 7 || seg[4] != 0 || (seg[5] >> 4) != 0 || o.pt >= o.P || td > 3 || !tables[td].defined) return CCT_E_JPEG;
			o.table = tables[td];
			break;
		}  // APPn, COM and whatever else carries a length: skipped
	}
	if (o.ri % o.X) return CCT_E_JPEG;  // a DRI that is not whole rows
	o.s0 = pos;
	for (size_t i = pos;;) {
		const uint8_t *q = i < len ? (const uint8_t *)memchr(f + i, 0xFF, len - i) : nullptr;
		if (!q || (size_t)(q - f) + 1 >= len) return CCT_E_JPEG;  // no EOI
		const size_t j = (size_t)(q - f);
		const int nx = f[j + 1];
		if (nx == 0 || (nx >= 0xD0 && nx <= 0xD7)) i = j + 2;
		else if (nx == 0xFF) i = j + 1;
		else if (nx == 0xD9) { o.s1 = j; break; }
		else return CCT_E_JPEG;  // DNL, a second scan, anything but EOI
	}
	return CCT_OK;
}

const char *refusal(int code)
{
	return code == CCT_E_JPEG    ? "not a JPEG this reader takes"
	       : code == CCT_E_MIXED ? "the frame's shape or precision is not the call's"
	                             : "entropy-coded data: a code outside the table, data that ends early or is left over, or a wrong RST";
}

}  // namespace

void cct::jpegll_release()
{
	g_enc_ws.release();
	for (auto &w : g_dec_ws) w.release();
}

extern "C" {

// A sample costs 31 bits at most: a code of up to 16 bits and up to 15 extra bits (category 16 has none).  An interval of s
// samples is padded to ceil(31 s / 8) bytes at most, byte stuffing doubles that when every byte is 0xFF, and every interval
// but the first is led by a two-byte RST; the headers and EOI take JPL_HDR_MAX at most.
size_t cct_jpegll_bound(int rows, int cols, int restart_rows)
{
	if (!shape_ok(rows, cols) || restart_rows < 0 || (restart_rows > 0 && (size_t)restart_rows * (size_t)cols > 65535)) return 0;
	const size_t rpi = restart_rows ? (size_t)restart_rows : (size_t)rows, n_int = ((size_t)rows + rpi - 1) / rpi;
	const size_t isz = std::min(rpi, (size_t)rows) * (size_t)cols;
	return JPL_HDR_MAX + n_int * (2 * ((31 * isz + 7) / 8) + 2);
}

int cct_jpegll_info(const uint8_t *h_file, size_t len, int *rows, int *cols, int *precision)
{
	if (!h_file || !rows || !cols || !precision) return fail(CCT_E_ARG, "null argument");
	Parsed p;
	const int rc = parse_file(h_file, len, p);
	if (rc) return fail(rc, "%s", refusal(rc));
	*rows = p.Y; *cols = p.X; *precision = p.P;
	return CCT_OK;
}

int cct_jpegll_encode_batch(const void *images, int images_on_device, int n, int rows, int cols, int src_bits, int precision, int restart_rows,
                            uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes, uint32_t *h_status)
{
	return cct_jpegll_encode_batch_sv(images, images_on_device, n, rows, cols, src_bits, precision, 1, restart_rows, h_out, out_stride, h_out_sizes,
	                                  h_status, nullptr);
}

int cct_jpegll_encode_batch_sv(const void *images, int images_on_device, int n, int rows, int cols, int src_bits, int precision, int predictor,
                               int restart_rows, uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes, uint32_t *h_status,
                               uint32_t *h_predictors)
{
	if (predictor < 0 || predictor > 7) return fail(CCT_E_ARG, "JPEG Lossless: predictor %d: 1 .. 7, or 0 for the frame's best", predictor);
	int rc = check_shape(n, rows, cols);
	if (rc) return rc;
	if (src_bits != 8 && src_bits != 16) return fail(CCT_E_ARG, "JPEG Lossless: samples of %d bits: 8 or 16", src_bits);
	if (precision < 2 || precision > src_bits) return fail(CCT_E_ARG, "JPEG Lossless: precision %d: 2 .. %d", precision, src_bits);
	if (restart_rows < 0 || (restart_rows > 0 && (size_t)restart_rows * (size_t)cols > 65535))
		return fail(CCT_E_ARG, "JPEG Lossless: restart interval of %d rows: at most 65535 samples", restart_rows);
	const size_t bound = cct_jpegll_bound(rows, cols, restart_rows);
	if (out_stride < bound) return fail(CCT_E_CAP, "out_stride %zu too small (need cct_jpegll_bound = %zu)", out_stride, bound);
	if (n > 0 && (!images || !h_out || !h_out_sizes || !h_status)) return fail(CCT_E_ARG, "null argument");
	if (n == 0) return CCT_OK;
	std::lock_guard<std::mutex> lk(g_mu);
	ApiCall in_call;
	if ((rc = ensure_ctx())) return rc;
	hipStream_t st = main_stream();
	DevBuf *W = g_enc_ws.buf;
	EventPair &ev = g_enc_ws.ev;
	const size_t N = (size_t)rows * cols, img_bytes = N * (src_bits / 8), dstride = (bound + 3) & ~(size_t)3;
	const uint32_t rpi = restart_rows ? (uint32_t)restart_rows : (uint32_t)rows, n_int = ((uint32_t)rows + rpi - 1) / rpi;
	// predictor 0: seven histograms and seven tables a frame where a fixed predictor has one of each
	const uint32_t ncand = predictor ? 1u : JPL_NCAND;
	const size_t cand_bytes = predictor ? 0 : (size_t)(JPL_NCAND - 1) * (17 * 4 + sizeof(JplCode));
	const int per_pass = (int)std::max<size_t>(1, JPL_PASS_BYTES / (dstride + 4 * N + cand_bytes));
	float ms_sum = 0;
	std::vector<uint32_t> status, sel;
	StreamDrain drain(st);  // copies into caller memory land before any return
	for (int c0 = 0; c0 < n; c0 += per_pass) {
		const int nc = std::min(per_pass, n - c0);
		const void *d_img;
		if ((rc = rasters_to_device(images, images_on_device, c0, nc, img_bytes, W[E_IMG], st, &d_img))) return rc;
		const size_t hist_bytes = (size_t)nc * (17 * ncand + 2) * 4;  // 17 bins a candidate, the status word and the selection value of every frame
		if ((rc = W[E_HIST].ensure(hist_bytes))) return rc;
		if ((rc = W[E_CODES].ensure((size_t)nc * ncand * sizeof(JplCode)))) return rc;
		if ((rc = W[E_BITBUF].ensure((size_t)nc * N * 4))) return rc;
		if ((rc = W[E_INTS].ensure((size_t)nc * n_int * 3 * 4))) return rc;
		if ((rc = W[E_OUT].ensure((size_t)nc * dstride))) return rc;
		if ((rc = W[E_SIZES].ensure((size_t)nc * 4))) return rc;
		JplEncArgs a{};
		a.images = d_img; a.src_bits = (uint32_t)src_bits; a.n = (uint32_t)nc; a.rows = (uint32_t)rows; a.cols = (uint32_t)cols;
		a.precision = (uint32_t)precision; a.rpi = rpi; a.n_int = n_int; a.restart = restart_rows > 0;
		a.predictor = (uint32_t)predictor; a.ncand = ncand;
		a.hist = (uint32_t *)W[E_HIST].p; a.status = a.hist + (size_t)nc * 17 * ncand; a.sel = a.status + nc;
		a.codes = (JplCode *)W[E_CODES].p; a.bitbuf = (uint32_t *)W[E_BITBUF].p;
		a.ibytes = (uint32_t *)W[E_INTS].p; a.iff = a.ibytes + (size_t)nc * n_int; a.ioff = a.iff + (size_t)nc * n_int;
		a.out = (uint8_t *)W[E_OUT].p; a.out_stride = dstride; a.out_sizes = (uint32_t *)W[E_SIZES].p;
		if ((rc = ev.begin(st))) return rc;
		HIP_TRY(hipMemsetAsync(W[E_HIST].p, 0, hist_bytes, st));
		HIP_TRY(launch_jpl_encode(a, st));
		if ((rc = ev.end(st))) return rc;
		status.assign(nc, 0);
		HIP_TRY(hipMemcpyAsync(h_out_sizes + c0, W[E_SIZES].p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(status.data(), a.status, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
		if (h_predictors) {
			sel.assign(nc, 0);
			HIP_TRY(hipMemcpyAsync(sel.data(), a.sel, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
		}
		HIP_TRY(hipStreamSynchronize(st));
		if ((rc = ev.add_ms(ms_sum))) return rc;
		for (int i = 0; i < nc; i++) h_status[c0 + i] = status[i] ? CCT_E_OVERFLOW : CCT_OK;
		if (h_predictors) std::copy(sel.begin(), sel.end(), h_predictors + c0);
		if ((rc = files_to_host(h_out + (size_t)c0 * out_stride, out_stride, h_out_sizes + c0, nc, W[E_OUT].p, dstride, 0, bound, "frame", c0, "bound", st)))
			return rc;
	}
	set_last_kernel_ms(true, ms_sum);
	for (int i = 0; i < n; i++)
		if (h_status[i] != CCT_OK) return fail((int)h_status[i], "frame %d: a sample does not fit the precision of %d bits", i, precision);
	return CCT_OK;
}

int cct_jpegll_decode_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int rows, int cols, int bits, void *images,
                            int images_on_device, size_t images_cap_px, uint32_t *h_status)
{
	int rc = check_shape(n, rows, cols);
	if (rc) return rc;
	if (bits != 8 && bits != 16) return fail(CCT_E_ARG, "JPEG Lossless: %d bits allocated: 8 or 16", bits);
	const size_t N = (size_t)rows * cols, px_bytes = (size_t)bits / 8;
	if (images_cap_px / N < (size_t)n) return fail(CCT_E_CAP, "output holds %zu pixels, need %zu", images_cap_px, (size_t)n * N);
	if (n > 0 && (!h_files || !h_offsets || !images || !h_status)) return fail(CCT_E_ARG, "null argument");
	if ((rc = check_offsets(h_offsets, n, "file"))) return rc;
	if (n == 0) return CCT_OK;
	// the marker walk: every structural refusal is decided here, before the device is touched
	std::vector<Parsed> parsed(n);
	for (int i = 0; i < n; i++) {
		const size_t len = (size_t)(h_offsets[i + 1] - h_offsets[i]);
		int r = len > 0xFFFFFFFFull ? CCT_E_JPEG : parse_file(h_files + h_offsets[i], len, parsed[i]);
		if (r == CCT_OK && (parsed[i].Y != rows || parsed[i].X != cols || parsed[i].P > bits)) r = CCT_E_MIXED;
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
	std::vector<JplFrame> frames;
	std::vector<uint32_t> int_frame, status;
	std::vector<int> frame_of;
	StreamDrain drain(st);  // declared after the vectors the copies land in
	for (int c0 = 0; c0 < n;) {
		int c1 = c0 + 1;
		while (c1 < n && h_offsets[c1 + 1] - h_offsets[c0] <= JPL_PASS_BYTES / 4 && (size_t)(c1 + 1 - c0) * N * (2 + px_bytes) <= JPL_PASS_BYTES) c1++;
		const uint64_t a0 = h_offsets[c0], a1 = h_offsets[c1];
		frames.clear(); int_frame.clear(); frame_of.clear();
		uint64_t nsub = 0;
		bool any_generic = false;
		for (int i = c0; i < c1; i++) {
			if (h_status[i] != CCT_OK) continue;
			const Parsed &p = parsed[i];
			JplFrame f{};
			f.src = h_offsets[i] - a0 + p.s0;
			f.len = (uint32_t)(p.s1 - p.s0);
			f.slot = (uint32_t)(i - c0);
			f.ss = (uint32_t)p.ss; f.pt = (uint32_t)p.pt; f.init = 1u << (p.P - p.pt - 1);
			f.rpi = p.ri ? (uint32_t)(p.ri / cols) : (uint32_t)rows;
			f.n_int = ((uint32_t)rows + f.rpi - 1) / f.rpi;
			f.int0 = (uint32_t)int_frame.size();
			f.sub0 = (uint32_t)nsub;
			nsub += (uint64_t)f.len * 8 / JPL_SUB + f.n_int;
			int code = 0, k = 0;
			f.maxcode[0] = -1;
			for (int l = 1; l <= 16; l++) {
				const int b = p.table.bits[l - 1];
				f.delta[l] = k - code;
				code += b; k += b;
				f.maxcode[l] = b ? code - 1 : -1;
				code <<= 1;
			}
			memcpy(f.huffval, p.table.vals, (size_t)p.table.nval);
			any_generic |= p.ss != 1;
			int_frame.insert(int_frame.end(), f.n_int, (uint32_t)frames.size());
			frames.push_back(f); frame_of.push_back(i);
		}
		if (!frames.empty()) {
			if (nsub > 0x7FFFFFFFull || int_frame.size() > 0x7FFFFFFFull) return fail(CCT_E_ARG, "JPEG Lossless: too much coded data in one pass");
			const size_t abytes = (size_t)(a1 - a0), nf = frames.size(), ni = int_frame.size();
			uint8_t *d_img = images_on_device ? (uint8_t *)images + (size_t)c0 * N * px_bytes : nullptr;
			if (!images_on_device) {
				if ((rc = W[D_IMG].ensure((size_t)(c1 - c0) * N * px_bytes))) return rc;
				d_img = (uint8_t *)W[D_IMG].p;
			}
			if ((rc = W[D_FILES].ensure(abytes + 16))) return rc;
			if ((rc = W[D_UBUF].ensure(abytes + 16))) return rc;
			if ((rc = W[D_FRAMES].ensure(nf * sizeof(JplFrame)))) return rc;
			if ((rc = W[D_INT_FRAME].ensure(ni * 4))) return rc;
			if ((rc = W[D_ISTART].ensure((ni + nf) * 4))) return rc;
			if ((rc = W[D_SUB].ensure((size_t)nsub * 3 * 4 + 16))) return rc;
			if ((rc = W[D_DIFF].ensure((size_t)(c1 - c0) * N * 2))) return rc;
			if ((rc = W[D_STATUS].ensure(nf * 4))) return rc;
			HIP_TRY(hipMemcpyAsync(W[D_FILES].p, h_files + a0, abytes, hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(W[D_FRAMES].p, frames.data(), nf * sizeof(JplFrame), hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(W[D_INT_FRAME].p, int_frame.data(), ni * 4, hipMemcpyHostToDevice, st));
			JplDecArgs a{};
			a.files = (const uint8_t *)W[D_FILES].p; a.frames = (const JplFrame *)W[D_FRAMES].p; a.nframes = (uint32_t)nf;
			a.int_frame = (const uint32_t *)W[D_INT_FRAME].p; a.total_int = (uint32_t)ni;
			a.rows = (uint32_t)rows; a.cols = (uint32_t)cols; a.out_bits = (uint32_t)bits;
			a.ubuf = (uint8_t *)W[D_UBUF].p; a.istart = (uint32_t *)W[D_ISTART].p;
			a.sub_start = (uint32_t *)W[D_SUB].p; a.sub_land = a.sub_start + nsub; a.sub_cnt = a.sub_land + nsub;
			a.diff = (uint16_t *)W[D_DIFF].p; a.status = (uint32_t *)W[D_STATUS].p; a.images = d_img; a.any_generic = any_generic;
			if ((rc = ev.begin(st))) return rc;
			HIP_TRY(hipMemsetAsync(W[D_STATUS].p, 0, nf * 4, st));
			HIP_TRY(launch_jpl_decode(a, st));
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
