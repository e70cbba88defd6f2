// Strip-organised grayscale TIFF behind the C ABI: host side of tiff_kernels.hip.  Encode takes the encode slot (g_mu, the
// main stream; Deflate strips go through its DEFLATE pass, deflate_on_main), the reader a decode slot (lease_decode_slot;
// Deflate strips through launch_inflate on the slot's stream); passes, copies and timing are the scaffold of host.h.  The
// workspaces are this file's own.  The host parses every IFD and refuses what the reader does not take before anything is
// uploaded; what reaches the device is a list of strips whose coded bytes lie inside the uploaded files.
// tests/tiff_model.py restates the layout, the parser and its refusals.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "cct_internal.h"
#include "deflate_workspace.h"
#include "host.h"

using namespace cct;

namespace {

constexpr size_t TIFF_PASS_BYTES = (size_t)512 << 20;  // strip bytes (encode) / file and raster bytes (read) on the device at a time
constexpr size_t TIFF_IFD_MAX = 2 + 12 * 10 + 4;       // ten tags

enum { E_IMG, E_STRIPS, E_SSIZES, E_CODED, E_CSIZES, E_SOFF, E_OUT, E_FSIZES, E_NBUF };
enum { D_FILES, D_STRIPS, D_DECODED, D_LZW_STATUS, D_Z, D_ZOFFS, D_ZSIZES, D_ZSTATUS, D_IMG, D_NBUF };
Workspace<E_NBUF> g_enc_ws;             // under g_mu
Workspace<D_NBUF> g_dec_ws[DEC_SLOTS];  // under the slot's lock

int check_shape(int n, int rows, int cols, int bits)
{
	if (bits != 8 && bits != 16) return fail(CCT_E_ARG, "TIFF: %d bits per sample: 8 or 16", bits);
	if (rows < 1 || cols < 1 || rows > 65535 || cols > 65535)
		return fail(CCT_E_ARG, "TIFF shape %d x %d: rows and cols are 1 .. 65535", rows, cols);
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	return CCT_OK;
}

// Pillow's rule (TiffImagePlugin: STRIP_SIZE = 65536) unless the caller names a height
uint32_t strip_rows(int rows, int cols, int bits, int rows_per_strip)
{
	const size_t row_bytes = (size_t)cols * (bits / 8);
	const size_t rps = rows_per_strip > 0 ? (size_t)rows_per_strip : std::max<size_t>(1, 65536 / row_bytes);
	return (uint32_t)std::min<size_t>((size_t)rows, rps);
}

size_t coded_bound(size_t strip_bytes, int compression)
{
	if (compression == 5) return tiff_lzw_bound(strip_bytes);
	if (compression == 8) return deflate_out_stride(deflate_in_stride(strip_bytes), 8) - 13;
	return strip_bytes;
}

// ---- the parser --------------------------------------------------------------------------------------------------------

struct TiffDesc {
	uint32_t rows = 0, cols = 0, bits = 0, compression = 1, predictor = 1, rps = 0;
	bool big = false;
	std::vector<uint32_t> offs, counts;
};

struct Reader {
	const uint8_t *f; size_t len; bool big;
	uint32_t u16(size_t o) const { return big ? (uint32_t)f[o] << 8 | f[o + 1] : (uint32_t)f[o + 1] << 8 | f[o]; }
	uint32_t u32(size_t o) const { return big ? u16(o) << 16 | u16(o + 2) : u16(o + 2) << 16 | u16(o); }
};

// the values of a SHORT or LONG entry at `e`; false for another type, or an array that leaves the file
bool entry_values(const Reader &r, size_t e, std::vector<uint32_t> &v)
{
	const uint32_t type = r.u16(e + 2), count = r.u32(e + 4);
	if (type != 3 && type != 4) return false;
	const size_t size = type == 3 ? 2 : 4;
	if (count == 0 || count > 0x10000000u) return false;
	size_t at = e + 8;
	if ((size_t)count * size > 4) {
		at = r.u32(e + 8);
		if (at > r.len || (size_t)count * size > r.len - at) return false;
	}
	v.resize(count);
	for (uint32_t k = 0; k < count; k++) v[k] = type == 3 ? r.u16(at + 2 * (size_t)k) : r.u32(at + 4 * (size_t)k);
	return true;
}

// CCT_OK or CCT_E_TIFF: what the reader takes is listed in include/compact_hip.h
int parse_tiff(const uint8_t *f, size_t len, TiffDesc &d)
{
	if (len < 8 || len > 0xFFFFFFFFull) return CCT_E_TIFF;
	Reader r{f, len, false};
	if (f[0] == 'I' && f[1] == 'I') r.big = false;
	else if (f[0] == 'M' && f[1] == 'M') r.big = true;
	else return CCT_E_TIFF;
	if (r.u16(2) != 42) return CCT_E_TIFF;  // 43: BigTIFF
	const size_t ifd = r.u32(4);
	if (ifd < 8 || ifd > len || len - ifd < 2) return CCT_E_TIFF;
	const size_t ntags = r.u16(ifd);
	if (ntags == 0 || 12 * ntags > len - ifd - 2) return CCT_E_TIFF;
	d = TiffDesc();
	d.big = r.big;
	bool have[6] = {false, false, false, false, false, false};  // cols, rows, bits, photometric, offsets, counts
	uint32_t rps = 0xFFFFFFFFu;
	std::vector<uint32_t> v;
	for (size_t k = 0; k < ntags; k++) {
		const size_t e = ifd + 2 + 12 * k;
		const uint32_t tag = r.u16(e);
		switch (tag) {
		case 256: case 257: case 258: case 259: case 262: case 266: case 277: case 278: case 284: case 317: case 339:
			if (!entry_values(r, e, v) || v.size() != 1) return CCT_E_TIFF;
			break;
		case 273: case 279:
			if (!entry_values(r, e, v)) return CCT_E_TIFF;
			break;
		case 322: case 323: case 324: case 325: return CCT_E_TIFF;  // tiles
		default: continue;  // unknown tags are ignored
		}
		switch (tag) {
		case 256: d.cols = v[0]; have[0] = true; break;
		case 257: d.rows = v[0]; have[1] = true; break;
		case 258: d.bits = v[0]; have[2] = true; break;
		case 259: d.compression = v[0]; break;
		case 262: if (v[0] != 1) return CCT_E_TIFF; have[3] = true; break;
		case 266: if (v[0] != 1) return CCT_E_TIFF; break;
		case 277: if (v[0] != 1) return CCT_E_TIFF; break;
		case 278: rps = v[0]; break;
		case 284: if (v[0] != 1) return CCT_E_TIFF; break;
		case 317: d.predictor = v[0]; break;
		case 339: if (v[0] != 1) return CCT_E_TIFF; break;
		case 273: d.offs = v; have[4] = true; break;
		case 279: d.counts = v; have[5] = true; break;
		}
	}
	for (bool h : have) if (!h) return CCT_E_TIFF;
	if (d.bits != 8 && d.bits != 16) return CCT_E_TIFF;
	if (d.rows < 1 || d.cols < 1 || d.rows > 65535 || d.cols > 65535) return CCT_E_TIFF;
	if (d.compression == 32946) d.compression = 8;
	if (d.compression != 1 && d.compression != 5 && d.compression != 8) return CCT_E_TIFF;
	if (d.predictor != 1 && !(d.predictor == 2 && d.compression != 1)) return CCT_E_TIFF;
	if (rps == 0) return CCT_E_TIFF;
	d.rps = std::min(rps, d.rows);
	const size_t nstrips = (d.rows + d.rps - 1) / d.rps;
	if (d.offs.size() != nstrips || d.counts.size() != nstrips) return CCT_E_TIFF;
	for (size_t s = 0; s < nstrips; s++)
		if (d.offs[s] > len || d.counts[s] > len - d.offs[s]) return CCT_E_TIFF;  // a strip outside the file
	return CCT_OK;
}

}  // namespace

void cct::tiff_release()
{
	g_enc_ws.release();
	for (auto &w : g_dec_ws) w.release();
}

extern "C" {

size_t cct_tiff_bound(int rows, int cols, int bits, int compression, int rows_per_strip)
{
	if ((bits != 8 && bits != 16) || rows < 1 || cols < 1 || rows > 65535 || cols > 65535 || rows_per_strip < 0) return 0;
	if (compression != 1 && compression != 5 && compression != 8) return 0;
	const uint32_t rps = strip_rows(rows, cols, bits, rows_per_strip);
	const size_t spf = ((size_t)rows + rps - 1) / rps, strip_bytes = (size_t)rps * cols * (bits / 8);
	const size_t b = 8 + spf * coded_bound(strip_bytes, compression) + 1 + TIFF_IFD_MAX + 8 * spf;
	return b < ((size_t)1 << 32) ? b : 0;
}

int cct_tiff_encode_batch(const void *images, int images_on_device, int n, int rows, int cols, int bits, int compression, int predictor,
                          int rows_per_strip, int level, uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes)
{
	int rc = check_shape(n, rows, cols, bits);
	if (rc) return rc;
	if (compression != 1 && compression != 5 && compression != 8)
		return fail(CCT_E_ARG, "TIFF compression %d: 1 (none), 5 (LZW) or 8 (Deflate)", compression);
	if (predictor != 1 && predictor != 2) return fail(CCT_E_ARG, "TIFF predictor %d: 1 or 2", predictor);
	if (predictor == 2 && compression == 1) return fail(CCT_E_ARG, "TIFF predictor 2 goes with LZW or Deflate, not with uncompressed strips");
	if (rows_per_strip < 0) return fail(CCT_E_ARG, "TIFF rows_per_strip %d: 0 (the 64 KiB rule) or a height from 1 up", rows_per_strip);
	if (compression == 8) {
		if (level == -1) level = 6;
		if (level >= 0 && level <= 3) return fail(CCT_E_ARG, "TIFF Deflate level %d: deflate_stored / deflate_fast: not on the device", level);
		if (level < 4 || level > 9) return fail(CCT_E_ARG, "TIFF Deflate level %d: levels are -1 and 4 .. 9", level);
	}
	const size_t bound = cct_tiff_bound(rows, cols, bits, compression, rows_per_strip);
	if (!bound) return fail(CCT_E_ARG, "TIFF shape %d x %d: the file could pass 4 GiB", rows, cols);
	if (out_stride < bound) return fail(CCT_E_CAP, "out_stride %zu too small (need cct_tiff_bound = %zu)", out_stride, bound);
	if (n > 0 && (!images || !h_out || !h_out_sizes)) return fail(CCT_E_ARG, "null argument");
	if (n == 0) return CCT_OK;
	std::lock_guard<std::mutex> lk(g_mu);
	ApiCall in_call;
	if ((rc = ensure_ctx())) return rc;
	hipStream_t st = main_stream();
	DevBuf *W = g_enc_ws.buf;
	EventPair &ev = g_enc_ws.ev;
	const int bps = bits / 8;
	const uint32_t rps = strip_rows(rows, cols, bits, rows_per_strip);
	const size_t spf = ((size_t)rows + rps - 1) / rps, strip_bytes = (size_t)rps * cols * bps, img_bytes = (size_t)rows * cols * bps;
	const size_t strip_stride = deflate_in_stride(strip_bytes), lzw_stride = tiff_lzw_bound(strip_bytes);
	const size_t zstride = deflate_out_stride(strip_stride, 8), fstride = (bound + 3) & ~(size_t)3;
	const size_t per_file = spf * std::max(strip_stride, compression == 5 ? lzw_stride : (size_t)0) + fstride;
	const int per_pass = (int)std::max<size_t>(1, std::min<size_t>(TIFF_PASS_BYTES / per_file, 0x7FFFFFFFull / spf));
	float ms_sum = 0;
	StreamDrain drain(st);  // copies into caller memory land before any return
	for (int c0 = 0; c0 < n; c0 += per_pass) {
		const int nc = std::min(per_pass, n - c0);
		const size_t nstrips = (size_t)nc * spf;
		const void *d_img;
		if ((rc = rasters_to_device(images, images_on_device, c0, nc, img_bytes, W[E_IMG], st, &d_img))) return rc;
		if ((rc = W[E_STRIPS].ensure(nstrips * strip_stride))) return rc;
		if ((rc = W[E_SSIZES].ensure(nstrips * 4))) return rc;
		if ((rc = W[E_SOFF].ensure(nstrips * 4))) return rc;
		if ((rc = W[E_OUT].ensure((size_t)nc * fstride))) return rc;
		if ((rc = W[E_FSIZES].ensure((size_t)nc * 4))) return rc;
		if (compression == 5) {
			if ((rc = W[E_CODED].ensure(nstrips * lzw_stride))) return rc;
			if ((rc = W[E_CSIZES].ensure(nstrips * 4))) return rc;
		}
		if ((rc = ev.begin(st))) return rc;
		if (compression == 8) HIP_TRY(hipMemsetAsync(W[E_STRIPS].p, 0, nstrips * strip_stride, st));  // the DEFLATE pass reads the padding
		HIP_TRY(launch_tiff_stage(d_img, nc, rows, cols, bps, predictor, (int)rps, (int)spf, (uint8_t *)W[E_STRIPS].p, strip_stride,
		                          (uint32_t *)W[E_SSIZES].p, st));
		TiffPackArgs pk{};
		pk.src = (const uint8_t *)W[E_STRIPS].p; pk.src_stride = strip_stride; pk.src_skip = 0; pk.src_sizes = (const uint32_t *)W[E_SSIZES].p;
		if (compression == 5) {
			HIP_TRY(launch_tiff_lzw_encode((const uint8_t *)W[E_STRIPS].p, strip_stride, (const uint32_t *)W[E_SSIZES].p, (int)nstrips,
			                               (uint8_t *)W[E_CODED].p, lzw_stride, (uint32_t *)W[E_CSIZES].p, st));
			pk.src = (const uint8_t *)W[E_CODED].p; pk.src_stride = lzw_stride; pk.src_sizes = (const uint32_t *)W[E_CSIZES].p;
		} else if (compression == 8) {
			if ((rc = deflate_on_main((const uint8_t *)W[E_STRIPS].p, strip_stride, (const uint32_t *)W[E_SSIZES].p, (int)nstrips, zstride, level,
			                          &pk.src, &pk.src_sizes)))
				return rc;
			pk.src_stride = zstride; pk.src_skip = 13;
		}
		pk.spf = (uint32_t)spf; pk.rows = (uint32_t)rows; pk.cols = (uint32_t)cols; pk.bits = (uint32_t)bits;
		pk.compression = (uint32_t)compression; pk.predictor = (uint32_t)predictor; pk.rps = rps;
		pk.strip_off = (uint32_t *)W[E_SOFF].p;
		pk.out = (uint8_t *)W[E_OUT].p; pk.out_stride = fstride; pk.out_sizes = (uint32_t *)W[E_FSIZES].p;
		HIP_TRY(launch_tiff_pack(pk, nc, st));
		if ((rc = ev.end(st))) return rc;
		HIP_TRY(hipMemcpyAsync(h_out_sizes + c0, W[E_FSIZES].p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		if ((rc = ev.add_ms(ms_sum))) return rc;
		if ((rc = files_to_host(h_out + (size_t)c0 * out_stride, out_stride, h_out_sizes + c0, nc, W[E_OUT].p, fstride, 0, bound, "file", c0, "bound", st)))
			return rc;
	}
	set_last_kernel_ms(true, ms_sum);
	return CCT_OK;
}

int cct_tiff_info(const uint8_t *h_file, size_t len, int *rows, int *cols, int *bits)
{
	if (!h_file || !rows || !cols || !bits) return fail(CCT_E_ARG, "null argument");
	TiffDesc d;
	if (parse_tiff(h_file, len, d)) return fail(CCT_E_TIFF, "not a TIFF file cct_tiff_read_batch takes");
	*rows = (int)d.rows; *cols = (int)d.cols; *bits = (int)d.bits;
	return CCT_OK;
}

int cct_tiff_read_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int rows, int cols, int bits, void *images,
                        int images_on_device, size_t images_cap_px, uint32_t *h_status)
{
	int rc = check_shape(n, rows, cols, bits);
	if (rc) return rc;
	const size_t N = (size_t)rows * cols;
	if (images_cap_px / N < (size_t)n) return fail(CCT_E_CAP, "output holds %zu pixels, need %zu", images_cap_px, (size_t)n * N);
	if (n > 0 && (!h_files || !h_offsets || !images || !h_status)) return fail(CCT_E_ARG, "null argument");
	if ((rc = check_offsets(h_offsets, n, "file"))) return rc;
	if (n == 0) return CCT_OK;
	// every IFD is read before the device is touched
	std::vector<TiffDesc> desc(n);
	const int bps = bits / 8;
	const size_t row_bytes = (size_t)cols * bps, img_bytes = N * bps;
	for (int i = 0; i < n; i++) {
		TiffDesc &d = desc[i];
		h_status[i] = (uint32_t)parse_tiff(h_files + h_offsets[i], (size_t)(h_offsets[i + 1] - h_offsets[i]), d);
		if (h_status[i] == CCT_OK && (d.rows != (uint32_t)rows || d.cols != (uint32_t)cols || d.bits != (uint32_t)bits)) h_status[i] = CCT_E_TIFF;
		if (h_status[i] != CCT_OK) continue;
		for (size_t s = 0; s < d.offs.size(); s++) {
			const size_t want = (size_t)std::min(d.rps, d.rows - (uint32_t)s * d.rps) * row_bytes;
			// an uncompressed strip is its rows; a coded strip of no bytes yields none
			if (d.compression == 1 ? d.counts[s] < want : d.counts[s] == 0) h_status[i] = CCT_E_STREAM;
		}
	}
	DecLease L;
	if ((rc = lease_decode_slot(L))) return rc;
	hipStream_t st = L.stream;
	DevBuf *W = g_dec_ws[L.slot].buf;
	EventPair &ev = g_dec_ws[L.slot].ev;
	float ms_sum = 0;
	std::vector<TiffStrip> strips;      // LZW strips first, then Deflate, then uncompressed ones
	std::vector<TiffStrip> part[3];
	std::vector<uint64_t> zoffs;
	std::vector<uint32_t> lzw_status, zstatus, zsizes;
	StreamDrain drain(st);  // declared after the vectors the copies land in
	for (int c0 = 0; c0 < n;) {
		int c1 = c0 + 1;
		while (c1 < n && h_offsets[c1 + 1] - h_offsets[c0] <= TIFF_PASS_BYTES && (size_t)(c1 + 1 - c0) * img_bytes <= TIFF_PASS_BYTES) c1++;
		const uint64_t a0 = h_offsets[c0], a1 = h_offsets[c1];
		for (auto &p : part) p.clear();
		size_t lzw_bytes = 0, zwant_max = 0;
		for (int i = c0; i < c1; i++) {
			if (h_status[i] != CCT_OK) continue;
			const TiffDesc &d = desc[i];
			for (size_t s = 0; s < d.offs.size(); s++) {
				TiffStrip t{};
				t.src = h_offsets[i] - a0 + d.offs[s];
				t.len = d.counts[s];
				t.file = (uint32_t)(i - c0);
				t.row0 = (uint32_t)s * d.rps;
				t.nrows = std::min(d.rps, d.rows - t.row0);
				t.want = (uint32_t)(t.nrows * row_bytes);
				t.flags = (d.big ? TIFF_F_BIG_ENDIAN : 0) | (d.predictor == 2 ? TIFF_F_PREDICTOR : 0) | (d.compression == 1 ? TIFF_F_FROM_FILE : 0);
				if (d.compression == 5) { t.dst = lzw_bytes; lzw_bytes += (t.want + 3) & ~(size_t)3; }
				if (d.compression == 8) zwant_max = std::max<size_t>(zwant_max, t.want);
				part[d.compression == 5 ? 0 : d.compression == 8 ? 1 : 2].push_back(t);
			}
		}
		lzw_bytes = (lzw_bytes + 255) & ~(size_t)255;  // the INFLATE kernel's output starts aligned
		const size_t nl = part[0].size(), nz = part[1].size();
		const size_t zout_stride = (zwant_max + 15) & ~(size_t)15;
		zoffs.assign(nz + 1, 0);
		for (size_t k = 0; k < nz; k++) {
			part[1][k].dst = lzw_bytes + k * zout_stride;
			zoffs[k + 1] = zoffs[k] + part[1][k].len;
		}
		strips.clear();
		for (auto &p : part) strips.insert(strips.end(), p.begin(), p.end());
		if (!strips.empty()) {
			const size_t abytes = (size_t)(a1 - a0), ns = strips.size();
			const size_t zbytes = (size_t)zoffs[nz], zpad = (zbytes + 31) & ~(size_t)15;
			uint8_t *d_img = images_on_device ? (uint8_t *)images + (size_t)c0 * img_bytes : nullptr;
			if (!images_on_device) {
				if ((rc = W[D_IMG].ensure((size_t)(c1 - c0) * img_bytes))) return rc;
				d_img = (uint8_t *)W[D_IMG].p;
			}
			if ((rc = W[D_FILES].ensure(abytes + 16))) return rc;
			if ((rc = W[D_STRIPS].ensure(ns * sizeof(TiffStrip)))) return rc;
			if ((rc = W[D_DECODED].ensure(lzw_bytes + nz * zout_stride + 16))) return rc;
			if ((rc = W[D_LZW_STATUS].ensure(nl * 4 + 4))) return rc;
			if (nz) {
				if ((rc = W[D_Z].ensure(zpad + 16))) return rc;
				if ((rc = W[D_ZOFFS].ensure((nz + 1) * 8))) return rc;
				if ((rc = W[D_ZSIZES].ensure(nz * 4))) return rc;
				if ((rc = W[D_ZSTATUS].ensure(nz * 4))) return rc;
			}
			HIP_TRY(hipMemcpyAsync(W[D_FILES].p, h_files + a0, abytes, hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(W[D_STRIPS].p, strips.data(), ns * sizeof(TiffStrip), hipMemcpyHostToDevice, st));
			const TiffStrip *d_strips = (const TiffStrip *)W[D_STRIPS].p;
			if (nz) {
				HIP_TRY(hipMemcpyAsync(W[D_ZOFFS].p, zoffs.data(), (nz + 1) * 8, hipMemcpyHostToDevice, st));
				HIP_TRY(hipMemsetAsync(W[D_Z].p, 0, zpad + 16, st));  // the INFLATE kernel reads ahead of a stream's end
			}
			if ((rc = ev.begin(st))) return rc;
			if (nl)
				HIP_TRY(launch_tiff_lzw_decode((const uint8_t *)W[D_FILES].p, d_strips, (uint32_t)nl, (uint8_t *)W[D_DECODED].p,
				                               (uint32_t *)W[D_LZW_STATUS].p, st));
			if (nz) {
				HIP_TRY(launch_tiff_gather((const uint8_t *)W[D_FILES].p, d_strips + nl, (uint32_t)nz, (const uint64_t *)W[D_ZOFFS].p,
				                           (uint8_t *)W[D_Z].p, st));
				InflateArgs ia{};
				ia.in = (const uint8_t *)W[D_Z].p; ia.in_total = zpad;
				ia.offsets = (const uint64_t *)W[D_ZOFFS].p; ia.skip = 0;
				ia.out = (uint8_t *)W[D_DECODED].p + lzw_bytes; ia.out_stride = zout_stride;
				ia.out_sizes = (uint32_t *)W[D_ZSIZES].p; ia.status = (uint32_t *)W[D_ZSTATUS].p;
				HIP_TRY(launch_inflate(ia, (int)nz, st, inflate_lanes_for_call()));
			}
			HIP_TRY(launch_tiff_unpredict((const uint8_t *)W[D_FILES].p, (const uint8_t *)W[D_DECODED].p, d_strips, (uint32_t)ns, rows, cols, bps,
			                              d_img, st));
			if ((rc = ev.end(st))) return rc;
			lzw_status.assign(nl, 0); zstatus.assign(nz, 0); zsizes.assign(nz, 0);
			if (nl) HIP_TRY(hipMemcpyAsync(lzw_status.data(), W[D_LZW_STATUS].p, nl * 4, hipMemcpyDeviceToHost, st));
			if (nz) {
				HIP_TRY(hipMemcpyAsync(zstatus.data(), W[D_ZSTATUS].p, nz * 4, hipMemcpyDeviceToHost, st));
				HIP_TRY(hipMemcpyAsync(zsizes.data(), W[D_ZSIZES].p, nz * 4, hipMemcpyDeviceToHost, st));
			}
			HIP_TRY(hipStreamSynchronize(st));
			if ((rc = ev.add_ms(ms_sum))) return rc;
			for (size_t k = 0; k < nl; k++)
				if (lzw_status[k]) h_status[c0 + strips[k].file] = CCT_E_STREAM;
			for (size_t k = 0; k < nz; k++) {
				uint32_t &fs = h_status[c0 + strips[nl + k].file];
				if (fs != CCT_OK) continue;  // the file's first bad strip names the code
				if (zstatus[k] & CCT_ST_ZLIB) fs = CCT_E_ZLIB;
				else if ((zstatus[k] & CCT_ST_STREAM) || zsizes[k] != strips[nl + k].want) fs = CCT_E_STREAM;
			}
			if (!images_on_device && (rc = good_rasters_to_host(images, d_img, img_bytes, h_status, c0, c1, st))) return rc;
		}
		c0 = c1;
	}
	set_last_kernel_ms(false, ms_sum);
	for (int i = 0; i < n; i++)
		if (h_status[i] != CCT_OK)
			return fail((int)h_status[i], "file %d: %s", i,
			            h_status[i] == CCT_E_TIFF ? "not a TIFF file of this shape that the reader takes" : "a strip that does not decode to its rows");
	return CCT_OK;
}

}  // extern "C"
