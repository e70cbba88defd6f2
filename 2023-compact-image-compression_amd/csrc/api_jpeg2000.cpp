// JPEG 2000 Part-1 lossless files behind the C ABI: host side of jpeg2000_kernels.hip.  Encode takes the encode slot (g_mu,
// the main stream); passes, copies and timing are the scaffold of host.h, the workspace is this file's own.  The host lays
// the subbands and code-blocks out once per call (j2k_layout) and builds the headers, which are the same for every frame
// but for two lengths the device patches; cct_j2k_info walks the boxes and reads SIZ on the host.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "cct_internal.h"
#include "host.h"

using namespace cct;

namespace {

constexpr size_t J2K_MAX_PIXELS = (size_t)1 << 26;    // the cap of the JPEG Lossless codec
constexpr size_t J2K_PASS_BYTES = (size_t)512 << 20;  // device bytes of the frames of one pass (one frame at least)

constexpr size_t J2K_DEC_PASS_BYTES = (size_t)512 << 20;  // likewise for the files of one decode pass

enum { E_IMG, E_PLANE_A, E_PLANE_B, E_LAYOUT, E_SLABS, E_CBOUT, E_TT, E_OUT, E_SIZES, E_NBUF };
enum { D_FILES, D_SEGS, D_FLIST, D_LAYOUT, D_CBS, D_TT, D_CHUNKS, D_STATUS, D_PLANE_A, D_PLANE_B, D_IMG, D_NBUF };
Workspace<E_NBUF> g_enc_ws;             // under g_mu
Workspace<D_NBUF> g_dec_ws[DEC_SLOTS];  // under the slot's lock

bool shape_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && rows <= 65535 && cols <= 65535 && (size_t)rows * (size_t)cols <= J2K_MAX_PIXELS; }
bool coding_ok(int levels, int codeblock) { return levels >= 0 && levels <= 8 && (codeblock == 32 || codeblock == 64); }

uint32_t be16(const uint8_t *p) { return (uint32_t)p[0] << 8 | (uint32_t)p[1]; }
uint32_t be32(const uint8_t *p) { return be16(p) << 16 | be16(p + 2); }

// The box walk of a JP2 file to the contents of its jp2c box; a raw codestream is the whole file.  [*pos, *end) is the
// codestream (a jp2c length of 0, or one that leaves the file, ends it with the file).  Every read is checked against len first.
int codestream_range(const uint8_t *f, size_t len, size_t *pos, size_t *end)
{
	static const uint8_t sig[12] = {0, 0, 0, 12, 'j', 'P', ' ', ' ', 13, 10, 0x87, 10};
	*pos = 0; *end = len;
	if (len < 12 || memcmp(f, sig, 12)) return CCT_OK;
	for (size_t at = 12;;) {
		if (len - at < 8) return CCT_E_J2K;  // no jp2c box
		uint64_t ln = be32(f + at);
		size_t hd = 8;
		if (ln == 1) {
			if (len - at < 16) return CCT_E_J2K;
			ln = (uint64_t)be32(f + at + 8) << 32 | be32(f + at + 12);
			hd = 16;
		}
		if (!memcmp(f + at + 4, "jp2c", 4)) {
			*pos = at + hd;
			if (ln >= hd && ln <= len - at) *end = at + (size_t)ln;
			return CCT_OK;
		}
		if (ln < hd || ln > len - at) return CCT_E_J2K;  // 0 (to the end of the file) on a box that is not jp2c: none follows
		at += (size_t)ln;
	}
}

// SOC and SIZ at the head of the codestream codestream_range finds: the raw fields of a SIZ of one component (Lsiz 41) for the
// caller's own rules.  The segment lies inside the file, or (to_jp2c_end) inside the jp2c box, which ends at end <= len.
struct Siz { uint32_t xs, ys, xo, yo, xt, yt, xto, yto, nc, ssiz, xr, yr; size_t next, end; };  // next: the marker behind SIZ; end: of the codestream
int read_siz(const uint8_t *f, size_t len, bool to_jp2c_end, Siz &z)
{
	size_t pos;
	if (codestream_range(f, len, &pos, &z.end)) return CCT_E_J2K;
	const size_t room = (to_jp2c_end ? z.end : len) - pos;
	if (room < 6 || f[pos] != 0xFF || f[pos + 1] != 0x4F || f[pos + 2] != 0xFF || f[pos + 3] != 0x51) return CCT_E_J2K;
	const size_t lsiz = be16(f + pos + 4);
	if (lsiz != 41 || room - 4 < lsiz) return CCT_E_J2K;
	const uint8_t *s = f + pos + 6;  // Rsiz 2, Xsiz, Ysiz, XOsiz, YOsiz, XTsiz, YTsiz, XTOsiz, YTOsiz 4 each, Csiz 2, Ssiz, XRsiz, YRsiz 1 each
	z.xs = be32(s + 2); z.ys = be32(s + 6); z.xo = be32(s + 10); z.yo = be32(s + 14); z.xt = be32(s + 18); z.yt = be32(s + 22);
	z.xto = be32(s + 26); z.yto = be32(s + 30); z.nc = be16(s + 34); z.ssiz = s[36]; z.xr = s[37]; z.yr = s[38];
	z.next = pos + 4 + lsiz;
	return CCT_OK;
}

// tests/jpeg2000_model.py info(): CCT_OK or CCT_E_J2K.  SIZ is bounded by the file; an image origin and a precision of 1 pass.
int parse_file(const uint8_t *f, size_t len, int *rows, int *cols, int *precision)
{
	Siz z;
	if (read_siz(f, len, false, z)) return CCT_E_J2K;
	if (z.nc != 1 || (z.ssiz & 0x80) || z.ssiz + 1 > 16 || z.xs <= z.xo || z.ys <= z.yo || z.xs - z.xo > 0x7FFFFFFFu || z.ys - z.yo > 0x7FFFFFFFu) return CCT_E_J2K;
	*rows = (int)(z.ys - z.yo); *cols = (int)(z.xs - z.xo); *precision = (int)z.ssiz + 1;
	return CCT_OK;
}

// What the decoder needs of a file it takes (tests/jpeg2000_decode_model.py walk()): CCT_OK or CCT_E_J2K.
struct DecParsed {
	uint32_t rows = 0, cols = 0, precision = 0, levels = 0, layers = 0, seq = 0, xcb = 0, ycb = 0, mb[25] = {};
	size_t data0 = 0, data1 = 0;  // the tile data: behind SOD, up to the end of the tile-part
};
int walk_file(const uint8_t *f, size_t len, DecParsed &o)
{
	Siz z;
	if (read_siz(f, len, true, z)) return CCT_E_J2K;
	if (z.nc != 1 || (z.ssiz & 0x80) || z.ssiz + 1 < 2 || z.ssiz + 1 > 16 || !z.xs || !z.ys || z.xs > 0x7FFFFFFFu || z.ys > 0x7FFFFFFFu) return CCT_E_J2K;
	if (z.xo || z.yo || z.xto || z.yto || z.xt < z.xs || z.yt < z.ys || z.xr != 1 || z.yr != 1) return CCT_E_J2K;  // an origin, more than one tile, subsampling
	o.rows = z.ys; o.cols = z.xs; o.precision = z.ssiz + 1;
	size_t pos = z.next, end = z.end;
	bool have_sot = false, have_cod = false, have_qcd = false;
	size_t sot = 0, nexp = 0;
	uint32_t psot = 0, guard = 0;
	uint8_t exps[25] = {};
	for (;;) {  // the main header up to SOT, then the tile-part header up to SOD
		if (end - pos < 2 || f[pos] != 0xFF) return CCT_E_J2K;
		const uint32_t mk = 0xFF00u | f[pos + 1];
		if (mk == 0xFF93) {
			if (!have_sot) return CCT_E_J2K;
			pos += 2;
			break;
		}
		if (end - pos < 4) return CCT_E_J2K;
		const size_t ln = be16(f + pos + 2);
		if (ln < 2 || ln > end - pos - 2) return CCT_E_J2K;  // a segment that leaves the file
		const uint8_t *seg = f + pos + 4;
		const size_t sl = ln - 2;
		if (mk == 0xFF90) {  // SOT: tile 0, its only tile-part
			if (have_sot || sl != 8 || seg[0] || seg[1] || seg[6] != 0 || seg[7] > 1) return CCT_E_J2K;
			have_sot = true; sot = pos; psot = be32(seg + 2);
		} else if (mk == 0xFF52) {  // COD: Scod, progression, layers, MCT, levels, xcb - 2, ycb - 2, style, transform; no precinct sizes
			if (sl != 10 || seg[0] != 0 || seg[1] > 4 || seg[4] != 0 || seg[8] != 0 || seg[9] != 1) return CCT_E_J2K;
			o.layers = be16(seg + 2); o.levels = seg[5]; o.xcb = seg[6] + 2u; o.ycb = seg[7] + 2u; o.seq = seg[1] != 0;
			if (o.layers < 1 || o.layers > 32 || o.levels > 8 || seg[6] > 4 || seg[7] > 4) return CCT_E_J2K;
			have_cod = true;
		} else if (mk == 0xFF5C) {  // QCD: no quantization
			if (sl < 1 || (seg[0] & 31)) return CCT_E_J2K;
			guard = seg[0] >> 5;
			nexp = std::min<size_t>(sl - 1, 25);
			for (size_t k = 0; k < nexp; k++) exps[k] = seg[1 + k] >> 3;
			have_qcd = true;
		} else if (mk != 0xFF64 && mk != 0xFF55 && mk != 0xFF57 && mk != 0xFF58 && mk != 0xFF63) {  // COM, TLM, PLM, PLT, CRG are skipped
			return CCT_E_J2K;  // COC, QCC, RGN, POC, PPM, PPT, a second SIZ, anything of Part 2
		}
		pos += 2 + ln;
	}
	if (!have_cod || !have_qcd || nexp < 1 + 3 * (size_t)o.levels) return CCT_E_J2K;
	for (uint32_t b = 0; b < 1 + 3 * o.levels; b++) {
		o.mb[b] = guard + exps[b] >= 1 ? guard + exps[b] - 1 : 0;
		if (o.mb[b] > J2K_DEC_MB_MAX) return CCT_E_J2K;
	}
	o.data0 = pos;
	o.data1 = psot ? std::min(sot + (size_t)psot, end) : end;
	if (o.data1 < o.data0) return CCT_E_J2K;
	return CCT_OK;
}

const char *dec_refusal(int code)
{
	return code == CCT_E_J2K     ? "not a JPEG 2000 file this decoder takes"
	       : code == CCT_E_MIXED ? "the file's shape or precision is not the call's"
	                             : "packets: a header or code-block bytes beyond the tile data, too many zero bit-planes or passes, an Lblock above 32";
}

}  // namespace

void cct::j2k_release()
{
	g_enc_ws.release();
	for (auto &w : g_dec_ws) w.release();
}

extern "C" {

// Headers (J2K_HDR_MAX) and EOC, the packet headers, and the slabs of the layout at precision 16, the largest.
// Packet headers: a tag tree over l leaves has fewer than 2 l + 16 nodes; a node of the inclusion tree costs one bit and a
// node of the zero-bit-plane tree at most mb + 1 <= 20; a code-block adds its passes (16 bits at most), Lblock growth (at
// most 30 ones and a zero) and a length of at most 32 + 7 bits: under 16 bytes, under 19 with a stuffed bit behind every
// 0xFF, so J2K_CB_HDR_BYTES = 32 a code-block and J2K_PKT_BYTES = 512 a packet for the 6 x 16 extra nodes of its trees, the
// first bit and the padding.  Slabs: j2k_slab_cap (cct_internal.h).
size_t cct_j2k_bound(int rows, int cols, int levels, int codeblock, int jp2)
{
	(void)jp2;  // J2K_HDR_MAX holds the boxes either way
	if (!shape_ok(rows, cols) || !coding_ok(levels, codeblock)) return 0;
	J2kLayout L;
	j2k_layout((uint32_t)rows, (uint32_t)cols, 16, (uint32_t)levels, (uint32_t)codeblock, L);
	return L.bound;
}

int cct_j2k_info(const uint8_t *h_file, size_t len, int *rows, int *cols, int *precision)
{
	if (!h_file || !rows || !cols || !precision) return fail(CCT_E_ARG, "null argument");
	const int rc = parse_file(h_file, len, rows, cols, precision);
	if (rc) return fail(rc, "not a JPEG 2000 codestream or JP2 file of one unsigned component");
	return CCT_OK;
}

int cct_j2k_encode_batch(const void *images, int images_on_device, int n, int rows, int cols, int src_bits, int precision, int shift, int levels,
                         int codeblock, int jp2, uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes, uint32_t *h_status)
{
	if (!shape_ok(rows, cols))
		return fail(CCT_E_ARG, "JPEG 2000 shape %d x %d: rows and cols 1 .. 65535, at most %zu pixels", rows, cols, J2K_MAX_PIXELS);
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	if (src_bits != 8 && src_bits != 16) return fail(CCT_E_ARG, "JPEG 2000: samples of %d bits: 8 or 16", src_bits);
	if (precision < 2 || precision > 16 || precision > src_bits) return fail(CCT_E_ARG, "JPEG 2000: precision %d: 2 .. %d", precision, src_bits);
	if (shift < 0 || shift > 15 || precision - shift < 1) return fail(CCT_E_ARG, "JPEG 2000: shift %d: 0 .. 15 and below the precision", shift);
	if (levels < 0 || levels > 8) return fail(CCT_E_ARG, "JPEG 2000: %d decomposition levels: 0 .. 8", levels);
	if (codeblock != 32 && codeblock != 64) return fail(CCT_E_ARG, "JPEG 2000: code-blocks of %d: 32 or 64", codeblock);
	const size_t bound = cct_j2k_bound(rows, cols, levels, codeblock, jp2);
	if (out_stride < bound) return fail(CCT_E_CAP, "out_stride %zu too small (need cct_j2k_bound = %zu)", out_stride, bound);
	if (n > 0 && (!images || !h_out || !h_out_sizes || !h_status)) return fail(CCT_E_ARG, "null argument");
	if (n == 0) return CCT_OK;
	J2kLayout L;
	j2k_layout((uint32_t)rows, (uint32_t)cols, (uint32_t)precision, (uint32_t)levels, (uint32_t)codeblock, L);  // L.bound <= bound: smaller slabs
	std::lock_guard<std::mutex> lk(g_mu);
	ApiCall in_call;
	int rc;
	if ((rc = ensure_ctx())) return rc;
	hipStream_t st = main_stream();
	DevBuf *W = g_enc_ws.buf;
	EventPair &ev = g_enc_ws.ev;
	const size_t N = (size_t)rows * cols, img_bytes = N * (src_bits / 8), dstride = (L.bound + 3) & ~(size_t)3, nb = L.blocks.size();
	const size_t blocks_bytes = (nb * sizeof(J2kBlock) + 15) & ~(size_t)15, bands_bytes = L.bands.size() * sizeof(J2kBand);
	const size_t per_frame = 8 * N + L.slab_bytes + dstride + nb * sizeof(J2kBlockOut) + 6 * (size_t)L.tt_nodes;
	const int per_pass = (int)std::max<size_t>(1, J2K_PASS_BYTES / per_frame);
	float ms_sum = 0;
	std::vector<uint32_t> status;
	StreamDrain drain(st);  // copies into caller memory land before any return; L outlives the upload below
	if ((rc = W[E_LAYOUT].ensure(blocks_bytes + bands_bytes))) return rc;
	HIP_TRY(hipMemcpyAsync(W[E_LAYOUT].p, L.blocks.data(), nb * sizeof(J2kBlock), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync((uint8_t *)W[E_LAYOUT].p + blocks_bytes, L.bands.data(), bands_bytes, hipMemcpyHostToDevice, st));
	for (int c0 = 0; c0 < n; c0 += per_pass) {
		const int nc = std::min(per_pass, n - c0);
		const void *d_img;
		if ((rc = rasters_to_device(images, images_on_device, c0, nc, img_bytes, W[E_IMG], st, &d_img))) return rc;
		if ((rc = W[E_PLANE_A].ensure((size_t)nc * N * 4))) return rc;
		if ((rc = W[E_PLANE_B].ensure((size_t)nc * N * 4))) return rc;
		if ((rc = W[E_SLABS].ensure((size_t)nc * L.slab_bytes))) return rc;
		if ((rc = W[E_CBOUT].ensure((size_t)nc * nb * sizeof(J2kBlockOut)))) return rc;
		if ((rc = W[E_TT].ensure((size_t)nc * 6 * L.tt_nodes))) return rc;
		if ((rc = W[E_OUT].ensure((size_t)nc * dstride))) return rc;
		if ((rc = W[E_SIZES].ensure((size_t)nc * 8))) return rc;  // sizes, then the status words
		J2kArgs a{};
		a.images = d_img; a.src_bits = (uint32_t)src_bits; a.n = (uint32_t)nc; a.rows = (uint32_t)rows; a.cols = (uint32_t)cols;
		a.precision = (uint32_t)precision; a.shift = (uint32_t)shift; a.levels = (uint32_t)levels; a.codeblock = (uint32_t)codeblock;
		const int stages = tuning_env("CCT_J2K_STAGES", 7);  // tools/bench_jpeg2000.py: time the stages (read per call: the tool changes it); the files are valid at 7 only
		a.stages = (uint32_t)stages | 1u;
		a.plane_a = (int32_t *)W[E_PLANE_A].p; a.plane_b = (int32_t *)W[E_PLANE_B].p;
		a.blocks = (const J2kBlock *)W[E_LAYOUT].p; a.nblocks = (uint32_t)nb;
		a.bands = (const J2kBand *)((const uint8_t *)W[E_LAYOUT].p + blocks_bytes); a.nbands = (uint32_t)L.bands.size();
		a.slabs = (uint8_t *)W[E_SLABS].p; a.slab_stride = L.slab_bytes;
		a.cbout = (J2kBlockOut *)W[E_CBOUT].p; a.tt = (uint8_t *)W[E_TT].p; a.tt_nodes = L.tt_nodes;
		a.out_sizes = (uint32_t *)W[E_SIZES].p; a.status = a.out_sizes + nc;
		a.hdr_len = j2k_headers((uint32_t)rows, (uint32_t)cols, (uint32_t)precision, (uint32_t)levels, (uint32_t)codeblock, jp2 != 0, a.hdr, &a.psot_at,
		                        &a.jp2c_at);
		a.out = (uint8_t *)W[E_OUT].p; a.out_stride = dstride;
		if ((rc = ev.begin(st))) return rc;
		HIP_TRY(hipMemsetAsync(W[E_SIZES].p, 0, (size_t)nc * 8, st));
		HIP_TRY(launch_j2k_encode(a, st));
		if ((rc = ev.end(st))) return rc;
		status.assign(nc, 0);
		HIP_TRY(hipMemcpyAsync(h_out_sizes + c0, W[E_SIZES].p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(status.data(), a.status, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		if ((rc = ev.add_ms(ms_sum))) return rc;
		for (int i = 0; i < nc; i++)
			h_status[c0 + i] = (status[i] & (J2K_ST_OVERFLOW | J2K_ST_GUARD)) ? CCT_E_OVERFLOW : status[i] ? CCT_E_CAP : CCT_OK;
		if ((rc = files_to_host(h_out + (size_t)c0 * out_stride, out_stride, h_out_sizes + c0, nc, W[E_OUT].p, dstride, 0, L.bound, "frame", c0, "bound", st)))
			return rc;
	}
	set_last_kernel_ms(true, ms_sum);
	for (int i = 0; i < n; i++) {
		if (h_status[i] == CCT_E_OVERFLOW)
			return fail(CCT_E_OVERFLOW, "frame %d: a sample does not fit the precision of %d bits, or a coefficient the guard bits", i, precision);
		if (h_status[i] != CCT_OK) return fail((int)h_status[i], "frame %d: a code-block's bytes do not fit its slab", i);
	}
	return CCT_OK;
}

int cct_j2k_decode_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int rows, int cols, int bits, int shift, void *images,
                         int images_on_device, size_t images_cap_px, uint32_t *h_status)
{
	if (!shape_ok(rows, cols))
		return fail(CCT_E_ARG, "JPEG 2000 shape %d x %d: rows and cols 1 .. 65535, at most %zu pixels", rows, cols, J2K_MAX_PIXELS);
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	if (bits != 8 && bits != 16) return fail(CCT_E_ARG, "JPEG 2000: %d bits allocated: 8 or 16", bits);
	if (shift < 0 || shift > 15) return fail(CCT_E_ARG, "JPEG 2000: shift %d: 0 .. 15", shift);
	const size_t N = (size_t)rows * cols, px_bytes = (size_t)bits / 8;
	if (images_cap_px / N < (size_t)n) return fail(CCT_E_CAP, "output holds %zu pixels, need %zu", images_cap_px, (size_t)n * N);
	if (n > 0 && (!h_files || !h_offsets || !images || !h_status)) return fail(CCT_E_ARG, "null argument");
	int rc;
	if ((rc = check_offsets(h_offsets, n, "file"))) return rc;
	if (n == 0) return CCT_OK;
	// the marker walk: every structural refusal is decided here, before the device is touched.  Files of the same coding
	// (the usual batch has one) share a layout.
	std::vector<DecParsed> parsed(n);
	std::vector<J2kDecLayout> layouts;
	std::vector<int> layout_of(n, -1);
	for (int i = 0; i < n; i++) {
		const size_t len = (size_t)(h_offsets[i + 1] - h_offsets[i]);
		DecParsed &p = parsed[i];
		int r = len > 0x7FFFFFFFull ? CCT_E_J2K : walk_file(h_files + h_offsets[i], len, p);
		if (r == CCT_OK && (p.rows != (uint32_t)rows || p.cols != (uint32_t)cols || p.precision > (uint32_t)bits)) r = CCT_E_MIXED;
		h_status[i] = (uint32_t)r;
		if (r) continue;
		for (size_t k = 0; k < layouts.size() && layout_of[i] < 0; k++)
			if (layouts[k].levels == p.levels && layouts[k].xcb == p.xcb && layouts[k].ycb == p.ycb && !memcmp(layouts[k].mb, p.mb, sizeof(p.mb)))
				layout_of[i] = (int)k;
		if (layout_of[i] < 0) {
			layouts.emplace_back();
			J2kDecLayout &L = layouts.back();
			L.levels = p.levels; L.xcb = p.xcb; L.ycb = p.ycb;
			memcpy(L.mb, p.mb, sizeof(p.mb));
			j2k_dec_layout((uint32_t)rows, (uint32_t)cols, L);
			layout_of[i] = (int)layouts.size() - 1;
		}
	}
	if (std::all_of(h_status, h_status + n, [](uint32_t s) { return s != CCT_OK; }))  // nothing to send: no device needed
		return fail((int)h_status[0], "file 0: %s", dec_refusal((int)h_status[0]));
	std::vector<J2kDecBlock> blocks;
	std::vector<J2kDecBand> bands;
	std::vector<uint32_t> blk0(layouts.size()), band0(layouts.size());
	for (size_t k = 0; k < layouts.size(); k++) {
		blk0[k] = (uint32_t)blocks.size(); band0[k] = (uint32_t)bands.size();
		blocks.insert(blocks.end(), layouts[k].blocks.begin(), layouts[k].blocks.end());
		bands.insert(bands.end(), layouts[k].bands.begin(), layouts[k].bands.end());
	}
	const size_t blocks_bytes = (blocks.size() * sizeof(J2kDecBlock) + 15) & ~(size_t)15;
	auto chunk_cap = [&](int i) { return std::min<uint64_t>(parsed[i].data1 - parsed[i].data0, (uint64_t)layouts[layout_of[i]].blocks.size() * parsed[i].layers); };
	auto file_bytes = [&](int i) -> uint64_t {  // device bytes a file of the batch takes in its pass
		uint64_t b = 2 * (h_offsets[i + 1] - h_offsets[i]) + N * (8 + px_bytes);
		if (h_status[i] == CCT_OK) {
			const J2kDecLayout &L = layouts[layout_of[i]];
			b += L.blocks.size() * sizeof(J2kDecCb) + 4 * (uint64_t)L.tt_nodes + chunk_cap(i) * sizeof(J2kDecChunk) + sizeof(J2kDecFile);
		}
		return b;
	};
	const int stages = tuning_env("CCT_J2K_DEC_STAGES", 15);  // tools/bench_jpeg2000_decode.py: time the stages (read per call); the rasters are valid at 15 only
	DecLease lease;
	if ((rc = lease_decode_slot(lease))) return rc;
	hipStream_t st = lease.stream;
	DevBuf *W = g_dec_ws[lease.slot].buf;
	EventPair &ev = g_dec_ws[lease.slot].ev;
	float ms_sum = 0;
	std::vector<J2kDecFile> flist;
	std::vector<J2kDecRun> runs;
	std::vector<uint32_t> status;
	std::vector<int> file_of;
	StreamDrain drain(st);  // declared after the vectors the copies land in
	if ((rc = W[D_LAYOUT].ensure(blocks_bytes + bands.size() * sizeof(J2kDecBand)))) return rc;
	HIP_TRY(hipMemcpyAsync(W[D_LAYOUT].p, blocks.data(), blocks.size() * sizeof(J2kDecBlock), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync((uint8_t *)W[D_LAYOUT].p + blocks_bytes, bands.data(), bands.size() * sizeof(J2kDecBand), hipMemcpyHostToDevice, st));
	for (int c0 = 0; c0 < n;) {
		int c1 = c0 + 1;
		uint64_t pass_bytes = file_bytes(c0);
		while (c1 < n && pass_bytes + file_bytes(c1) <= J2K_DEC_PASS_BYTES) pass_bytes += file_bytes(c1++);
		const uint64_t a0 = h_offsets[c0], a1 = h_offsets[c1];
		flist.clear(); runs.clear(); file_of.clear();
		uint64_t ncbs = 0, tt_bytes = 0, nchunks = 0;
		uint32_t max_levels = 0;
		for (int i = c0; i < c1; i++) {
			if (h_status[i] != CCT_OK) continue;
			const DecParsed &p = parsed[i];
			const J2kDecLayout &L = layouts[layout_of[i]];
			J2kDecFile f{};
			f.src = h_offsets[i] - a0 + p.data0; f.len = (uint32_t)(p.data1 - p.data0); f.slot = (uint32_t)(i - c0);
			f.precision = p.precision; f.levels = p.levels; f.layers = p.layers; f.seq = p.seq;
			f.blk0 = blk0[layout_of[i]]; f.nblocks = (uint32_t)L.blocks.size(); f.band0 = band0[layout_of[i]];
			f.cb0 = (uint32_t)ncbs; f.tt0 = tt_bytes; f.tt_nodes = L.tt_nodes; f.chunk0 = nchunks; f.chunk_cap = (uint32_t)chunk_cap(i);
			f.xcb = p.xcb; f.ycb = p.ycb;
			if (runs.empty() || runs.back().xcb != p.xcb || runs.back().ycb != p.ycb) runs.push_back(J2kDecRun{f.cb0, 0, p.xcb, p.ycb});
			runs.back().ncbs += f.nblocks;
			ncbs += f.nblocks; tt_bytes += 4 * (uint64_t)L.tt_nodes; nchunks += f.chunk_cap;
			max_levels = std::max(max_levels, p.levels);
			flist.push_back(f); file_of.push_back(i);
		}
		if (!flist.empty()) {
			if (ncbs > 0x7FFFFFFFull) return fail(CCT_E_ARG, "JPEG 2000: too many code-blocks in one pass");
			const size_t abytes = (size_t)(a1 - a0), nf = flist.size();
			uint8_t *d_img = images_on_device ? (uint8_t *)images + (size_t)c0 * N * px_bytes : nullptr;
			if (!images_on_device) {
				if ((rc = W[D_IMG].ensure((size_t)(c1 - c0) * N * px_bytes))) return rc;
				d_img = (uint8_t *)W[D_IMG].p;
			}
			if ((rc = W[D_FILES].ensure(abytes + 16))) return rc;
			if ((rc = W[D_SEGS].ensure(abytes + 16))) return rc;  // Tier-1 reads whole aligned words
			if ((rc = W[D_FLIST].ensure(nf * sizeof(J2kDecFile)))) return rc;
			if ((rc = W[D_CBS].ensure((size_t)ncbs * sizeof(J2kDecCb)))) return rc;
			if ((rc = W[D_TT].ensure((size_t)tt_bytes))) return rc;
			if ((rc = W[D_CHUNKS].ensure((size_t)nchunks * sizeof(J2kDecChunk) + 16))) return rc;
			if ((rc = W[D_STATUS].ensure(nf * 4))) return rc;
			if ((rc = W[D_PLANE_A].ensure((size_t)(c1 - c0) * N * 4))) return rc;
			if ((rc = W[D_PLANE_B].ensure((size_t)(c1 - c0) * N * 4))) return rc;
			HIP_TRY(hipMemcpyAsync(W[D_FILES].p, h_files + a0, abytes, hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(W[D_FLIST].p, flist.data(), nf * sizeof(J2kDecFile), hipMemcpyHostToDevice, st));
			J2kDecArgs a{};
			a.files = (const uint8_t *)W[D_FILES].p; a.segs = (uint8_t *)W[D_SEGS].p;
			a.flist = (const J2kDecFile *)W[D_FLIST].p; a.nfiles = (uint32_t)nf;
			a.blocks = (const J2kDecBlock *)W[D_LAYOUT].p; a.bands = (const J2kDecBand *)((const uint8_t *)W[D_LAYOUT].p + blocks_bytes);
			a.cbs = (J2kDecCb *)W[D_CBS].p; a.ncbs = (uint32_t)ncbs; a.tt = (uint8_t *)W[D_TT].p; a.chunks = (J2kDecChunk *)W[D_CHUNKS].p;
			a.status = (uint32_t *)W[D_STATUS].p; a.plane_a = (int32_t *)W[D_PLANE_A].p; a.plane_b = (int32_t *)W[D_PLANE_B].p;
			a.nslots = (uint32_t)(c1 - c0); a.rows = (uint32_t)rows; a.cols = (uint32_t)cols; a.max_levels = max_levels;
			a.out_bits = (uint32_t)bits; a.shift = (uint32_t)shift; a.stages = (uint32_t)stages | 1u;
			a.images = d_img;
			if ((rc = ev.begin(st))) return rc;
			HIP_TRY(hipMemsetAsync(W[D_STATUS].p, 0, nf * 4, st));
			HIP_TRY(launch_j2k_decode(a, runs.data(), runs.size(), st));
			if ((rc = ev.end(st))) return rc;
			status.assign(nf, 0);
			HIP_TRY(hipMemcpyAsync(status.data(), W[D_STATUS].p, nf * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			if ((rc = ev.add_ms(ms_sum))) return rc;
			for (size_t k = 0; k < nf; k++)
				if (status[k]) h_status[file_of[k]] = CCT_E_STREAM;
			if (!images_on_device && (rc = good_rasters_to_host(images, d_img, N * px_bytes, h_status, c0, c1, st))) return rc;
		}
		c0 = c1;
	}
	set_last_kernel_ms(false, ms_sum);
	for (int i = 0; i < n; i++)
		if (h_status[i] != CCT_OK) return fail((int)h_status[i], "file %d: %s", i, dec_refusal((int)h_status[i]));
	return CCT_OK;
}

}  // extern "C"
