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

enum { E_IMG, E_PLANE_A, E_PLANE_B, E_LAYOUT, E_SLABS, E_CBOUT, E_TT, E_OUT, E_SIZES, E_NBUF };
Workspace<E_NBUF> g_enc_ws;  // under g_mu

bool shape_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && rows <= 65535 && cols <= 65535 && (size_t)rows * (size_t)cols <= J2K_MAX_PIXELS; }
bool coding_ok(int levels, int codeblock) { return levels >= 0 && levels <= 8 && (codeblock == 32 || codeblock == 64); }

uint32_t be16(const uint8_t *p) { return (uint32_t)p[0] << 8 | (uint32_t)p[1]; }
uint32_t be32(const uint8_t *p) { return be16(p) << 16 | be16(p + 2); }

// tests/jpeg2000_model.py info(): CCT_OK or CCT_E_J2K.  Every read is checked against len first.
int parse_file(const uint8_t *f, size_t len, int *rows, int *cols, int *precision)
{
	static const uint8_t sig[12] = {0, 0, 0, 12, 'j', 'P', ' ', ' ', 13, 10, 0x87, 10};
	size_t pos = 0;
	if (len >= 12 && !memcmp(f, sig, 12)) {
		for (pos = 12;;) {
			if (len - pos < 8) return CCT_E_J2K;  // no jp2c box
			uint64_t ln = be32(f + pos);
			size_t hd = 8;
			if (ln == 1) {
				if (len - pos < 16) return CCT_E_J2K;
				ln = (uint64_t)be32(f + pos + 8) << 32 | be32(f + pos + 12);
				hd = 16;
			}
			if (!memcmp(f + pos + 4, "jp2c", 4)) { pos += hd; break; }
			if (ln < hd || ln > len - pos) return CCT_E_J2K;  // 0 (to the end of the file) on a box that is not jp2c: none follows
			pos += (size_t)ln;
		}
	}
	if (len - pos < 6 || f[pos] != 0xFF || f[pos + 1] != 0x4F || f[pos + 2] != 0xFF || f[pos + 3] != 0x51) return CCT_E_J2K;
	const size_t lsiz = be16(f + pos + 4);
	if (lsiz != 41 || len - pos - 4 < lsiz) return CCT_E_J2K;  // one component; SIZ inside the file
	const uint8_t *s = f + pos + 6;  // Rsiz 2, Xsiz, Ysiz, XOsiz, YOsiz, XTsiz, YTsiz, XTOsiz, YTOsiz 4 each, Csiz 2, Ssiz 1
	const uint32_t xs = be32(s + 2), ys = be32(s + 6), xo = be32(s + 10), yo = be32(s + 14), nc = be16(s + 34), ssiz = s[36];
	if (nc != 1 || (ssiz & 0x80) || ssiz + 1 > 16 || xs <= xo || ys <= yo || xs - xo > 0x7FFFFFFFu || ys - yo > 0x7FFFFFFFu) return CCT_E_J2K;
	*rows = (int)(ys - yo); *cols = (int)(xs - xo); *precision = (int)ssiz + 1;
	return CCT_OK;
}

}  // namespace

void cct::j2k_release() { g_enc_ws.release(); }

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
		const char *stages = getenv("CCT_J2K_STAGES");  // tools/bench_jpeg2000.py: time the stages; the files are valid at 7 only
		a.stages = stages ? (uint32_t)atoi(stages) | 1u : 7u;
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

}  // extern "C"
