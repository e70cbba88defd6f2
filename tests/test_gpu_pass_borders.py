"""Batches that run as several passes: the seven pass loops of the JPEG-LS, TIFF and PNG entry points, each
run once over a border with the plans of tests/pass_borders.py.  Pass 2 and later index device pointers, host results,
statuses and the per-pass tables by c0; every small-shape test of these codecs runs with c0 == 0.

Encoders: file i of the multi-pass batch is byte for byte the file a single-pass call of the distinct rasters gives (the
calls the small-shape tests hold to the models, Pillow and zlib; the distinct rasters are held to those references here
too), from host memory and from a DeviceBuffer.  Decoders: every good raster comes back, into host memory and into
out_dev, the refusals planted on both sides of the border sit at their indices with the models' codes, and a sentinel
shows what was written where.  After each big call a small call of another shape must still agree with its model: the
workspaces and tables the big call left must not leak into it.

tests/test_pass_borders_host.py asserts, without a device, that each plan crosses its border where this file says."""
import io
import zlib

import numpy as np
import pytest

import jpeg_ls_model as jm
import pass_borders as pb
import png8_model as p8
import png_files as pf
import png_model as pm
import tiff_model as tm

pytestmark = pytest.mark.gpu

SENTINEL16 = pb.SENTINEL * 0x0101


def _lib():
    from cct_hip import _ffi
    return _ffi.lib()


def _same_files(plan, got, want, idx, where):
    """got[i] is the single-pass file of frame i's raster, for every i"""
    assert len(got) == plan.n
    for key, at in idx.items():
        for i in at:
            assert got[i] == want[key], f"{plan.name} ({where}): file {i} ({key}) of passes {plan.passes} is not its single-pass file"


def _encode_both_ways(plan, encode, want, imgs, idx, small):
    """One call from host memory, one from a DeviceBuffer (images + c0 * img_bytes): the same files.  small() runs after each:
    a single-pass call of another shape against its model, which the big call's workspaces and tables must not reach."""
    import cct_hip
    got = encode(imgs)
    small()
    _same_files(plan, got, want, idx, "host rasters")
    d = cct_hip.DeviceBuffer.from_numpy(imgs)
    try:
        from_dev = encode(d, shape=imgs.shape, dtype=imgs.dtype)
    finally:
        d.free()
    small()
    _same_files(plan, from_dev, want, idx, "device rasters")


# ---- encoders ----------------------------------------------------------------------------------------------------------------

def test_jpegls_encode_batch_over_a_pass_border():
    """1226 uint8 frames of 40 x 500 at precision 7 in intervals of 16 lines run as 1223 + 3.  The frames at c0 - 1 and
    c0 + 1 hold a sample of 128: CCT_E_OVERFLOW and size 0 at exactly those indices, every other file right.  The model
    encodes every distinct raster (20000 samples each: affordable), and the device decoder returns them."""
    import cct_hip
    L = _lib()
    plan = pb.jls_encode_plan()
    print(plan.describe())
    prec, rr = plan.params["precision"], plan.params["restart_rows"]
    imgs, table, idx = pb.rasters_of(plan)
    good = [k for k in table if k[0] != "overflow"]
    small = cct_hip.jpeg_ls_encode_batch(np.stack([table[k] for k in good]), precision=prec, restart_rows=rr)   # one pass
    want = dict(zip(good, small))
    for k in good:
        assert want[k] == jm.encode_frame(table[k], prec, rr), k
    assert np.array_equal(cct_hip.jpeg_ls_decode_batch(small, plan.rows, plan.cols, bits=8), np.stack([table[k] for k in good]))
    bad = sorted(i for i, r in plan.roles.items() if r == "overflow")
    c0 = plan.passes[1][0]
    assert bad == [c0 - 1, c0 + 1] and all(imgs[i].max() == 1 << prec for i in bad)
    stride = L.cct_jpegls_bound(plan.rows, plan.cols, rr)
    c = jm.raster_cases(17, 130, 12)
    small_imgs, small_want = np.stack(list(c.values())), [jm.encode_frame(x, 12, 2) for x in c.values()]
    d = cct_hip.DeviceBuffer.from_numpy(imgs)
    try:
        for where, ptr, on_device in (("host rasters", imgs.ctypes.data, 0), ("device rasters", d.ptr, 1)):
            out = np.empty((plan.n, stride), np.uint8)
            sizes, status = np.full(plan.n, 0xFFFFFFFF, np.uint32), np.full(plan.n, 0xFFFFFFFF, np.uint32)
            rc = L.cct_jpegls_encode_batch(ptr, on_device, plan.n, plan.rows, plan.cols, 8, prec, rr, out.ctypes.data, stride, sizes.ctypes.data,
                                           status.ctypes.data)
            # the big call's workspaces and interval tables must not leak into a small one of another shape
            assert cct_hip.jpeg_ls_encode_batch(small_imgs, precision=12, restart_rows=2) == small_want, where
            assert rc == pb.E_OVERFLOW, where
            assert np.flatnonzero(status).tolist() == bad and (status[bad] == pb.E_OVERFLOW).all(), (where, np.flatnonzero(status)[:8])
            assert np.flatnonzero(sizes == 0).tolist() == bad, where
            for key, at in idx.items():
                if key[0] != "overflow":
                    for i in at:
                        assert sizes[i] == len(want[key]) and out[i, :sizes[i]].tobytes() == want[key], (where, i, key)
    finally:
        d.free()


def _tiff_encode_over_a_border(plan):
    import cct_hip
    print(plan.describe())
    comp, pred = plan.params["compression"], plan.params["predictor"]
    imgs, table, idx = pb.rasters_of(plan)
    keys = list(table)
    want = dict(zip(keys, cct_hip.tiff_encode_batch(np.stack([table[k] for k in keys]), comp, pred)))   # one pass
    for k in keys:
        if comp == "none":  # Pillow writes no file of this layout without a coder: the model's file
            assert want[k] == tm.write_file(table[k], comp, pred), k
        else:
            assert tm.same_file(want[k], tm.pillow_file(table[k], comp, pred)), k
        assert len(tm.parse(want[k])["offs"]) == 2
    name, a, rpss = [c for c in tm.raster_cases() if c[0] == "smooth_37x50"][0]
    small_want = [tm.write_file(a, c, 1 if c == "none" else 2, 7) for c in ("lzw", "deflate", "none")]

    def small():
        assert [cct_hip.tiff_encode_batch(a, c, 1 if c == "none" else 2, 7)[0] for c in ("lzw", "deflate", "none")] == small_want

    _encode_both_ways(plan, lambda x, **kw: cct_hip.tiff_encode_batch(x, comp, pred, **kw), want, imgs, idx, small)


def test_tiff_encode_batch_lzw_over_a_pass_border():
    """1377 uint16 rasters of 100 x 500 as LZW with the predictor, two strips a file (65 + 35 rows), run as 1375 + 2: the
    coded strips have slots of their own (E_CODED, E_CSIZES), sized by nc * 2 strips"""
    _tiff_encode_over_a_border(pb.tiff_encode_plan())


def test_tiff_encode_batch_deflate_over_a_pass_border():
    """The same rasters as Deflate with the predictor.  The strips go through the DEFLATE pass of the encode slot, one string a
    strip at memLevel 8 and the default strategy, which no PNG batch reaches: nc * 2 strings in the full pass and 4 in the
    last one, so other DEFLATE arguments and another captured graph, the slot's streams and size table left from the
    fuller pass, and pk.src 13 bytes into that slot's stride."""
    _tiff_encode_over_a_border(pb.tiff_encode_deflate_plan())


def test_tiff_encode_batch_none_over_a_pass_border():
    """The same rasters uncompressed: the files are packed straight from the staged strips (pk.src = W[E_STRIPS] at
    strip_stride), the one path on which the strip stride of a pass reaches the file."""
    _tiff_encode_over_a_border(pb.tiff_encode_none_plan())


def _png_references(want, table, depth):
    """Pillow's decode of each distinct file is the raster, and the IDAT data inflates to the filtered rows"""
    from PIL import Image
    for k, f in want.items():
        x = table[k]
        assert np.array_equal(np.array(Image.open(io.BytesIO(f))), x), k
        rows = pm.filter_rows(x)[1] if depth == 16 else p8.filter_rows8(x)[1]
        assert zlib.decompress(pm.idat_stream(f)) == rows, k
        assert f == (pm.pillow_bytes(x, 6) if depth == 16 else p8.pillow8_bytes(x, 6)), k


def test_png_encode_batch_over_a_pass_border():
    """2051 uint16 slices of 512 x 511 at level 6: 524032 bytes of DEFLATE input a slice, 2049 slices a pass, 2049 + 2.  The
    last pass has other DEFLATE arguments and another captured graph than the first."""
    import cct_hip
    plan = pb.png_encode_plan(16)
    print(plan.describe())
    imgs, table, idx = pb.rasters_of(plan)
    keys = list(table)
    want = dict(zip(keys, cct_hip.png_encode_batch(np.stack([table[k] for k in keys]), level=6)))
    _png_references(want, table, 16)
    odd = pm.cases()["odd"]
    odd_want = pm.png_bytes(odd, 6)

    def small():
        assert cct_hip.png_encode_batch(odd, level=6)[0] == odd_want

    _encode_both_ways(plan, lambda x, **kw: cct_hip.png_encode_batch(x, level=6, shape=kw.get("shape")), want, imgs, idx, small)


def test_png_encode8_batch_over_a_pass_border():
    """the same shape through the 8-bit writer: 262400 bytes a slice, 4092 slices a pass, 4092 + 2 uint8 slices"""
    import cct_hip
    plan = pb.png_encode_plan(8)
    print(plan.describe())
    imgs, table, idx = pb.rasters_of(plan)
    keys = list(table)
    want = dict(zip(keys, cct_hip.png8_encode_batch(np.stack([table[k] for k in keys]), level=6)))
    _png_references(want, table, 8)
    odd = (pm.cases()["odd"] & 255).astype(np.uint8)
    odd_want = p8.png8_bytes(odd, 6)

    def small():
        assert cct_hip.png8_encode_batch(odd, level=6)[0] == odd_want

    _encode_both_ways(plan, lambda x, **kw: cct_hip.png8_encode_batch(x, level=6, **kw), want, imgs, idx, small)


# ---- decoders ----------------------------------------------------------------------------------------------------------------

def _decode_raw(plan, blob, offs, images, on_device, cap_px, status):
    L = _lib()
    arg = 0 if plan.entry == "cct_png_read_batch" else 16   # the reader's shift; the others' bits
    return getattr(L, plan.entry)(blob, offs.ctypes.data, plan.n, plan.rows, plan.cols, arg, images, on_device, cap_px, status.ctypes.data)


def _check_rasters(plan, got, table, idx, where, keeps_sentinel):
    """every good raster is its source; keeps_sentinel(role) -> the slots of that role must still hold the sentinel"""
    for key, at in idx.items():
        f, x, st = table[key]
        if st == 0:
            bad = [int(i) for i in at if not np.array_equal(got[i], x)]
            assert not bad, f"{plan.name} ({where}): rasters {bad[:6]} ({key}) of passes {plan.passes} are not their source"
        elif keeps_sentinel(key[0]):
            bad = [int(i) for i in at if not (got[i] == SENTINEL16).all()]
            assert not bad, f"{plan.name} ({where}): the slots of the refused files {bad[:6]} ({key}) were written"


def _decode_both_ways(plan, host_keeps, device_keeps, small):
    """One call into host memory, one into out_dev, both over a sentinel.  Statuses at exactly the plan's indices.  small()
    runs after each call: a single-pass call of another shape against its model."""
    import cct_hip
    print(plan.describe())
    files, table, idx = pb.batch_of(plan)
    want = np.array([table[k][2] for k in plan.keys()], np.uint32)
    blob = b"".join(files)
    offs = np.zeros(plan.n + 1, np.uint64)
    np.cumsum([len(f) for f in files], out=offs[1:])
    px = plan.rows * plan.cols
    first = int(want[np.flatnonzero(want)[0]]) if want.any() else 0
    host = np.full((plan.n + 1, plan.rows, plan.cols), SENTINEL16, np.uint16)
    status = np.full(plan.n, 0xFFFFFFFF, np.uint32)
    rc = _decode_raw(plan, blob, offs, host.ctypes.data, 0, plan.n * px, status)
    small()
    assert rc == first
    assert np.array_equal(status, want), ("host", np.flatnonzero(status != want)[:8], status[status != want][:8], want[status != want][:8])
    _check_rasters(plan, host, table, idx, "host memory", host_keeps)
    assert (host[plan.n] == SENTINEL16).all()
    del host
    d = cct_hip.DeviceBuffer((plan.n + 1) * px * 2)
    try:
        from cct_hip import _ffi
        _ffi.check(_lib().cct_dev_memset(d.ptr, pb.SENTINEL, d.nbytes))
        status = np.full(plan.n, 0xFFFFFFFF, np.uint32)
        rc = _decode_raw(plan, blob, offs, d.ptr, 1, plan.n * px, status)
        small()
        assert rc == first
        dev = d.download(np.uint16, (plan.n + 1) * px).reshape(plan.n + 1, plan.rows, plan.cols)
    finally:
        d.free()
    assert np.array_equal(status, want), ("out_dev", np.flatnonzero(status != want)[:8], status[status != want][:8], want[status != want][:8])
    _check_rasters(plan, dev, table, idx, "out_dev", device_keeps)
    assert (dev[plan.n] == SENTINEL16).all()   # nothing behind the batch


def _refusals_are_where_the_plan_says(plan):
    c0 = plan.passes[1][0]
    files, table, idx = pb.batch_of(plan)
    codes = [table[plan.key(i)][2] for i in range(c0 - 3, c0 + 3)]
    assert codes[0] == 0 and codes[5] == 0 and all(codes[1:5])
    return codes


HOST_REFUSED = lambda role: role.startswith("host:")  # noqa: E731
ANY_REFUSED = lambda role: True  # noqa: E731
NONE = lambda role: False  # noqa: E731


def _small_jls_decode():
    import cct_hip
    c = jm.raster_cases(5, 63, 8)
    files = [jm.encode_frame(x, 8, rr) for x, rr in zip(c.values(), (0, 1, 2, 0, 1, 2, 0))]
    assert np.array_equal(cct_hip.jpeg_ls_decode_batch(files, 5, 63, bits=8), np.stack(list(c.values())))


def test_jpegls_decode_batch_over_the_raster_border():
    """13424 files of 40 x 500 at precision 12: 13421 uint16 rasters fill 512 MiB, so the batch runs as 13421 + 3 while its
    files take a quarter of the 128 MiB a pass may hold.  c0 - 2: a scan header of two components (CCT_E_JPEGLS); c0 - 1: a last
    interval three bytes short (CCT_E_STREAM); c0: a first interval four bytes short (CCT_E_STREAM); c0 + 1: a file that ends
    in its SOF55 (CCT_E_JPEGLS).  A refused frame's slot in host memory stays as it was (good_rasters_to_host), and in
    out_dev the slot of a frame the host refused."""
    plan = pb.jls_decode_rasters_plan()
    assert _refusals_are_where_the_plan_says(plan) == [0, pb.E_JPEGLS, pb.E_STREAM, pb.E_STREAM, pb.E_JPEGLS, 0]
    _decode_both_ways(plan, ANY_REFUSED, HOST_REFUSED, _small_jls_decode)


def test_jpegls_decode_batch_over_the_file_byte_border():
    """10615 files of 24 x 250 white noise at precision 16: 12.6 KB a file for 12 KB of raster, so 128 MiB of files end the
    first pass after 10613 of them, with a quarter of the raster budget used: the cut rule no other test reaches."""
    plan = pb.jls_decode_files_plan()
    assert plan.why == ["files", "end"]
    _decode_both_ways(plan, ANY_REFUSED, HOST_REFUSED, _small_jls_decode)


def test_jpegls_decode_batch_with_a_pass_of_refused_files():
    """13421 good files, 13421 files of four bytes the marker walk refuses, 2 good files: the refused run is one pass by its
    rasters, frames.empty(), and leaves host and device slots alone; the passes around it decode."""
    plan = pb.jls_decode_refused_pass_plan()
    _decode_both_ways(plan, ANY_REFUSED, HOST_REFUSED, _small_jls_decode)


def _small_tiff_read():
    import cct_hip
    name, a, rpss = [c for c in tm.raster_cases() if c[0] == "smooth_37x50"][0]
    files = [tm.write_file(a, "deflate", 2, 7), tm.write_file(a, "none", 1, 37), tm.write_file(a, "lzw", 2, 1), tm.build_file(a, 8, 1, 5, "MM")]
    assert np.array_equal(cct_hip.tiff_read_batch(files, 37, 50), np.stack([a] * 4))


def test_tiff_read_batch_over_the_raster_border():
    """29025 files of 37 x 250 uint16 in strips of 16 rows: LZW, Deflate and uncompressed, II and MM, by index % 7 in the pass
    of 29020 and by name in the pass of 5 (Deflate MM, uncompressed MM, LZW II, Deflate II reach the device), so all of
    part[0 .. 2] is filled in both passes and differently.  c0 - 2: PackBits (CCT_E_TIFF); c0 - 1: an
    LZW strip half there; c0: a Deflate strip with a flipped bit, as tiff_model.damaged_files() builds them, with the
    model's codes; c0 + 1: BigTIFF (CCT_E_TIFF)."""
    plan = pb.tiff_read_rasters_plan()
    codes = _refusals_are_where_the_plan_says(plan)
    assert codes[1] == codes[4] == pb.E_TIFF and codes[2] == pb.E_STREAM and codes[3] in (pb.E_ZLIB, pb.E_STREAM)
    _decode_both_ways(plan, ANY_REFUSED, HOST_REFUSED, _small_tiff_read)


def test_tiff_read_batch_over_the_file_byte_border():
    """23870 files of white noise, LZW (a third longer than the raster) and Deflate in both byte orders: 512 MiB of files end
    the first pass after 23868, with 421 MiB of rasters"""
    plan = pb.tiff_read_files_plan()
    assert plan.why == ["files", "end"]
    _decode_both_ways(plan, ANY_REFUSED, HOST_REFUSED, _small_tiff_read)


def test_tiff_read_batch_with_a_pass_of_refused_files():
    """29020 good files, 29020 files of four bytes, 2 good files: strips.empty() in the middle pass"""
    plan = pb.tiff_read_refused_pass_plan()
    _decode_both_ways(plan, ANY_REFUSED, HOST_REFUSED, _small_tiff_read)


def _small_png_read():
    import cct_hip
    cases = pf.chunk_cases()
    assert np.array_equal(cct_hip.png_read_batch([f for _, f, _ in cases]), np.stack([x for _, _, x in cases]))


def test_png_read_batch_over_a_pass_border():
    """2052 files of 512 x 511, 8 and 16 bits deep by index: 2049 + 3.  c0 - 2: a file cut inside its IDAT (CCT_E_PNG);
    c0 - 1: a data byte flipped under its CRC (CCT_E_CRC); c0: a stream whose Adler-32 is off (CCT_E_ZLIB); c0 + 1: a bad
    signature (CCT_E_PNG).  The header leaves a refused file's raster unspecified: nothing outside its slot may change."""
    plan = pb.png_read_plan()
    assert _refusals_are_where_the_plan_says(plan) == [0, pb.E_PNG, pb.E_CRC, pb.E_ZLIB, pb.E_PNG, 0]
    _decode_both_ways(plan, NONE, NONE, _small_png_read)


def test_png_read_batch_with_a_pass_of_refused_files():
    """2049 good files, 2049 files of four bytes, 2 good files: max_bpp == 0 in the middle pass, which then touches nothing on
    the device.  In host memory the reader copies whole passes back, so the refused pass's slots there are unspecified like
    any refused file's; in out_dev they stay as they were."""
    plan = pb.png_read_refused_pass_plan()
    _decode_both_ways(plan, NONE, HOST_REFUSED, _small_png_read)
