"""Device JPEG 2000 lossless decoder (cct_j2k_decode_batch): it inverts the device encoder over shapes, precisions, levels and
code-block sizes; it equals tests/jpeg2000_decode_model.py on OpenJPEG's own files, on hand-built files and on damaged files;
the refusals per file and per call; the two real slices; a batch of two passes."""
import functools
import io

import numpy as np
import pytest

import golden_inputs as gi
import jpeg2000_decode_model as d
import jpeg2000_model as m

pytestmark = pytest.mark.gpu

CODES = {"CCT_E_STREAM": 4, "CCT_E_MIXED": 10, "CCT_E_J2K": 14}
E_STREAM, E_CAP, E_ARG, E_MIXED, E_J2K = 4, 6, 9, 10, 14


def needs_pillow():
    if not d.pillow_has_jpeg2000():
        pytest.skip("this Pillow has no JPEG 2000 codec")


@pytest.mark.parametrize("precision", sorted(m.PRECISIONS))
def test_decode_inverts_the_device_encoder(precision):
    import cct_hip
    bits = 8 if precision == 8 else 16
    for rows, cols, cbs in m.SHAPES:
        imgs = np.stack(list(m.raster_cases(rows, cols, precision, m.PRECISIONS[precision]).values()))
        for cb in cbs:
            for levels in m.LEVELS:
                files = cct_hip.jpeg2000_encode_batch(imgs, precision=precision, levels=levels, codeblock=cb)
                got = cct_hip.jpeg2000_decode_batch(files, rows, cols, bits=bits)  # one mixed batch per shape
                assert got.dtype == imgs.dtype and np.array_equal(got, imgs), (rows, cols, cb, levels)


def test_shift_jp2_device_output_and_the_empty_batch():
    import cct_hip
    imgs = np.stack([p[0] for p in m.phantoms()[:2]]) >> 4  # 12 bits of 128 x 128
    for jp2 in (False, True):
        files = cct_hip.jpeg2000_encode_batch(imgs, precision=16, shift=4, jp2=jp2)
        assert np.array_equal(cct_hip.jpeg2000_decode_batch(files, 128, 128, shift=4), imgs)
        assert np.array_equal(cct_hip.jpeg2000_decode_batch(files, 128, 128), imgs << 4)
    mixed = [files[0], cct_hip.jpeg2000_encode_batch(imgs[1], precision=12, levels=2, codeblock=32)[0]]  # two codings, two precisions
    out = cct_hip.DeviceBuffer(2 * 128 * 128 * 2)
    try:
        assert cct_hip.jpeg2000_decode_batch(mixed, 128, 128, out_dev=out) == (2, 128, 128)
        got = out.download(np.uint16, 2 * 128 * 128).reshape(2, 128, 128)
        assert np.array_equal(got[0], imgs[0] << 4) and np.array_equal(got[1], imgs[1])
        with pytest.raises(ValueError):
            cct_hip.jpeg2000_decode_batch(mixed + mixed, 128, 128, out_dev=out)  # does not fit
        assert cct_hip.jpeg2000_decode_batch([], 128, 128, out_dev=out) == (0, 128, 128)
    finally:
        out.free()
    low = np.minimum(imgs[:1] >> 4, 255).astype(np.uint8)
    f8 = cct_hip.jpeg2000_encode_batch(low, levels=2, codeblock=32)
    assert np.array_equal(cct_hip.jpeg2000_decode_batch(f8, 128, 128, bits=8), low)
    assert np.array_equal(cct_hip.jpeg2000_decode_batch(f8, 128, 128, bits=16), low)  # 8 bits of precision fit 16 allocated
    empty = cct_hip.jpeg2000_decode_batch([], 4, 4)
    assert empty.shape == (0, 4, 4) and empty.dtype == np.uint16
    res, status = cct_hip.jpeg2000_decode_batch([], 4, 4, bits=8, raise_errors=False)
    assert res.shape == (0, 4, 4) and res.dtype == np.uint8 and status.size == 0
    t = (cct_hip._ffi.C.c_float * 6)()
    cct_hip.jpeg2000_decode_batch(f8, 128, 128, bits=8)
    cct_hip._ffi.lib().cct_last_timings(t)
    assert t[4] > 0  # the decode kernels were timed


def test_device_equals_the_model_on_foreign_and_hand_built_files():
    """No encoder of this project takes part.  The model is run here on the small files; for OpenJPEG's 70 x 130 files, where it takes
    seconds, tests/test_jpeg2000_decode_model.py holds it to the same rasters, which are what Pillow decodes."""
    import cct_hip
    hand = d.handbuilt_set()
    got = cct_hip.jpeg2000_decode_batch([f for _, f, _ in hand], 33, 65)  # 32 x 32 and 8 x 64 code-blocks, 16 and 12 bits in one batch
    for (name, f, want), g in zip(hand, got):
        assert np.array_equal(g, want) and np.array_equal(g, d.decode(f, 33, 65)), name
    img, cases = d.marker_cases()
    res, status = cct_hip.jpeg2000_decode_batch([f for _, f, _ in cases], 9, 11, raise_errors=False)
    for (name, f, want), g, s in zip(cases, res, status):
        assert s == CODES.get(want, 0) and (s or np.array_equal(g, img)), (name, s)
    if not d.pillow_has_jpeg2000():
        return
    fs = d.foreign_set()
    got = cct_hip.jpeg2000_decode_batch([f for _, f, _ in fs[:-1]], 70, 130)  # five codings and both packet sequences in one batch
    for (name, f, want), g in zip(fs[:-1], got):
        assert np.array_equal(g, want), name
    assert np.array_equal(cct_hip.jpeg2000_decode_batch([fs[-1][1]], 70, 130, bits=8)[0], fs[-1][2])
    assert np.array_equal(cct_hip.jpeg2000_decode_batch([fs[3][1]], 70, 130, shift=3)[0], fs[3][2] >> 3)


def test_refusals_per_file():
    import cct_hip
    hand = d.handbuilt_set()
    good, img = hand[0][1], hand[0][2]
    refused = d.refused_set()
    batch = [good] + [x for _, f in refused for x in (f, good)]
    res, status = cct_hip.jpeg2000_decode_batch(batch, 33, 65, raise_errors=False)
    assert list(status) == [0] + [E_J2K, 0] * len(refused), list(status)
    for k in range(0, len(batch), 2):
        assert np.array_equal(res[k], img), k  # the neighbours are decoded
    with pytest.raises(ValueError):
        cct_hip.jpeg2000_decode_batch(batch, 33, 65)
    with pytest.raises(ValueError):
        cct_hip.jpeg2000_decode_batch([refused[-1][1]], 33, 65)  # nothing to send to the device
    # a wrong shape, and 16 bits of precision at 8 bits allocated
    res, status = cct_hip.jpeg2000_decode_batch([good, m.encode(img[:, :64], 16, levels=1), good], 33, 65, raise_errors=False)
    assert list(status) == [0, E_MIXED, 0] and np.array_equal(res[0], img) and np.array_equal(res[2], img)
    low = (img >> 8).astype(np.uint8)
    res, status = cct_hip.jpeg2000_decode_batch([good, m.encode(low, 8, levels=1)], 33, 65, bits=8, raise_errors=False)
    assert list(status) == [E_MIXED, 0] and np.array_equal(res[1], low)
    # a refused file's slot is its own: the rasters on either side in a device buffer are whole
    out = cct_hip.DeviceBuffer(3 * 33 * 65 * 2)
    try:
        out.upload(np.full((3, 33, 65), 0xABCD, np.uint16))
        shape, status = cct_hip.jpeg2000_decode_batch([good, good[:200], good], 33, 65, out_dev=out, raise_errors=False)
        assert shape == (3, 33, 65) and list(status) == [0, E_STREAM, 0]
        got = out.download(np.uint16, 3 * 33 * 65).reshape(3, 33, 65)
        assert np.array_equal(got[0], img) and np.array_equal(got[2], img)
    finally:
        out.free()


def test_refusals_per_call():
    import cct_hip
    L = cct_hip._ffi.lib()
    f = d.handbuilt_set()[0][1]
    offs = np.array([0, len(f)], np.uint64)
    out = np.zeros((33, 65), np.uint16)
    status = np.zeros(1, np.uint32)

    def call(n=1, rows=33, cols=65, bits=16, shift=0, cap=33 * 65):
        return L.cct_j2k_decode_batch(f, offs.ctypes.data, n, rows, cols, bits, shift, out.ctypes.data, 0, cap, status.ctypes.data)
    assert call() == 0 and np.array_equal(out, d.handbuilt_set()[0][2])
    for bad in (dict(rows=0), dict(cols=0), dict(rows=65536), dict(cols=65536), dict(rows=65535, cols=65535), dict(n=-1), dict(bits=12), dict(bits=32),
                dict(shift=-1), dict(shift=16)):
        assert call(**bad) == E_ARG, bad
    assert call(cap=33 * 65 - 1) == E_CAP
    assert call(n=0, cap=0) == 0
    assert L.cct_j2k_decode_batch(None, offs.ctypes.data, 1, 33, 65, 16, 0, out.ctypes.data, 0, 33 * 65, status.ctypes.data) == E_ARG
    for bad in (dict(bits=12), dict(shift=16), dict(shift=-1), dict(rows=0), dict(cols=65536), dict(rows=65535, cols=65535)):
        with pytest.raises(ValueError):
            cct_hip.jpeg2000_decode_batch([f], **{"rows": 33, "cols": 65, **bad})
    for bad in (f, [1], [f, "x"]):
        with pytest.raises(TypeError):
            cct_hip.jpeg2000_decode_batch(bad, 33, 65)
    with pytest.raises(TypeError):
        cct_hip.jpeg2000_decode_batch([f], 33, 65, out_dev=out)
    with pytest.raises(TypeError):
        cct_hip.jpeg2000_decode_batch([f], 33.5, 65)


@pytest.mark.parametrize("base", ("model 33 x 65", "OpenJPEG three layers"))
def test_damaged_files_equal_the_model(base):
    """The damages are jpeg2000_decode_model.DAMAGES: truncation at every structural boundary and inside packet headers, single
    bytes changed in packet headers and in MQ-coded bytes.  The host emulation (tools/debug/j2k_dec_host_emu) ran this set under
    AddressSanitizer and UBSan before it ran here; no fault is expected."""
    import cct_hip
    if base not in {b for b, *_ in d.damaged_set()}:
        needs_pillow()
    want = d.damaged_expected(base)
    assert len(want) == len(d.DAMAGES) >= 40
    res, status = cct_hip.jpeg2000_decode_batch([g for _, g, _ in want], 33, 65, raise_errors=False)
    for (dmg, g, w), r, s in zip(want, res, status):
        if isinstance(w, str):
            assert s == CODES[w], (dmg, s, w)
        else:
            assert s == 0 and np.array_equal(r, w), (dmg, s)
    d_ok = [g for _, g, w in want if not isinstance(w, str)]
    assert np.array_equal(cct_hip.jpeg2000_decode_batch(d_ok, 33, 65), np.stack([w for _, _, w in want if not isinstance(w, str)]))


@functools.lru_cache(maxsize=None)
def real_slices():
    return np.stack([gi.load_slice("slice0671"), gi.load_slice("slice3706")])


def test_real_slices_full_size():
    """512 x 512, where the model is not run: the device decodes the device's files and, where Pillow has the codec, OpenJPEG's
    files of the same slices to the bytes Pillow decodes them to."""
    import cct_hip
    imgs = real_slices()
    for shift, jp2, cb in ((4, True, 64), (0, False, 64), (0, False, 32)):
        files = cct_hip.jpeg2000_encode_batch(imgs, precision=16, shift=shift, jp2=jp2, codeblock=cb)
        assert np.array_equal(cct_hip.jpeg2000_decode_batch(files, 512, 512, shift=shift), imgs)
    if not d.pillow_has_jpeg2000():
        return
    from PIL import Image
    for shift in (0, 4):
        files = [d.openjpeg((x.astype(np.uint32) << shift).astype(np.uint16), no_jp2=bool(shift)) for x in imgs]
        got = cct_hip.jpeg2000_decode_batch(files, 512, 512)
        for f, g, x in zip(files, got, imgs):
            assert g.tobytes() == np.array(Image.open(io.BytesIO(f))).tobytes() and np.array_equal(g >> shift, x)
        assert np.array_equal(cct_hip.jpeg2000_decode_batch(files, 512, 512, shift=shift), imgs)


def test_batches_of_several_passes_equal_single_frames():
    """A file of 512 x 512 holds 10 bytes a sample of planes and raster on the device, its bytes twice (the upload and the
    segments) and some 10 KB of code-block records, tag trees and chunks: 3.0 MB at 185 KB a file, so a pass of 512 MiB
    (csrc/api_jpeg2000.cpp J2K_DEC_PASS_BYTES) takes about 178 files and per_pass + 8 run as two passes."""
    import cct_hip
    two = real_slices()
    files = cct_hip.jpeg2000_encode_batch(two)
    per_pass = (512 << 20) // (10 * 512 * 512 + 2 * max(len(f) for f in files) + 112 * 48 + 4 * 200 + 96)
    assert 150 < per_pass < 200
    n = per_pass + 8
    got = cct_hip.jpeg2000_decode_batch([files[i % 2] for i in range(n)], 512, 512)
    assert all(np.array_equal(got[i], two[i % 2]) for i in range(n))
