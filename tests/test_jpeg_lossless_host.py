"""JPEG Lossless without a GPU: tests/jpeg_lossless_model.py against libjpeg-turbo (through Pillow) at precision 8, its own
round trip at precisions 12 and 16, the two known answers, and the host's marker walk (cct_jpegll_info and the refusals
cct_jpegll_decode_batch decides before it needs a device) against the model's for every damaged file."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import jpeg_lossless_model as m

E_STREAM, E_CAP, E_ARG, E_MIXED, E_JPEG = 4, 6, 9, 10, 13
KNOWN = ("ffd8ffc3000b100001000801011100ffc4001700010101010000000000000000000000001001020fffda00080101000100004a77ff00f6bfffd9")
SHAPES = ((1, 1), (1, 7), (5, 1), (19, 23), (64, 64))


@pytest.mark.parametrize("shape", SHAPES)
def test_model_files_open_in_pillow(shape):
    if not m.pillow_opens_sof3():
        pytest.skip("this Pillow's libjpeg does not open SOF3")
    from PIL import Image
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    smooth = (128 + 60 * np.sin(np.arange(shape[0])[:, None] / 4.0) * np.cos(np.arange(shape[1])[None] / 3.0)).astype(np.uint8)
    for img in (rng.integers(0, 256, shape).astype(np.uint8), smooth):
        for ss in range(1, 8):
            for pt in (0, 2):
                for rr in (0, 1, 2, 3):
                    f = m.encode_frame(img, 8, ss, pt, rr)
                    want = (img >> pt) << pt
                    assert np.array_equal(np.array(Image.open(io.BytesIO(f))), want), (ss, pt, rr)
                    assert np.array_equal(m.decode_frame(f, *shape, bits=8), want), (ss, pt, rr)
                    assert m.info(f) == (*shape, 8)


@pytest.mark.parametrize("precision", [12, 16])
def test_model_round_trips(precision):
    rng = np.random.default_rng(precision)
    for shape in SHAPES:
        for name, img in m.raster_cases(*shape, precision, np.uint16).items():
            for ss, pt, rr in ((1, 0, 0), (1, 0, 2), (4, 0, 1), (5, 2, 0), (6, 0, 3), (7, 1, 2), (2, 0, 0), (3, 3, 1)):
                f = m.encode_frame(img, precision, ss, pt, rr)
                assert np.array_equal(m.decode_frame(f, *shape), (img >> pt) << pt), (shape, name, ss, pt, rr)
        img = rng.integers(0, 1 << precision, shape).astype(np.uint16)
        f = m.encode_frame(img, precision, table=m.FLAT5, pre_segments=[m.segment(0xE0, b"JFIF\0"), m.segment(0xFE, b"hello")])
        assert np.array_equal(m.decode_frame(f, *shape), img)


def test_known_answers():
    img = np.array([[0, 65535, 0, 32768, 0, 32767, 65535, 1]], dtype=np.uint16)
    f = m.encode_frame(img, 16)
    assert f.hex() == KNOWN
    assert np.array_equal(m.decode_frame(f, 1, 8), img)
    bits, vals = m.huffman_table(m.FIB)  # unrestricted lengths reach 17: Figure K.3 runs
    assert bits == [1] * 14 + [0, 3] and vals == list(range(16, -1, -1))
    fib = m.fibonacci_raster()
    assert fib.shape == (1, 6763)
    cat, _ = m.categories(m.differences(fib, 16)[0])
    assert tuple(np.bincount(cat.ravel(), minlength=17)) == m.FIB
    f = m.encode_frame(fib, 16)
    at = f.index(b"\xff\xc4")
    assert f[at + 5:at + 21] == bytes(bits) and f[at + 21:at + 38] == bytes(vals)
    assert np.array_equal(m.decode_frame(f, 1, 6763), fib)


@functools.lru_cache(maxsize=None)
def damaged():
    img = np.random.default_rng(3).integers(0, 4096, (5, 37)).astype(np.uint16)
    return img, m.damaged_files(img, 12)


def test_model_refuses_every_damaged_file():
    img, files = damaged()
    assert len(files) >= 35
    for name, (f, kind) in files.items():
        with pytest.raises(m.JpegError) as e:
            m.decode_frame(f, 5, 37, 16)
        assert e.value.kind == kind, name
    with pytest.raises(m.JpegError) as e:
        m.decode_frame(m.encode_frame(img, 12), 5, 37, 8)  # the precision does not fit 8 bits
    assert e.value.kind == "MIXED"


def test_info_matches_the_model():
    import cct_hip
    from cct_hip import _ffi
    img, files = damaged()
    for p, dt in ((8, np.uint8), (12, np.uint16), (16, np.uint16)):
        for ss, pt, rr in ((1, 0, 0), (7, 2, 1)):
            f = m.encode_frame(img.astype(dt) if p > 8 else (img >> 4).astype(dt), p, ss, pt, rr,
                               pre_segments=[m.segment(0xE1, b"x" * 300), m.segment(0xFE, b"")])
            assert cct_hip.jpeg_lossless_info(f) == (5, 37, p) == m.info(f)
            assert cct_hip.jpeg_lossless_info(f + b"\0") == (5, 37, p)  # the pad byte of a DICOM fragment
    for name, (f, kind) in files.items():
        if kind == "JPEG":
            with pytest.raises(ValueError):
                cct_hip.jpeg_lossless_info(f)
            r, c, p = C.c_int(), C.c_int(), C.c_int()
            assert _ffi.lib().cct_jpegll_info(f, len(f), C.byref(r), C.byref(c), C.byref(p)) == E_JPEG, name
            assert b"not a JPEG" in _ffi.lib().cct_last_error()
        else:
            assert cct_hip.jpeg_lossless_info(f) == m.info(f), name  # the walk takes it; the shape or the data is wrong
    with pytest.raises(TypeError):
        cct_hip.jpeg_lossless_info("file.jpg")


def test_host_parser_refuses_before_it_needs_a_device():
    """a batch in which the marker walk refuses every file returns the statuses without a device"""
    import cct_hip
    img, files = damaged()
    batch = [(name, f, E_JPEG if kind == "JPEG" else E_MIXED) for name, (f, kind) in files.items() if kind in ("JPEG", "MIXED")]
    for bits in (16, 8):
        if bits == 8:  # every file of precision 12 is refused now, whatever else is wrong with its data
            batch += [(name, f, E_MIXED) for name, (f, kind) in files.items() if kind == "STREAM"]
            batch.append(("precision_above_bits", m.encode_frame(img, 12), E_MIXED))
        res, status = cct_hip.jpeg_lossless_decode_batch([f for _, f, _ in batch], 5, 37, bits=bits, raise_errors=False)
        assert res.shape == (len(batch), 5, 37)
        for (name, _, want), s in zip(batch, status):
            assert s == want, (name, bits)
    with pytest.raises(ValueError):
        cct_hip.jpeg_lossless_decode_batch([files["no_soi"][0]], 5, 37)


def test_arguments_are_checked_before_any_device_call():
    import cct_hip
    L = cct_hip._ffi.lib()
    img = np.zeros((4, 4), np.uint16)
    with pytest.raises(TypeError):
        cct_hip.jpeg_lossless_encode_batch(img.astype(np.int16))
    with pytest.raises(TypeError):
        cct_hip.jpeg_lossless_encode_batch(img, precision=12.0)
    for kw in ({"precision": 1}, {"precision": 17}, {"restart_rows": -1}, {"shape": (4, 4)}):
        with pytest.raises(ValueError):
            cct_hip.jpeg_lossless_encode_batch(img, **kw)
    with pytest.raises(ValueError):
        cct_hip.jpeg_lossless_encode_batch(img.astype(np.uint8), precision=9)
    with pytest.raises(ValueError):
        cct_hip.jpeg_lossless_encode_batch(np.zeros((3, 2, 40000), np.uint8), restart_rows=2)  # Ri > 65535
    with pytest.raises(ValueError):
        cct_hip.jpeg_lossless_encode_batch(np.zeros((2, 2, 2, 2), np.uint8))
    assert cct_hip.jpeg_lossless_encode_batch(np.zeros((0, 4, 4), np.uint8)) == []
    with pytest.raises(TypeError):
        cct_hip.jpeg_lossless_decode_batch(b"one file", 4, 4)
    with pytest.raises(TypeError):
        cct_hip.jpeg_lossless_decode_batch([b""], 4.0, 4)
    with pytest.raises(ValueError):
        cct_hip.jpeg_lossless_decode_batch([b""], 4, 4, bits=12)
    with pytest.raises(ValueError):
        cct_hip.jpeg_lossless_decode_batch([b""], 0, 4)
    assert cct_hip.jpeg_lossless_decode_batch([], 4, 4).shape == (0, 4, 4)
    # the C ABI: the bound and its refusals
    assert L.cct_jpegll_bound(512, 512, 0) == 72 + 2 * ((31 * 512 * 512 + 7) // 8) + 2
    assert L.cct_jpegll_bound(5, 7, 2) == 72 + 3 * (2 * ((31 * 14 + 7) // 8) + 2)
    assert L.cct_jpegll_bound(0, 7, 0) == 0 and L.cct_jpegll_bound(4, 40000, 2) == 0 and L.cct_jpegll_bound(70000, 1, 0) == 0
    out = np.zeros(16, np.uint8)
    sizes, status = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    args = (out.ctypes.data, out.size, sizes.ctypes.data, status.ctypes.data)
    assert L.cct_jpegll_encode_batch(img.ctypes.data, 0, 1, 4, 4, 16, 16, 0, *args) == E_CAP
    assert L.cct_jpegll_encode_batch(img.ctypes.data, 0, 1, 4, 4, 12, 12, 0, *args) == E_ARG
    assert L.cct_jpegll_encode_batch(img.ctypes.data, 0, 1, 4, 4, 8, 9, 0, *args) == E_ARG
    assert L.cct_jpegll_encode_batch(img.ctypes.data, 0, -1, 4, 4, 16, 16, 0, *args) == E_ARG
    assert cct_hip._ffi.E_JPEG == E_JPEG and L.cct_version() == 1
