"""The 8-bit PNG model (tests/png8_model.py) against Pillow and the recorded Pillow files (tests/golden/png8.json), the
integer window map at its edges, and the argument checks of the 8-bit device PNG writer, which must refuse before any
device call.  CPU only."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import golden_inputs as gi
import png8_model as p8
import png_model as pm

FIXTURE = json.load(open(os.path.join(gi.GOLDEN, "png8.json")))
NAMES = sorted(p8.cases())


@pytest.fixture(scope="module")
def model_files():
    """(name, level) -> the model's file, built once"""
    return {(n, lv): p8.png8_bytes(p8.samples_of(n), lv) for n in NAMES for lv in p8.LEVELS}


def test_fixture_lists_every_case():
    assert sorted(FIXTURE["files"]) == NAMES and FIXTURE["levels"] == list(p8.LEVELS)


@pytest.mark.parametrize("level", p8.LEVELS)
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_recorded_pillow_file(model_files, name, level):
    fx = FIXTURE["files"][name][str(level)]
    png = model_files[name, level]
    assert len(png) == fx["size"] and hashlib.sha1(png).hexdigest() == fx["sha1"]


@pytest.mark.parametrize("level", p8.LEVELS)
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_pillow(model_files, name, level):
    pytest.importorskip("PIL")
    assert model_files[name, level] == p8.pillow8_bytes(p8.samples_of(name), level)


def test_two_window_cases_write_two_idat_chunks(model_files):
    for name in NAMES:
        for level in p8.LEVELS:
            n_idat = sum(1 for t, _ in pm.chunks(model_files[name, level]) if t == b"IDAT")
            if name in p8.TWO_IDAT:
                assert n_idat == 2, (name, level)
            assert pm.chunks(model_files[name, level])[0][1][8:] == bytes([8, 0, 0, 0, 0])  # depth 8, grayscale


def test_every_filter_type_is_chosen_somewhere():
    seen = set()
    for name in NAMES:
        seen |= set(p8.filter_rows8(p8.samples_of(name))[0].tolist())
    assert seen == {0, 1, 2, 4}


def test_zero_rows_stop_at_none():
    types, rows = p8.filter_rows8(p8.samples_of("u8_zeros16"))
    assert not types.any() and rows == bytes(16 * 17)


def test_window8_edges():
    w8 = lambda v, lo, hi: int(p8.window8(np.array([[v]], np.uint16), lo, hi)[0, 0])  # noqa: E731
    lo, hi = 864, 1264
    assert w8(lo, lo, hi) == 0 and w8(lo - 1, lo, hi) == 0 and w8(0, lo, hi) == 0
    assert w8(lo + 1, lo, hi) == 1  # (510 + 400) // 800
    assert w8(hi, lo, hi) == 255 and w8(hi + 1, lo, hi) == 255 and w8(65535, lo, hi) == 255
    assert w8(hi - 1, lo, hi) == 254  # (399 * 510 + 400) // 800
    assert [w8(v, 1000, 1001) for v in (999, 1000, 1001, 1002)] == [0, 0, 255, 255]  # w = 1
    assert [w8(v, 10, 12) for v in (10, 11, 12)] == [0, 128, 255]  # w = 2: the half rounds up
    assert w8(65535, 0, 65535) == 255 and w8(0, 0, 65535) == 0 and w8(65534, 0, 65535) == 255 and w8(128, 0, 65535) == 0
    assert w8(129, 0, 65535) == 1  # (129 * 510 + 65535) // 131070
    ident = np.arange(256, dtype=np.uint16)[None]
    assert np.array_equal(p8.window8(ident, 0, 255)[0], np.arange(256))
    assert np.array_equal(p8.window8(ident.astype(np.uint8), 0, 255)[0], np.arange(256))


def test_window8_is_rounding_with_halves_up():
    from fractions import Fraction
    rng = np.random.default_rng(5)
    for lo, hi in ((0, 1600), (864, 1264), (0, 65535), (7, 8), (100, 102), (3, 40000)):
        v = np.concatenate([rng.integers(0, 65536, 200), [lo, hi, lo + 1, hi - 1, (lo + hi) // 2]]).astype(np.uint16)
        got = p8.window8(v[None], lo, hi)[0]
        for x, y in zip(v.tolist(), got.tolist()):
            q = Fraction((min(max(x, lo), hi) - lo) * 255, hi - lo)
            assert y == (2 * q.numerator + q.denominator) // (2 * q.denominator)  # floor(q + 1/2)


def test_numerator_of_the_map_stays_below_2_to_25():
    assert 65535 * 510 + 65535 < 1 << 25


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test: the checks run before it is touched."""
    from cct_hip import _ffi

    def boom():
        raise AssertionError("the library was called before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", boom)


U8, U16 = np.zeros((2, 3, 4), np.uint8), np.zeros((2, 3, 4), np.uint16)


@pytest.mark.parametrize("kw", [dict(level=0), dict(level=1), dict(level=3), dict(level=10), dict(level=-2), dict(level=True),
                                dict(level=6.0), dict(window=(0, 255)), dict(window=(3, 9)), dict(shape=(2, 3, 4)),
                                dict(dtype=np.uint8)])
def test_png8_refusals_of_a_uint8_array_before_the_device(no_device, kw):
    import cct_hip
    with pytest.raises((ValueError, TypeError)):
        cct_hip.png8_encode_batch(U8, **kw)


@pytest.mark.parametrize("window", [None, (5, 5), (9, 3), (-1, 100), (0, 65536), (0.0, 100.0), (True, 5), (1, 2, 3), 7, "ab",
                                    (0,), [None, 4]])
def test_png8_refusals_of_windows_before_the_device(no_device, window):
    import cct_hip
    with pytest.raises((ValueError, TypeError)):
        cct_hip.png8_encode_batch(U16, window=window)
    if window is not None:
        with pytest.raises((ValueError, TypeError)):
            cct_hip.decode_png8_batch([b"x"], window)


@pytest.mark.parametrize("arr", [np.zeros((3, 4), np.int16), np.zeros((3, 4), np.int8), np.zeros((3, 4), np.float32),
                                 np.zeros((3, 4), np.uint32), np.zeros((0, 4), np.uint16), np.zeros((3, 0), np.uint16),
                                 np.zeros((2, 0, 5), np.uint16), np.zeros(5, np.uint16), np.zeros((1, 2, 3, 4), np.uint16)])
def test_png8_refuses_bad_rasters_before_the_device(no_device, arr):
    import cct_hip
    with pytest.raises((ValueError, TypeError)):
        cct_hip.png8_encode_batch(arr, window=(0, 100))
    if arr.dtype == np.uint16:
        with pytest.raises((ValueError, TypeError)):
            cct_hip.png8_encode_batch(arr.astype(np.uint8))


def test_png8_refuses_shapes_beyond_one_pass(no_device):
    from cct_hip.batch import _png8_args
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (1, 40000, 30000), (0, 0, 0))
    with pytest.raises(ValueError):
        _png8_args(huge, None, 6, None, None)
    # between the two limits (the C entry takes it): Python sizes the output with cct_png_bound, which has no figure there
    between = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (1, 20000, 30000), (0, 0, 0))
    with pytest.raises(ValueError):
        _png8_args(between, None, 6, None, None)


@pytest.mark.parametrize("kw", [dict(level=3), dict(level=True), dict(level=10)])
def test_decode_png8_batch_refusals_before_the_device(no_device, kw):
    import cct_hip
    with pytest.raises((ValueError, TypeError)):
        cct_hip.decode_png8_batch([b"x"], (864, 1264), **kw)
    with pytest.raises(TypeError):
        cct_hip.decode_png8_batch(b"one file, not a list", (864, 1264))
    with pytest.raises(TypeError):
        cct_hip.decode_png8_batch(["text"], (864, 1264))


def test_device_buffer_arguments_are_checked_before_the_device(no_device):
    import cct_hip
    from cct_hip import batch
    buf = object.__new__(batch.DeviceBuffer)  # no allocation (a null ptr is never freed): the checks look at nbytes alone
    buf.ptr, buf.nbytes = 0, 24
    for kw in (dict(), dict(shape=(2, 3, 4)), dict(dtype=np.uint8), dict(shape=(2, 3, 4), dtype=np.int16),
               dict(shape=(2, 3, 4), dtype="nonsense"), dict(shape=(2, 3, 4), dtype=np.uint16),  # no window
               dict(shape=(2, 3, 4), dtype=np.uint8, window=(0, 255)), dict(shape=(2, 3, 5), dtype=np.uint8),
               dict(shape=(2, 3, 4), dtype=np.uint16, window=(0, 9)),  # 48 bytes
               dict(shape=(3,), dtype=np.uint8), dict(shape=(-1, 3, 4), dtype=np.uint8)):
        with pytest.raises((ValueError, TypeError)):
            cct_hip.png8_encode_batch(buf, **kw)


def test_png_encode_batch_still_refuses_uint8(no_device):
    import cct_hip
    with pytest.raises(TypeError):
        cct_hip.png_encode_batch(np.zeros((3, 4), np.uint8))


def test_decoder_checks_the_preview_window_before_the_device(no_device):
    import cct_hip
    from codec.core import Decoder
    cfg = cct_hip.default_config()
    with open(os.path.join(gi.GOLDEN, "slice0671.cct"), "rb") as f:
        cct = f.read()
    for bad in ((5, 5), (0, 70000), "ab", (1.5, 9)):
        cfg["decoder"]["preview_window"] = bad
        with pytest.raises((ValueError, TypeError)):
            Decoder(cfg, cct, "unused.png").decode()


def test_encode8_refusals_in_the_library():
    from cct_hip import _ffi
    L = _ffi.lib()
    out = np.zeros(1 << 16, np.uint8)
    sizes = np.zeros(1, np.uint32)
    img = np.zeros((4, 4), np.uint16)

    def call(n=1, rows=4, cols=4, src_bits=16, lo=0, hi=100, level=6, stride=out.size):
        return L.cct_png_encode8_batch(img.ctypes.data, 0, n, rows, cols, src_bits, lo, hi, level, out.ctypes.data, stride,
                                       sizes.ctypes.data)
    for kw in (dict(level=0), dict(level=3), dict(level=10), dict(level=-2), dict(src_bits=12), dict(src_bits=0),
               dict(src_bits=32), dict(lo=-1), dict(hi=65536), dict(lo=100, hi=100), dict(lo=101, hi=100),
               dict(src_bits=8), dict(src_bits=8, lo=0, hi=254), dict(src_bits=8, lo=1, hi=255), dict(rows=0), dict(cols=0),
               dict(rows=-3), dict(n=-1), dict(rows=40000, cols=30000), dict(rows=1, cols=(1 << 30) - 512)):
        assert call(**kw) == _ffi.E_ARG, kw
    assert L.cct_png_bound(4, 4) > 0
    assert call(stride=L.cct_png_bound(4, 4) - 1) == _ffi.E_CAP
    # only the 8-bit file of this shape fits one pass: cct_png_bound has no figure, the writer's own bound holds
    assert L.cct_png_bound(20000, 30000) == 0 and call(rows=20000, cols=30000) == _ffi.E_CAP


def test_png_bound_covers_the_8_bit_files():
    from cct_hip import _ffi
    L = _ffi.lib()
    for name in NAMES:
        rows, cols = p8.samples_of(name).shape
        assert L.cct_png_bound(rows, cols) >= max(FIXTURE["files"][name][str(lv)]["size"] for lv in p8.LEVELS)


def test_header_and_binding_agree():
    from cct_hip import _ffi
    import ctypes as C
    text = open(os.path.join(gi.ROOT, "include", "compact_hip.h")).read()
    assert "#define CCT_ABI_VERSION 1" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+cct_png_encode8_batch\s*\(([^)]*)\)\s*;", text)
    assert m, "cct_png_encode8_batch is not declared in include/compact_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const void *images", "int images_on_device", "int n", "int rows", "int cols", "int src_bits", "int lo",
                      "int hi", "int level", "uint8_t *h_out", "size_t out_stride", "uint32_t *h_out_sizes"]
    kinds = [C.c_void_p if "*" in p else C.c_size_t if p.startswith("size_t") else C.c_int for p in params]
    res, args = _ffi._SIGS["cct_png_encode8_batch"]
    assert res is C.c_int and args == kinds
    assert "cct_png_encode8_batch" in _ffi.exported_symbols()
    assert hasattr(_ffi.lib(), "cct_png_encode8_batch")
