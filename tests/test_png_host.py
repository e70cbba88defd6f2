"""The PNG model (tests/png_model.py) against Pillow and the reference's recorded PNGs, and the argument checks of the
device PNG writer and of zlib_compress_batch(mem_level=...), which must refuse before any device call.  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest

import golden_inputs as gi
import png_model as pm

FIXTURE = json.load(open(os.path.join(gi.GOLDEN, "png.json")))


@pytest.mark.parametrize("level", [4, 5, 6, 7, 8, 9])
@pytest.mark.parametrize("name", sorted(pm.cases()))
def test_model_equals_pillow(name, level):
    img = pm.cases()[name]
    for shift in (0, 4):
        assert pm.png_bytes(img, level, shift) == pm.pillow_bytes(img, level, shift)


@pytest.mark.parametrize("level", [4, 6, 9])
@pytest.mark.parametrize("name", ["slice0671", "slice3706"])
def test_model_equals_pillow_on_the_slices(name, level):
    img = gi.load_slice(name)
    png = pm.png_bytes(img, level, 4)
    assert png == pm.pillow_bytes(img, level, 4)
    assert len(pm.zlib_stream(pm.filter_rows(img, 4)[1], level)) > 16383  # more than one memLevel-8 block


def test_wide_rows_take_chunks_of_four_bytes_per_column():
    img = pm.cases()["wide"]
    sizes = [len(d) for t, d in pm.chunks(pm.pillow_bytes(img, 6)) if t == b"IDAT"]
    assert len(sizes) == 2 and sizes[0] == 4 * img.shape[1]


def test_model_reproduces_the_reference_preview():
    fx = FIXTURE["preview"]
    png = pm.png_bytes(gi.load_slice(fx["slice"]), fx["level"], fx["shift"])
    assert len(png) == fx["size"]
    assert hashlib.sha256(png).hexdigest() == fx["sha256"]


def test_model_reproduces_the_csv_png_column():
    fx = FIXTURE["csv_png_column"]
    for name, size in fx["sizes"].items():
        assert len(pm.png_bytes(gi.load_slice(name), fx["level"], fx["shift"])) == size


def test_memlevel_9_differs_from_8_on_the_slices():
    import zlib
    rows = pm.filter_rows(gi.load_slice("slice0671"), 4)[1]
    for level in range(4, 10):
        c8 = zlib.compressobj(level, zlib.DEFLATED, 15, 8, pm.Z_FILTERED)
        assert c8.compress(rows) + c8.flush() != pm.zlib_stream(rows, level)


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test: the checks run before it is touched."""
    from cct_hip import _ffi

    def boom():
        raise AssertionError("the library was called before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", boom)


@pytest.mark.parametrize("kw", [dict(level=0), dict(level=1), dict(level=2), dict(level=3), dict(level=10),
                                dict(level=-2), dict(level=True), dict(level=6.0), dict(shift=16), dict(shift=-1),
                                dict(shift=True)])
def test_png_refusals_before_the_device(no_device, kw):
    import cct_hip
    with pytest.raises((ValueError, TypeError)):
        cct_hip.png_encode_batch(np.zeros((2, 3, 4), np.uint16), **kw)


@pytest.mark.parametrize("arr", [np.zeros((3, 4), np.int16), np.zeros((3, 4), np.uint8), np.zeros((3, 4), np.float32),
                                 np.zeros((0, 4), np.uint16), np.zeros((3, 0), np.uint16), np.zeros((2, 0, 5), np.uint16),
                                 np.zeros(5, np.uint16), np.zeros((1, 2, 3, 4), np.uint16)])
def test_png_refuses_bad_rasters_before_the_device(no_device, arr):
    import cct_hip
    with pytest.raises((ValueError, TypeError)):
        cct_hip.png_encode_batch(arr)


def test_png_refuses_shapes_beyond_one_pass(no_device):
    import cct_hip
    from cct_hip.batch import _png_args
    with pytest.raises(ValueError):
        _png_args(np.lib.stride_tricks.as_strided(np.zeros(1, np.uint16), (1, 20000, 30000), (0, 0, 0)), 6, 0, None)
    with pytest.raises(ValueError):
        cct_hip.decode_png_batch([b"x"], level=3)


@pytest.mark.parametrize("mem_level", [7, 10, 0, True, 8.0, "9"])
def test_zlib_mem_level_refusals_before_the_device(no_device, mem_level):
    import cct_hip
    with pytest.raises(ValueError):
        cct_hip.zlib_compress_batch([b"abc"], level=6, strategy=1, mem_level=mem_level)


def test_png_bound_and_refusals_in_the_library():
    from cct_hip import _ffi
    L = _ffi.lib()
    assert L.cct_png_bound(0, 5) == 0 and L.cct_png_bound(5, 0) == 0
    assert L.cct_png_bound(512, 512) >= len(pm.pillow_bytes(pm.cases()["random"], 9))
    out = np.zeros(1 << 16, np.uint8)
    sizes = np.zeros(1, np.uint32)
    img = np.zeros((4, 4), np.uint16)
    for level, shift, rows, cols in ((3, 0, 4, 4), (0, 0, 4, 4), (10, 0, 4, 4), (6, 16, 4, 4), (6, -1, 4, 4), (6, 0, 0, 4),
                                     (6, 0, 4, 0), (6, 0, 20000, 30000)):
        rc = L.cct_png_encode_batch(img.ctypes.data, 0, 1, rows, cols, shift, level, out.ctypes.data, out.size,
                                    sizes.ctypes.data)
        assert rc == _ffi.E_ARG, (level, shift, rows, cols)
    for ml in (7, 10):
        rc = L.cct_zlib_compress_batch_params(b"abc", np.array([0, 3], np.uint64).ctypes.data, 1, 6, 0, ml,
                                              out.ctypes.data, out.size, sizes.ctypes.data)
        assert rc == _ffi.E_ARG
