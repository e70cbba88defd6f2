"""Device PNG writer (cct_png_encode_batch / png_encode_batch / decode_png_batch) and the memLevel 9 device DEFLATE against
the CPU model of Pillow's PNG (tests/png_model.py) and Python's zlib."""
import copy
import hashlib
import io
import json
import os
import threading
import zlib

import numpy as np
import pytest

import golden_inputs as gi
import png_model as pm

pytestmark = pytest.mark.gpu

LEVELS = [-1, 4, 5, 6, 7, 8, 9]
FIXTURE = json.load(open(os.path.join(gi.GOLDEN, "png.json")))
Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 0, 1, 2, 3, 4
PAIRS = ([(lv, s) for s in (Z_DEFAULT_STRATEGY, Z_FILTERED, Z_FIXED) for lv in (-1, 4, 5, 6, 7, 8, 9)]
         + [(lv, s) for s in (Z_HUFFMAN_ONLY, Z_RLE) for lv in (-1, 1, 2, 3, 4, 5, 6, 7, 8, 9)])


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    cct_hip.device_info()
    return cct_hip


class _option:
    def __init__(self, hip, key, value):
        self.L, self.key, self.value = hip._ffi.lib(), key.encode(), value

    def __enter__(self):
        import ctypes as C
        old = C.c_int(0)
        self.L.cct_get_option(self.key, C.byref(old))
        self.old = old.value
        assert self.L.cct_set_option(self.key, self.value) == 0

    def __exit__(self, *exc):
        self.L.cct_set_option(self.key, self.old)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", sorted(pm.cases()))
def test_png_equals_model_from_the_host(hip, name, level):
    img = pm.cases()[name]
    shift = 4 if level % 2 else 0
    out = hip.png_encode_batch(np.stack([img, img[::-1]]), level=level, shift=shift)
    assert out == [pm.png_bytes(img, level, shift), pm.png_bytes(np.ascontiguousarray(img[::-1]), level, shift)]


@pytest.mark.parametrize("level", [-1, 6, 9])
@pytest.mark.parametrize("name", sorted(pm.cases()))
def test_png_equals_model_from_the_device(hip, name, level):
    img = pm.cases()[name]
    d = hip.DeviceBuffer.from_numpy(img)
    assert hip.png_encode_batch(d, level=level, shift=3, shape=img.shape) == [pm.png_bytes(img, level, 3)]


@pytest.mark.parametrize("level", [4, 6, 9])
@pytest.mark.parametrize("name", ["random", "wide", "odd", "Nx1"])
def test_png_with_host_deflate(hip, name, level):
    img = pm.cases()[name]
    with _option(hip, "device_deflate", 0):
        assert hip.png_encode_batch(img, level=level, shift=1) == [pm.png_bytes(img, level, 1)]


def test_preview_of_slice0671_is_the_reference_file(hip):
    fx = FIXTURE["preview"]
    png = hip.png_encode_batch(gi.load_slice(fx["slice"]), level=fx["level"], shift=fx["shift"])[0]
    assert len(png) == fx["size"] and hashlib.sha256(png).hexdigest() == fx["sha256"]


def test_csv_png_column(hip):
    fx = FIXTURE["csv_png_column"]
    names = sorted(fx["sizes"])
    out = hip.png_encode_batch(np.stack([gi.load_slice(n) for n in names]), level=fx["level"], shift=fx["shift"])
    assert [len(p) for p in out] == [fx["sizes"][n] for n in names]


def test_phantom_batch_of_256(hip):
    from PIL import Image
    imgs = np.stack([gi.ct_phantom(i % 32) for i in range(256)])
    out = hip.png_encode_batch(imgs, level=6, shift=4)
    for i in (0, 1, 77, 255):
        assert out[i] == pm.png_bytes(imgs[i], 6, 4)
    streams = [pm.idat_stream(p) for p in out]
    rows = hip.zlib_decompress_batch(streams, 512 * 1025)
    for i in range(0, 256, 17):
        assert rows[i] == pm.filter_rows(imgs[i], 4)[1]
        back = np.asarray(Image.open(io.BytesIO(out[i])))
        assert np.array_equal(back.astype(np.uint16), pm.samples(imgs[i], 4))


@pytest.mark.parametrize("name", ["slice0671", "slice3706"])
def test_decode_png_batch_equals_the_model(hip, name):
    cfg = hip.default_config()
    with open(os.path.join(gi.GOLDEN, name + ".cct"), "rb") as f:
        cct = f.read()
    pixels = hip.decode_batch([cct], cfg)[0]
    assert np.array_equal(pixels, gi.load_slice(name))
    out = hip.decode_png_batch([cct, cct], cfg)
    assert out == [pm.png_bytes(pixels, 9, 4)] * 2
    if name == FIXTURE["preview"]["slice"]:
        assert hashlib.sha256(out[0]).hexdigest() == FIXTURE["preview"]["sha256"]


def _blobs():
    rng = np.random.default_rng(9)
    rows = pm.filter_rows(gi.load_slice("slice3706"), 4)[1]  # > 32767 symbols at every level
    return [rows, rng.integers(0, 256, 150000, dtype=np.uint8).tobytes(), b"", b"a", b"ab",
            bytes(70000), rows[:40000] + rows[:40000]]


def _libz(data, level, strategy, mem_level):
    c = zlib.compressobj(6 if level == -1 else level, zlib.DEFLATED, 15, mem_level, strategy)
    return c.compress(data) + c.flush()


@pytest.mark.parametrize("level,strategy", PAIRS)
def test_zlib_mem_level_9_equals_libz(hip, level, strategy):
    blobs = _blobs()
    out = hip.zlib_compress_batch(blobs, level=level, strategy=strategy, mem_level=9)
    assert out == [_libz(b, level, strategy, 9) for b in blobs]


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("level,strategy", [(6, Z_FILTERED), (9, Z_DEFAULT_STRATEGY), (4, Z_FIXED), (6, Z_RLE)])
def test_zlib_mem_level_9_on_both_record_settings(hip, compact, level, strategy):
    blobs = _blobs()[:2]
    with _option(hip, "deflate_compact_records", compact):
        out = hip.zlib_compress_batch(blobs, level=level, strategy=strategy, mem_level=9)
    assert out == [_libz(b, level, strategy, 9) for b in blobs]


def test_zlib_mem_level_9_above_4_mib(hip):
    rng = np.random.default_rng(4)
    big = np.repeat(rng.integers(0, 40, 600000, dtype=np.uint8), 8).tobytes()  # 4.8 MB, long runs and chains
    for level, strategy in ((6, Z_FILTERED), (9, Z_DEFAULT_STRATEGY)):
        assert hip.zlib_compress_batch([big], level=level, strategy=strategy, mem_level=9) == \
            [_libz(big, level, strategy, 9)]


def test_mem_level_8_is_what_the_existing_entries_give(hip):
    blobs = _blobs()
    for level, strategy in ((9, 0), (6, 0), (6, Z_FILTERED), (5, Z_RLE)):
        a = hip.zlib_compress_batch(blobs, level=level, strategy=strategy, mem_level=8)
        assert a == hip.zlib_compress_batch(blobs, level=level, strategy=strategy)
        assert a == [_libz(b, level, strategy, 8) for b in blobs]


def test_png_next_to_encode_in_two_threads(hip):
    cfg = copy.deepcopy(hip.default_config())
    cfg["verbose"] = False
    imgs = np.stack([gi.ct_phantom(i) for i in range(8)])
    want_png = [pm.png_bytes(im, 6, 4) for im in imgs]
    want_cct = hip.encode_batch(imgs, cfg)
    errors = []

    def run(k):
        try:
            for _ in range(3):
                if k == 0:
                    assert hip.png_encode_batch(imgs, level=6, shift=4) == want_png
                else:
                    assert hip.encode_batch(imgs, cfg) == want_cct
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=run, args=(k,)) for k in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
