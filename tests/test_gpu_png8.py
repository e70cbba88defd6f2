"""The 8-bit device PNG writer (png_filter8_kernel, cct_png_encode8_batch / png8_encode_batch / decode_png8_batch, the
Decoder's preview_window) against the CPU model of Pillow's 8-bit PNG (tests/png8_model.py), the recorded Pillow files
(tests/golden/png8.json) and Pillow itself where it is installed."""
import hashlib
import json
import os

import numpy as np
import pytest

import golden_inputs as gi
import png8_model as p8
import png_model as pm

pytestmark = pytest.mark.gpu

FIXTURE = json.load(open(os.path.join(gi.GOLDEN, "png8.json")))
NAMES = sorted(p8.cases())
WINDOW = (864, 1264)


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    cct_hip.device_info()
    return cct_hip


@pytest.fixture(scope="module")
def want():
    """(name, level) -> the model's file: computed once, read by every test"""
    return {(n, lv): p8.png8_bytes(p8.samples_of(n), lv) for n in NAMES for lv in p8.LEVELS}


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


def _encode(hip, name, level, on_device=False):
    src, window = p8.cases()[name]
    if on_device:
        return hip.png8_encode_batch(hip.DeviceBuffer.from_numpy(src), window=window, level=level, shape=src.shape,
                                     dtype=src.dtype)
    return hip.png8_encode_batch(src, window=window, level=level)


def test_the_cases_reach_every_filter_type():
    seen = set()
    for name in NAMES:
        seen |= set(p8.filter_rows8(p8.samples_of(name))[0].tolist())
    assert seen == {0, 1, 2, 4}


@pytest.mark.parametrize("level", p8.LEVELS)
@pytest.mark.parametrize("name", NAMES)
def test_png8_equals_model_fixture_and_pillow(hip, want, name, level):
    out = _encode(hip, name, level)
    assert len(out) == 1
    png = out[0]
    fx = FIXTURE["files"][name][str(level)]
    assert png == want[name, level]
    assert len(png) == fx["size"] and hashlib.sha1(png).hexdigest() == fx["sha1"]
    if name in p8.TWO_IDAT:
        assert sum(1 for t, _ in pm.chunks(png) if t == b"IDAT") == 2
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    assert png == p8.pillow8_bytes(p8.samples_of(name), level)


@pytest.mark.parametrize("level", p8.LEVELS)
@pytest.mark.parametrize("name", ["u8_7x129", "u8_noise300x401", "u8_4x520", "u16_3x515", "u16_ramp", "slice0671_w864_1264"])
def test_png8_from_a_device_buffer(hip, want, name, level):
    assert _encode(hip, name, level, on_device=True) == [want[name, level]]


def test_default_level_is_6_and_minus_1_too(hip, want):
    src, _ = p8.cases()["u8_7x129"]
    assert hip.png8_encode_batch(src) == [want["u8_7x129", 6]] == hip.png8_encode_batch(src, level=-1)


@pytest.mark.parametrize("level", p8.LEVELS)
def test_batch_of_three_different_rasters(hip, want, level):
    a = p8.cases()["u8_7x129"][0]
    rng = np.random.default_rng(11)
    batch = np.stack([a, a[::-1], rng.integers(0, 256, a.shape, dtype=np.uint8)])
    assert hip.png8_encode_batch(batch, level=level) == [want["u8_7x129", level]] + [p8.png8_bytes(x, level) for x in batch[1:]]
    r = p8.cases()["u16_ramp"][0]
    batch = np.stack([r, r[::-1], (r.astype(np.uint32) * 3 & 0xFFFF).astype(np.uint16)])
    got = hip.png8_encode_batch(hip.DeviceBuffer.from_numpy(batch), window=(1000, 20000), level=level, shape=batch.shape,
                                dtype=np.uint16)
    assert got == [p8.png8_bytes(p8.window8(x, 1000, 20000), level) for x in batch]


def test_empty_batch(hip):
    assert hip.png8_encode_batch(np.zeros((0, 5, 7), np.uint8)) == []
    assert hip.png8_encode_batch(np.zeros((0, 5, 7), np.uint16), window=(0, 9)) == []
    assert hip.decode_png8_batch([], WINDOW) == []
    L = hip._ffi.lib()
    assert L.cct_png_encode8_batch(None, 0, 0, 5, 7, 8, 0, 255, 6, None, L.cct_png_bound(5, 7), None) == 0


@pytest.mark.parametrize("level", p8.LEVELS)
@pytest.mark.parametrize("name", ["u8_noise300x401", "u8_3x20000", "u8_37x1", "u16_3x515", "slice0671_w0_1600"])
def test_png8_with_host_deflate(hip, want, name, level):
    with _option(hip, "device_deflate", 0):
        assert _encode(hip, name, level) == [want[name, level]]


def test_out_stride_below_the_bound_is_refused(hip):
    L = hip._ffi.lib()
    img, out, sizes = np.zeros((4, 4), np.uint8), np.zeros(1 << 12, np.uint8), np.zeros(1, np.uint32)
    rc = L.cct_png_encode8_batch(img.ctypes.data, 0, 1, 4, 4, 8, 0, 255, 6, out.ctypes.data, L.cct_png_bound(4, 4) - 1,
                                 sizes.ctypes.data)
    assert rc == hip._ffi.E_CAP
    rc = L.cct_png_encode8_batch(img.ctypes.data, 0, 1, 4, 4, 8, 0, 255, 6, out.ctypes.data, L.cct_png_bound(4, 4),
                                 sizes.ctypes.data)
    assert rc == 0 and out[:sizes[0]].tobytes() == p8.png8_bytes(img, 6)


def test_the_reader_returns_the_bytes_written(hip):
    for name in ("u8_noise300x401", "u8_5x65", "u8_3x20000"):
        x8 = p8.cases()[name][0]
        back = hip.png_read_batch(hip.png8_encode_batch(np.stack([x8, x8[::-1]]), level=4))
        assert back.dtype == np.uint16 and np.array_equal(back, np.stack([x8, x8[::-1]]))
    for name in ("u16_ramp", "slice0671_w864_1264", "slice0671_w1000_1001", "u16_3x515"):
        x16, window = p8.cases()[name]
        assert np.array_equal(hip.png_read_batch(hip.png8_encode_batch(x16, window=window, level=4))[0], p8.window8(x16, *window))
    assert hip.png_info(hip.png8_encode_batch(p8.cases()["u8_5x65"][0])[0]) == (5, 65, 8)


def test_pillow_opens_the_files(hip):
    Image = pytest.importorskip("PIL.Image")
    import io
    for name in ("u8_noise300x401", "slice0671_w0_1600"):
        im = Image.open(io.BytesIO(_encode(hip, name, 6)[0]))
        assert im.mode == "L" and np.array_equal(np.asarray(im), p8.samples_of(name))


def test_decode_png8_batch_and_the_16_bit_previews(hip):
    from oracle import oracle
    cfg = hip.default_config()
    files = []
    for name in ("slice0671", "slice3706"):
        with open(os.path.join(gi.GOLDEN, name + ".cct"), "rb") as f:
            files.append(f.read())
    rasters = [np.frombuffer(oracle.decode(f), dtype=np.uint16).reshape(512, 512) for f in files]
    before = hip.decode_png_batch(files, cfg)
    out = hip.decode_png8_batch(files, WINDOW, cfg)
    assert out == [p8.png8_bytes(p8.window8(r, *WINDOW), 6) for r in rasters]
    assert out[0] == p8.png8_bytes(p8.samples_of("slice0671_w864_1264"), 6)
    assert hip.decode_png8_batch(files[:1], list(WINDOW), level=9) == [p8.png8_bytes(p8.window8(rasters[0], *WINDOW), 9)]
    after = hip.decode_png_batch(files, cfg)
    assert before == after == [pm.png_bytes(r, 9, 4) for r in rasters]
    fx = json.load(open(os.path.join(gi.GOLDEN, "png.json")))["preview"]
    assert fx["slice"] == "slice0671" and hashlib.sha256(after[0]).hexdigest() == fx["sha256"]


def test_decoder_preview_window(hip, tmp_path):
    import copy

    from codec.core import Decoder
    with open(os.path.join(gi.GOLDEN, "slice0671.cct"), "rb") as f:
        cct = f.read()
    img = gi.load_slice("slice0671")
    cfg = copy.deepcopy(hip.default_config())
    cfg["verbose"] = False
    cfg["decoder"]["preview_window"] = list(WINDOW)
    png8 = tmp_path / "windowed.png"
    pixels = Decoder(cfg, cct, str(png8)).decode()
    assert np.array_equal(pixels, img)
    assert png8.read_bytes() == p8.png8_bytes(p8.window8(img, *WINDOW), 6)
    assert Decoder(cfg, cct).decode() == img.tobytes()  # no out_path: the window is not used
    del cfg["decoder"]["preview_window"]
    png16 = tmp_path / "plain.png"
    pixels = Decoder(cfg, cct, str(png16)).decode()
    assert np.array_equal(pixels, img)
    depth = pm.chunks(png16.read_bytes())[0][1][8]
    assert depth == 16
    assert np.array_equal(hip.png_read_batch([png16.read_bytes()], shift=4)[0], img)
