"""Device DEFLATE at zlib levels 4 to 9 (and -1 = 6): byte-identical to zlib.compress(data, level) through the batch
entry, the encoder flag field and the Encoder's config['encoder']['deflate_level']; files of any level decode."""
import copy
import ctypes as C
import zlib

import numpy as np
import pytest

import golden_inputs as gi
from test_deflate_level_model import CORPUS

pytestmark = pytest.mark.gpu

LEVELS = [-1, 4, 5, 6, 7, 8, 9]
# the ZIP column of results/encoder-comparisons.csv: zlib.compress(image.tobytes()) of the raw slice (level 6)
ZIP_BYTES = {"slice0671": 270969, "slice3706": 273262}


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    cct_hip.device_info()
    return cct_hip


def _cfg(hip, level=None):
    cfg = copy.deepcopy(hip.default_config())
    cfg["verbose"] = False
    if level is not None:
        cfg["encoder"]["deflate_level"] = level
    return cfg


def _first_diff(a, b):
    return next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), None)


@pytest.mark.parametrize("level", LEVELS)
def test_batch_equals_zlib_at_every_level(hip, level):
    blobs = [x for _, x in CORPUS]  # one batch of mixed sizes, 0 to 512 KiB
    got = hip.zlib_compress_batch(blobs, level=level)
    for (name, b), g in zip(CORPUS, got):
        want = zlib.compress(b, level)
        assert g == want, f"{name} level {level}: {len(g)} vs {len(want)} bytes, first diff at {_first_diff(g, want)}"


def test_level9_through_the_new_entry_equals_the_old_entry(hip):
    from cct_hip import _ffi
    L = _ffi.lib()
    blobs = [x for _, x in CORPUS[:20]] + [CORPUS[-3][1]]
    offs = np.zeros(len(blobs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in blobs], out=offs[1:])
    data = b"".join(blobs)
    stride = (13 + max(len(b) for b in blobs) * 2 + 4096 + 63) & ~63
    outs, sizes = [], []
    for fn, extra in ((L.cct_zlib_compress_batch, ()), (L.cct_zlib_compress_batch_level, (9,))):
        out = np.zeros((len(blobs), stride), dtype=np.uint8)
        sz = np.zeros(len(blobs), dtype=np.uint32)
        _ffi.check(fn(data, offs.ctypes.data, len(blobs), *extra, out.ctypes.data, stride, sz.ctypes.data))
        outs.append([out[i, : sz[i]].tobytes() for i in range(len(blobs))])
    assert outs[0] == outs[1]
    assert outs[0] == [zlib.compress(b, 9) for b in blobs]


def test_zip_column_of_the_real_slices(hip):
    raws = [gi.load_slice(name).tobytes() for name in ZIP_BYTES]
    got = hip.zlib_compress_batch(raws, level=-1)
    assert [len(g) for g in got] == list(ZIP_BYTES.values())
    assert got == [zlib.compress(r) for r in raws]


def _images():
    return np.stack([gi.load_slice("slice0671"), gi.load_slice("slice3706"), gi.ct_phantom(7), gi.ct_phantom(11)])


@pytest.mark.parametrize("level", LEVELS[:-1])
def test_encode_batch_and_encoder_at_a_level(hip, level):
    from codec.core import Encoder
    imgs = _images()
    ref9 = hip.encode_batch(imgs, _cfg(hip))
    got = hip.encode_batch(imgs, _cfg(hip, level))
    for f9, f in zip(ref9, got):
        assert f[:13] == f9[:13]
        assert f[13:] == zlib.compress(zlib.decompress(f9[13:]), level)
    assert Encoder(_cfg(hip, level), imgs[0]).encode() == got[0]
    assert Encoder(_cfg(hip, 9), imgs[0]).encode() == ref9[0]


def test_decode_batch_of_mixed_levels(hip):
    from codec.core import Decoder
    imgs = _images()
    files = [hip.encode_batch(imgs[i: i + 1], _cfg(hip, lv))[0] for i, lv in enumerate([4, 6, None, 8])]
    assert len({f[14] for f in files}) == 3  # 5E, 9C, DA: the level shows in the zlib header only
    assert np.array_equal(hip.decode_batch(files, _cfg(hip)), imgs)
    assert Decoder(_cfg(hip), files[0]).decode() == imgs[0].tobytes()


@pytest.mark.parametrize("option", ["device_deflate", "deflate_graph", "deflate_fork", "deflate_compact_records"])
def test_same_bytes_on_every_path(hip, option):
    from cct_hip import _ffi
    L = _ffi.lib()
    imgs = _images()[:3]
    blobs = [x for name, x in CORPUS if "nice" in name or "payload" in name]
    old = C.c_int(0)
    _ffi.check(L.cct_get_option(option.encode(), C.byref(old)))
    try:
        for level in (4, 6, 8):
            want_files = [f[:13] + zlib.compress(zlib.decompress(f[13:]), level) for f in hip.encode_batch(imgs, _cfg(hip))]
            for value in (0, 1):
                _ffi.check(L.cct_set_option(option.encode(), value))
                assert hip.encode_batch(imgs, _cfg(hip, level)) == want_files, (option, value, level)
                if option != "device_deflate":
                    assert hip.zlib_compress_batch(blobs, level=level) == [zlib.compress(b, level) for b in blobs]
    finally:
        _ffi.check(L.cct_set_option(option.encode(), old.value))
