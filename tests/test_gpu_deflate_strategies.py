"""Device DEFLATE at every zlib strategy: byte-identical to zlib.compressobj(level, DEFLATED, 15, 8, strategy) through the
batch entry, the encoder flag field, the packed encode and the Encoder's config['encoder']['deflate_strategy'], on every
DEFLATE path option; files of every strategy decode on the device and through zlib."""
import copy
import ctypes as C
import threading
import zlib

import numpy as np
import pytest

import golden_inputs as gi
from test_deflate_level_model import CORPUS

pytestmark = pytest.mark.gpu

Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 0, 1, 2, 3, 4
PAIRS = ([(lv, s) for s in (Z_FILTERED, Z_FIXED) for lv in (-1, 4, 5, 6, 7, 8, 9)]
         + [(lv, s) for s in (Z_HUFFMAN_ONLY, Z_RLE) for lv in (-1, 1, 2, 3, 4, 5, 6, 7, 8, 9)])


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    cct_hip.device_info()
    return cct_hip


@pytest.fixture(scope="module")
def phantom_payloads(hip):
    """256 token payloads of 512x512 phantoms (the bench workload), without DEFLATE"""
    cfg = _cfg(hip)
    cfg["encoder"]["deflate_compression"] = False
    imgs = np.stack([gi.ct_phantom(i) for i in range(16)])
    payloads = [f[13:] for f in hip.encode_batch(imgs, cfg)]
    return [payloads[i % 16] for i in range(256)]


def _cfg(hip, level=None, strategy=None):
    cfg = copy.deepcopy(hip.default_config())
    cfg["verbose"] = False
    if level is not None:
        cfg["encoder"]["deflate_level"] = level
    if strategy is not None:
        cfg["encoder"]["deflate_strategy"] = strategy
    return cfg


def _libz(data, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(data) + c.flush()


def _first_diff(a, b):
    return next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), None)


def _edge_blobs():
    """run starts at 0 / 1 / 2, runs around MAX_MATCH, and symbol counts at and around multiples of 16383"""
    out = [b"", b"a", b"ab", b"aaa", b"aaaa", b"aaaaaa", b"a" * 600, b"xa" + b"a" * 300, b"xya" + b"a" * 300,
           b"q" * 257, b"q" * 258, b"q" * 259, b"\0" * 1000 + b"\1" * 517]
    for k in (1, 2):
        for d in (-1, 0, 1):
            n = 16383 * k + d
            out.append(bytes(i % 256 for i in range(n)))  # no run: n symbols under every strategy
    return out


@pytest.mark.parametrize("level,strategy", PAIRS)
def test_batch_equals_libz_on_the_corpus(hip, level, strategy):
    blobs = [x for _, x in CORPUS] + _edge_blobs()
    names = [n for n, _ in CORPUS] + [f"edge{i}" for i in range(len(_edge_blobs()))]
    got = hip.zlib_compress_batch(blobs, level=level, strategy=strategy)
    for name, b, g in zip(names, blobs, got):
        want = _libz(b, level, strategy)
        assert g == want, f"{name} ({level}, {strategy}): {len(g)} vs {len(want)} bytes, first diff at {_first_diff(g, want)}"


@pytest.mark.parametrize("level,strategy", [(9, Z_FILTERED), (6, Z_FILTERED), (9, Z_FIXED), (4, Z_FIXED),
                                            (9, Z_HUFFMAN_ONLY), (1, Z_HUFFMAN_ONLY), (9, Z_RLE), (2, Z_RLE)])
def test_batch_equals_libz_on_phantom_payloads(hip, phantom_payloads, level, strategy):
    got = hip.zlib_compress_batch(phantom_payloads, level=level, strategy=strategy)
    want = {}
    for i, (b, g) in enumerate(zip(phantom_payloads, got)):
        if i % 16 not in want:
            want[i % 16] = _libz(b, level, strategy)
        assert g == want[i % 16], f"payload {i}: first diff at {_first_diff(g, want[i % 16])}"


def test_strategy_0_equals_the_level_entry(hip):
    from cct_hip import _ffi
    L = _ffi.lib()
    blobs = [x for _, x in CORPUS[:20]] + [CORPUS[-3][1]]
    offs = np.zeros(len(blobs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in blobs], out=offs[1:])
    data = b"".join(blobs)
    stride = (13 + max(len(b) for b in blobs) * 2 + 4096 + 63) & ~63
    for level in (6, 9):
        outs = []
        for fn, extra in ((L.cct_zlib_compress_batch_level, (level,)), (L.cct_zlib_compress_batch_strategy, (level, 0))):
            out = np.zeros((len(blobs), stride), dtype=np.uint8)
            sz = np.zeros(len(blobs), dtype=np.uint32)
            _ffi.check(fn(data, offs.ctypes.data, len(blobs), *extra, out.ctypes.data, stride, sz.ctypes.data))
            outs.append([out[i, : sz[i]].tobytes() for i in range(len(blobs))])
        assert outs[0] == outs[1] == [zlib.compress(b, level) for b in blobs]


def test_alternating_strategies_on_one_slot(hip):
    """the graph cache keys on DeflateArgs: a pass never replays another strategy's graph"""
    blobs = [x for name, x in CORPUS if "payload" in name or "runs_nice" in name or "run2" in name]
    for strategy in (Z_DEFAULT_STRATEGY, Z_RLE, Z_FILTERED, Z_DEFAULT_STRATEGY, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED,
                     Z_DEFAULT_STRATEGY):
        got = hip.zlib_compress_batch(blobs, level=9, strategy=strategy)
        assert got == [_libz(b, 9, strategy) for b in blobs], strategy


def _images():
    return np.stack([gi.load_slice("slice0671"), gi.load_slice("slice3706"), gi.ct_phantom(7), gi.ct_phantom(11)])


@pytest.mark.parametrize("option", [None, "device_deflate", "deflate_fork", "deflate_graph"])
def test_files_equal_header_plus_libz_on_every_path(hip, option):
    from cct_hip import _ffi
    from codec.core import Encoder
    L = _ffi.lib()
    imgs = _images()
    ref = hip.encode_batch(imgs, _cfg(hip))
    payloads = [zlib.decompress(f[13:]) for f in ref]
    old = C.c_int(0)
    if option:
        _ffi.check(L.cct_get_option(option.encode(), C.byref(old)))
    try:
        for value in ((0, 1) if option else (None,)):
            if option:
                _ffi.check(L.cct_set_option(option.encode(), value))
            for level, strategy in ((9, Z_RLE), (3, Z_RLE), (9, Z_HUFFMAN_ONLY), (6, Z_FILTERED), (9, Z_FIXED),
                                    (9, Z_DEFAULT_STRATEGY)):
                want = [f[:13] + _libz(p, level, strategy) for f, p in zip(ref, payloads)]
                got = hip.encode_batch(imgs, _cfg(hip, level, strategy))
                assert got == want, (option, value, level, strategy)
                if option is None:
                    assert Encoder(_cfg(hip, level, strategy), imgs[0]).encode() == want[0]
            # the strategy flag without a level key: field 0 = level 9
            assert hip.encode_batch(imgs[:2], _cfg(hip, None, Z_RLE)) == [f[:13] + _libz(p, 9, Z_RLE)
                                                                          for f, p in zip(ref[:2], payloads[:2])]
    finally:
        if option:
            _ffi.check(L.cct_set_option(option.encode(), old.value))


def _packed(hip, imgs, flags):
    from cct_hip import _ffi
    L = _ffi.lib()
    n, h, w = imgs.shape
    imgs = np.ascontiguousarray(imgs)
    cap = n * (13 + 4 * h * w + 4096)
    out = np.zeros(cap, dtype=np.uint8)
    sizes, status, psz = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    offsets = np.zeros(n + 1, dtype=np.uint64)
    cfg = _cfg(hip)
    _, bs, eof, magic, ch, bpc = hip.codec_params(cfg)
    _ffi.check(L.cct_encode_batch_packed(imgs.ctypes.data, 0, n, w, h, bs, flags, eof, magic, ch, bpc, out.ctypes.data,
                                         cap, offsets.ctypes.data, sizes.ctypes.data, status.ctypes.data,
                                         psz.ctypes.data, None))
    return [out[offsets[i]:offsets[i + 1]].tobytes() for i in range(n)]


def test_packed_encode_with_rle_two_threads(hip):
    imgs = _images()
    ref = hip.encode_batch(imgs, _cfg(hip))
    want = [f[:13] + _libz(zlib.decompress(f[13:]), 9, Z_RLE) for f in ref]
    flags = hip.codec_params(_cfg(hip, None, Z_RLE))[0]
    results, errors = {}, []

    def run(k):
        try:
            for r in range(3):
                results[(k, r)] = _packed(hip, imgs, flags)
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(e)
    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 6
    for v in results.values():
        assert v == want


def test_every_strategy_decodes(hip):
    from codec.core import Decoder
    imgs = _images()
    files = []
    for i, (level, strategy) in enumerate([(9, Z_RLE), (1, Z_HUFFMAN_ONLY), (5, Z_FILTERED), (9, Z_FIXED)]):
        f = hip.encode_batch(imgs[i: i + 1], _cfg(hip, level, strategy))[0]
        assert zlib.decompress(f[13:]) == zlib.decompress(hip.encode_batch(imgs[i: i + 1], _cfg(hip))[0][13:])
        files.append(f)
    assert np.array_equal(hip.decode_batch(files, _cfg(hip)), imgs)
    for f, img in zip(files, imgs):
        assert Decoder(_cfg(hip), f).decode() == img.tobytes()
