"""CPU checks of the zlib strategy surface of the DEFLATE stage: config['encoder']['deflate_strategy'] -> the
CCT_FLAG_DEFLATE_STRATEGY field, refusals before any device call, the header / ABI declarations, and a Python model of
the device's Z_RLE and Z_HUFFMAN_ONLY parse and block split (dfl_rle_rec_kernel, dfl_huff_symbols_kernel, the block count
of dfl_tree_kernel) pinned block by block against the system libz."""
import copy
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import golden_inputs as gi
from deflate_blocks import blocks

Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 0, 1, 2, 3, 4
BLOCK_SYMS = 16383  # lit_bufsize - 1 at memLevel 8


def _cfg(level=None, strategy=None):
    import cct_hip
    cfg = copy.deepcopy(cct_hip.default_config())
    if level is not None:
        cfg["encoder"]["deflate_level"] = level
    if strategy is not None:
        cfg["encoder"]["deflate_strategy"] = strategy
    return cfg


def _libz(data, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(data) + c.flush()


# ------------------------------------------------------------------ surface

def test_zlib_constants_are_the_ones_the_field_carries():
    assert (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED) == (0, 1, 2, 3, 4)


def test_codec_params_maps_deflate_strategy():
    from cct_hip import _ffi, codec_params
    base = codec_params(_cfg())[0]
    assert base & _ffi.FLAG_STRATEGY_MASK == 0  # absent: field 0, the flags every existing caller sends
    for s in range(5):
        flags = codec_params(_cfg(strategy=s))[0]
        assert flags == base | (s << 12) == base | _ffi.flag_deflate_strategy(s)
    assert codec_params(_cfg(6, Z_FILTERED))[0] == base | (6 << 8) | (1 << 12)
    assert codec_params(_cfg(-1, Z_FIXED))[0] == base | (6 << 8) | (4 << 12)
    for level in (1, 2, 3):  # deflate_huff / deflate_rle take every level
        assert codec_params(_cfg(level, Z_RLE))[0] == base | (level << 8) | (3 << 12)
        assert codec_params(_cfg(level, Z_HUFFMAN_ONLY))[0] == base | (level << 8) | (2 << 12)
    assert codec_params(_cfg(strategy=Z_RLE), np.int16)[0] == base | _ffi.FLAG_SIGNED_SEG | (3 << 12)


def test_absent_key_leaves_every_flag_word_unchanged():
    from cct_hip import codec_params
    for level in (None, -1, 4, 9):
        cfg = _cfg(level)
        assert "deflate_strategy" not in cfg["encoder"]
        assert codec_params(cfg)[0] == codec_params(_cfg(level, 0))[0]
        assert codec_params(cfg)[0] >> 12 == 0


BAD_CONFIGS = [  # (level, strategy)
    (None, 5), (None, 7), (None, -1), (None, "3"), (None, 3.0), (None, True), (None, False),
    (0, 0), (0, 2), (0, 3), (1, 0), (2, 1), (3, 4), (1, Z_FIXED), (3, Z_FILTERED), (10, 3), (10, 2), (-2, 3),
]


@pytest.mark.parametrize("level,strategy", BAD_CONFIGS)
def test_bad_strategy_configs_raise_before_the_device(level, strategy):
    import cct_hip
    with pytest.raises(ValueError):
        cct_hip.codec_params(_cfg(level, strategy))
    img = np.zeros((1, 16, 16), dtype=np.uint16)
    with pytest.raises(ValueError):
        cct_hip.encode_batch(img, _cfg(level, strategy))
    if not isinstance(strategy, (str, float, bool)):
        with pytest.raises(ValueError) as e:
            cct_hip.zlib_compress_batch([b"abc"], level=9 if level is None else level, strategy=strategy)
        assert "strategy" in str(e.value)


@pytest.mark.parametrize("level,strategy", [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (3, 1), (2, 4), (10, 3),
                                            (-2, 2), (9, 5), (9, -1), (6, 7), (4, 100)])
def test_new_entry_refuses_without_a_gpu(level, strategy):
    from cct_hip import _ffi
    L = _ffi.lib()
    data = b"abcabcabc"
    offs = np.array([0, len(data)], dtype=np.uint64)
    out = np.zeros(4096, dtype=np.uint8)
    sizes = np.zeros(1, dtype=np.uint32)
    rc = L.cct_zlib_compress_batch_strategy(data, offs.ctypes.data, 1, level, strategy, out.ctypes.data, out.size,
                                            sizes.ctypes.data)
    assert rc == _ffi.E_ARG
    msg = _ffi.last_error()
    assert "strategy" in msg and str(strategy) in msg


@pytest.mark.parametrize("level_field,strategy_field", [(0, 5), (0, 6), (0, 7), (9, 5), (1, 0), (3, 1), (2, 4), (10, 2),
                                                        (15, 3), (1, 1)])
def test_encode_refuses_strategy_fields_without_a_gpu(level_field, strategy_field):
    from cct_hip import _ffi
    L = _ffi.lib()
    img = np.zeros((1, 16, 16), dtype=np.uint16)
    out = np.zeros(1 << 16, dtype=np.uint8)
    sizes, status, psz = (np.zeros(1, dtype=np.uint32) for _ in range(3))
    flags = (_ffi.FLAG_DEFLATE | _ffi.FLAG_FRACTAL | _ffi.FLAG_SEGMENTATION | (level_field << 8)
             | (strategy_field << 12))
    rc = L.cct_encode_batch(img.ctypes.data, 0, 1, 16, 16, 16, flags, -1, b"\0\0\0\0", 1, 2, out.ctypes.data, out.size,
                            sizes.ctypes.data, status.ctypes.data, psz.ctypes.data, None)
    assert rc == _ffi.E_ARG
    assert "strategy" in _ffi.last_error()
    offsets = np.zeros(2, dtype=np.uint64)
    rc = L.cct_encode_batch_packed(img.ctypes.data, 0, 1, 16, 16, 16, flags, -1, b"\0\0\0\0", 1, 2, out.ctypes.data,
                                   out.size, offsets.ctypes.data, sizes.ctypes.data, status.ctypes.data,
                                   psz.ctypes.data, None)
    assert rc == _ffi.E_ARG
    assert "strategy" in _ffi.last_error()


def test_header_declares_the_strategy_surface():
    text = open(os.path.join(gi.ROOT, "include", "compact_hip.h")).read()
    assert re.search(r"#define CCT_FLAG_DEFLATE_STRATEGY\(s\) \(\(\(\(uint32_t\)\(s\)\) & 7u\) << 12\)", text)
    assert re.search(r"#define CCT_FLAG_STRATEGY_MASK 0x7000u", text)
    assert ("int cct_zlib_compress_batch_strategy(const uint8_t *h_in, const uint64_t *h_offsets, int n, int level, "
            "int strategy,") in text
    assert re.search(r"#define CCT_ABI_VERSION 1\b", text)
    from cct_hip import _ffi
    assert _ffi.FLAG_STRATEGY_MASK == 0x7000 and _ffi.FLAG_STRATEGY_MASK & _ffi.FLAG_LEVEL_MASK == 0
    assert "cct_zlib_compress_batch_strategy" in _ffi.exported_symbols()
    assert hasattr(_ffi.lib(), "cct_zlib_compress_batch_strategy")
    restype, argtypes = _ffi._SIGS["cct_zlib_compress_batch_strategy"]
    assert restype == C.c_int and len(argtypes) == 8 and argtypes[3] == argtypes[4] == C.c_int


# ------------------------------------------------------------------ model of the short passes

def _rle_symbols(b):
    """deflate_rle's parse as dfl_rle_rec_kernel restates it: [literal byte] or [-length] (distance 1)"""
    out, p, n = [], 0, len(b)
    while p < n:
        if p > 0 and n - p >= 3 and b[p - 1] == b[p] == b[p + 1] == b[p + 2]:
            r = 3
            while r < 258 and p + r < n and b[p + r] == b[p - 1]:
                r += 1
            out.append(-r)
            p += r
        else:
            out.append(b[p])
            p += 1
    return out


_LBASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224]


def _length_code(lc):
    """trees.c _length_code[length - MIN_MATCH]"""
    if lc == 255:
        return 28
    return max(i for i, b in enumerate(_LBASE) if b <= lc)


def _model_blocks(syms):
    """block split of the short passes: a flush after every 16383 symbols, then the final flush (an empty final block when
    the count is a multiple of 16383) -> [(literal/length histogram, distance histogram)]"""
    nblocks = len(syms) // BLOCK_SYMS + 1
    out = []
    for m in range(nblocks):
        lf, df = [0] * 286, [0] * 30
        for s in syms[m * BLOCK_SYMS:(m + 1) * BLOCK_SYMS]:
            if s >= 0:
                lf[s] += 1
            else:
                lf[257 + _length_code(-s - 3)] += 1
                df[0] += 1
        lf[256] = 1
        out.append((lf, df))
    return out


def _check_against_libz(data, strategy):
    syms = _rle_symbols(data) if strategy == Z_RLE else list(data)
    model = _model_blocks(syms)
    stream = _libz(data, 9, strategy)
    got = blocks(stream)
    assert len(got) == len(model), (len(got), len(model), len(syms))
    for m, ((btype, lf, df, _), (mlf, mdf)) in enumerate(zip(got, model)):
        assert btype in (0, 1, 2)
        if btype:  # a stored block carries no symbols to count
            assert lf == mlf, f"block {m}: literal/length histogram"
            assert df == mdf, f"block {m}: distance histogram"
    return syms, got


def _padded_to(prefix, strategy, target):
    """prefix + literals that never form a run (so each adds exactly one symbol) -> exactly `target` symbols"""
    syms = len(_rle_symbols(prefix)) if strategy == Z_RLE else len(prefix)
    assert syms <= target
    start = (prefix[-1] + 1) % 256 if prefix else 0
    return prefix + bytes((start + i) % 256 for i in range(target - syms))


def _golden_payload(name):
    with open(os.path.join(gi.GOLDEN, name + ".cct"), "rb") as f:
        return zlib.decompress(f.read()[13:])


SMALL = [b"", b"a", b"ab", b"aa", b"aaa", b"aaaa", b"abcd", b"abab", b"aab", b"aaab", b"aaaaaa", b"a" * 600,
         b"q" * 3, b"q" * 257, b"q" * 258, b"q" * 259, b"x" + b"q" * 259, b"xx" + b"q" * 300 + b"y",
         b"zzz" + b"a" * 5, b"a" + b"z" * 4 + b"b", b"ab" + b"z" * 4 + b"c", b"\0" * 1000 + b"\1" * 517]


@pytest.mark.parametrize("strategy", [Z_RLE, Z_HUFFMAN_ONLY])
@pytest.mark.parametrize("i", range(len(SMALL)))
def test_model_blocks_equal_libz_small(strategy, i):
    _check_against_libz(SMALL[i], strategy)


def test_rle_position_one_matches():
    """deflate_rle compares in[0] and in[1] (the hash chains never reach back to position 0): literal + (5, 1), where
    level 9 writes two literals + (4, 1)"""
    assert _rle_symbols(b"aaaaaa") == [ord("a"), -5]
    rle = blocks(_libz(b"aaaaaa", 9, Z_RLE))
    assert rle[0][1][ord("a")] == 1 and rle[0][1][257 + _length_code(5 - 3)] == 1
    l9 = blocks(_libz(b"aaaaaa", 9, Z_DEFAULT_STRATEGY))
    assert l9[0][1][ord("a")] == 2 and l9[0][1][257 + _length_code(4 - 3)] == 1


@pytest.mark.parametrize("strategy", [Z_RLE, Z_HUFFMAN_ONLY])
@pytest.mark.parametrize("name", ["slice0671", "slice3706", "phantom256_s7"])
def test_model_blocks_equal_libz_golden_payloads(strategy, name):
    _check_against_libz(_golden_payload(name), strategy)


@pytest.mark.parametrize("strategy", [Z_RLE, Z_HUFFMAN_ONLY])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_model_block_split_at_multiples_of_16383(strategy, k, delta):
    target = BLOCK_SYMS * k + delta
    prefix = _golden_payload("slice0671")[: BLOCK_SYMS // 2] if strategy == Z_RLE else b""
    data = _padded_to(prefix, strategy, target)
    syms, got = _check_against_libz(data, strategy)
    assert len(syms) == target
    assert len(got) == (k + 1 if delta >= 0 else k)  # 16383 k symbols: an empty final block


@pytest.mark.parametrize("strategy", [Z_RLE, Z_HUFFMAN_ONLY])
def test_short_pass_bytes_do_not_depend_on_the_level(strategy):
    data = _golden_payload("slice0671")[:60000] + b"a" * 600
    want = _libz(data, 9, strategy)
    assert want[:2] == b"\x78\x01"
    for level in range(1, 9):
        assert _libz(data, level, strategy) == want


def test_header_byte_per_strategy():
    data = b"abc" * 100
    assert _libz(data, 9, Z_FIXED)[:2] == b"\x78\x01"
    assert _libz(data, 9, Z_FILTERED)[:2] == b"\x78\xda"
    assert _libz(data, 5, Z_FILTERED)[:2] == b"\x78\x5e"
