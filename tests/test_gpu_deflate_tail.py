"""Head and tail of the device DEFLATE pass against the system zlib, byte for byte: the clear of the output by need
(dfl_clear_kernel), the block histograms of dfl_tree_kernel, the emit kernel's tiles of EMIT_T symbols with several symbols per
lane, the layout kernel and the pack kernels.  What each input is meant to exercise is checked on zlib's own stream first (deflate_blocks), in
tests that need no GPU, so that the coverage cannot be lost without a failure."""
import functools
import zlib

import numpy as np
import pytest

import deflate_blocks as db

Z_HUFFMAN_ONLY, Z_RLE = 2, 3
EMIT_K = 4             # symbols per lane of dfl_emit_kernel
EMIT_T = 256 * EMIT_K  # symbols per iteration of one of its workgroups

FIB = [1, 1]
while len(FIB) < 20:
    FIB.append(FIB[-1] + FIB[-2])


def _libz(data, level=9, strategy=0, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, mem_level, strategy)
    return c.compress(data) + c.flush()


def _shape(stream):
    """[(block type, symbols without END_BLOCK)] of a zlib stream without stored blocks"""
    return [(t, sum(lf) - 1) for t, lf, _, _ in db.blocks(stream)]


def _compare(blobs, level=9, strategy=0, mem_level=8, what=""):
    import cct_hip
    cct_hip.device_info()
    got = cct_hip.zlib_compress_batch(blobs, level=level, strategy=strategy, mem_level=mem_level)
    for i, (b, g) in enumerate(zip(blobs, got)):
        want = _libz(b, level, strategy, mem_level)
        assert g == want, f"{what} blob {i} (len {len(b)}): {len(g)} vs {len(want)} bytes, first diff at " \
                          f"{next((k for k in range(min(len(g), len(want))) if g[k] != want[k]), None)}"


# ---------------------------------------------------------------------------------------------- emit tile edges
# Under Z_HUFFMAN_ONLY every byte is one symbol: block sizes are exact
TILE_LENGTHS_8 = sorted({0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 17407, 32766, 32767}
                        | {k * EMIT_T + d for k in (1, 2, 3, 4, 8, 15, 16, 17) for d in (-1, 0, 1)}
                        | {16383 + k * EMIT_T + d for k in (1, 2) for d in (-2, -1, 0, 1)})
TILE_LENGTHS_9 = sorted({32766, 32767, 32768, 32769, 65534, 65535}
                        | {k * EMIT_T + d for k in (31, 32) for d in (-1, 0, 1)}
                        | {32767 + EMIT_T + d for d in (-2, -1, 0, 1)})


@functools.lru_cache(maxsize=None)
def tile_blobs(mem_level):
    rng = np.random.default_rng(900 + mem_level)
    return [rng.integers(0, 200, n, dtype=np.uint8).tobytes() for n in (TILE_LENGTHS_8 if mem_level == 8 else TILE_LENGTHS_9)]


def test_tile_edge_inputs_have_the_blocks_they_are_meant_to():
    by_len = {len(b): b for b in tile_blobs(8)}
    for n, want in [(16383, [(2, 16383), (1, 0)]), (16384, [(2, 16383), (1, 1)]), (17407, [(2, 16383), (2, 1024)]),
                    (32766, [(2, 16383), (2, 16383), (1, 0)])]:
        assert _shape(_libz(by_len[n], 9, Z_HUFFMAN_ONLY)) == want, n
    by_len = {len(b): b for b in tile_blobs(9)}
    for n, want in [(32767, [(2, 32767), (1, 0)]), (32768, [(2, 32767), (1, 1)]), (32767 + EMIT_T, [(2, 32767), (2, EMIT_T)]),
                    (65534, [(2, 32767), (2, 32767), (1, 0)])]:
        assert _shape(_libz(by_len[n], 9, Z_HUFFMAN_ONLY, 9)) == want, n


@pytest.mark.gpu
@pytest.mark.parametrize("mem_level", [8, 9])
def test_emit_tile_edges(mem_level):
    _compare(list(tile_blobs(mem_level)), 9, Z_HUFFMAN_ONLY, mem_level, f"memLevel {mem_level}")


# ---------------------------------------------------------------------------------------------- longest codes in one lane
def _quad_positions(n):
    """where the four rarest literals go, next to each other: the start, 1020 .. 1024, around every multiple of the tile (the
    last lane of a tile, across the edge, the first lane of the next) and the end"""
    pos = {0, n - 4} | set(range(1020, 1025))
    for k in range(1, n // EMIT_T + 1):
        pos |= {k * EMIT_T - 4, k * EMIT_T - 2, k * EMIT_T}
    return sorted(p for p in pos if 0 <= p <= n - 4)


@functools.lru_cache(maxsize=None)
def long_code_blobs():
    """literal trees deeper than 15 bits (the overflow construction of test_gpu_tree_ties.py); every blob is the same multiset
    of bytes, with one occurrence of each of the four rarest literals adjacent at a chosen offset"""
    rng = np.random.default_rng(31)
    spec = FIB[1:14] + [400] * 32
    values = rng.permutation(256)[:len(spec)]
    rare = [int(v) for v in values[:4]]  # counts 1, 2, 3, 5
    counts = list(spec)
    for k in range(4):
        counts[k] -= 1
    body = np.repeat(values, counts).astype(np.uint8)
    rng.shuffle(body)
    n = len(body) + 4
    quad = np.array(rare, dtype=np.uint8)
    return rare, [np.concatenate([body[:p], quad, body[p:]]).tobytes() for p in _quad_positions(n)]


def test_long_code_inputs_put_the_longest_codes_side_by_side():
    rare, blobs = long_code_blobs()
    assert len(blobs) >= 40 and all(sorted(b) == sorted(blobs[0]) for b in blobs)  # one histogram: one set of code lengths
    (btype, lf, _, llen), = db.blocks(_libz(blobs[0], 9, Z_HUFFMAN_ONLY))
    assert btype == 2 and sum(lf) - 1 == 13785 and db.uncapped_depth(lf) == 17 and max(llen) == 15
    assert sorted(llen[v] for v in rare) == [14, 15, 15, 15]  # 59 bits in one lane
    for p, b in zip(_quad_positions(len(blobs[0])), blobs):
        assert list(b[p:p + 4]) == rare


@pytest.mark.gpu
def test_longest_codes_in_one_lane():
    _compare(long_code_blobs()[1], 9, Z_HUFFMAN_ONLY, 8, "long codes")


# ---------------------------------------------------------------------------------------------- long far matches in a row
@functools.lru_cache(maxsize=None)
def far_match_blob():
    rng = np.random.default_rng(41)
    a = rng.integers(0, 16, 6000, dtype=np.uint8).tobytes()
    mid = rng.integers(0, 16, 20000, dtype=np.uint8).tobytes()
    return a + mid + b"".join(a[250 * i:250 * i + 250] for i in reversed(range(24)))


def test_far_match_input_ends_in_long_far_matches():
    (btype, lf, df, _), = db.blocks(_libz(far_match_blob(), 9))
    # lengths >= 131 (codes >= 277, 5 extra bits) at distances >= 16385 (codes 28 / 29, 13 extra bits): symbols of more than
    # 30 bits each, one after the other
    assert btype == 2 and sum(lf[277:]) >= 24 and df[28] >= 24 and df[29] > 0, (sum(lf[277:]), df[28], df[29])


@pytest.mark.gpu
def test_long_far_matches_in_a_row():
    _compare([far_match_blob()], 9, 0, 8, "far matches")


# ---------------------------------------------------------------------------------------------- histogram extremes
@functools.lru_cache(maxsize=None)
def all_distance_codes_blob():
    """a match of six bytes at the base distance of every distance code, between stretches of random bytes"""
    rng = np.random.default_rng(51)
    data = bytearray(rng.integers(0, 64, 26000, dtype=np.uint8).tobytes())
    base = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
            8193, 12289, 16385, 24577]
    for d in base:
        for _ in range(6):
            data.append(data[len(data) - d])
        data += rng.integers(0, 64, 5, dtype=np.uint8).tobytes()
    return bytes(data)


def equal_counts_blob(literals=256):
    rng = np.random.default_rng(52)
    b = np.repeat(np.arange(literals, dtype=np.uint8), 40)
    rng.shuffle(b)
    return b.tobytes()


def test_histogram_inputs():
    for n, ml in [(16383, 8), (16384, 8), (32767, 9)]:
        (t, lf, _, _), *rest = db.blocks(_libz(b"q" * n, 9, Z_HUFFMAN_ONLY, ml))
        assert lf[ord("q")] == min(n, (1 << (ml + 6)) - 1) and sum(lf) == lf[ord("q")] + 1, (n, ml)  # one counter takes the block
    # 256 equal counts: eight bits each, so zlib stores the block -- after build_tree has seen the counts; 128 give a dynamic one
    assert [t for t, *_ in db.blocks(_libz(equal_counts_blob(), 9, Z_HUFFMAN_ONLY))] == [0]
    (t, lf, _, _), = db.blocks(_libz(equal_counts_blob(128), 9, Z_HUFFMAN_ONLY))
    assert t == 2 and lf[:256] == [40] * 128 + [0] * 128
    (t, lf, df, _), = db.blocks(_libz(b"z" * 70000, 9))
    assert lf[285] > 200 and df[0] == sum(df) and sum(lf[257:285]) <= 1  # length code 285 at distance code 0
    used = [0] * 30
    for t, lf, df, _ in db.blocks(_libz(all_distance_codes_blob(), 9)):
        assert t != 0
        used = [u + d for u, d in zip(used, df)]
    assert all(used), used


@pytest.mark.gpu
def test_histogram_extremes():
    _compare([b"q" * 16383, b"q" * 16384, equal_counts_blob(), equal_counts_blob(128)], 9, Z_HUFFMAN_ONLY, 8, "huffman only")
    _compare([b"q" * 32767, b"q" * 32768], 9, Z_HUFFMAN_ONLY, 9, "huffman only, memLevel 9")
    _compare([b"z" * 70000, all_distance_codes_blob()], 9, 0, 8, "level 9")


# ---------------------------------------------------------------------------------------------- clear by need
@functools.lru_cache(maxsize=None)
def dirty_calls():
    """three calls with the same n and the same longest blob (same strides, same buffers): files that fill the stride, then
    short ones in the same slice positions, then the first again"""
    rng = np.random.default_rng(61)
    full = [rng.integers(0, 256, 70000, dtype=np.uint8).tobytes() for _ in range(6)]
    short = [b"", b"\x07", rng.integers(0, 256, 10, dtype=np.uint8).tobytes(), rng.integers(0, 256, 1000, dtype=np.uint8).tobytes(),
             bytes(70000), full[5]]
    return full, short, full


def test_dirty_workspace_inputs():
    full, short, _ = dirty_calls()
    assert all(len(_libz(b)) == 70031 for b in full)  # 13 bytes more with the file header; zlib's bound is 70034
    assert len(_libz(short[4])) == 91
    assert [len(b) for b in short] == [0, 1, 10, 1000, 70000, 70000]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fork", "no_fork", "rle"])
def test_clear_by_need_on_a_dirty_workspace(mode):
    import cct_hip
    from cct_hip import _ffi
    cct_hip.device_info()
    L = _ffi.lib()
    strategy = Z_RLE if mode == "rle" else 0
    try:
        if mode == "no_fork":
            _ffi.check(L.cct_set_option(b"deflate_fork", 0))
        for k, blobs in enumerate(dirty_calls()):
            _compare(list(blobs), 9, strategy, 8, f"{mode} call {k + 1}")
    finally:
        _ffi.check(L.cct_set_option(b"deflate_fork", 1))


@pytest.mark.gpu
def test_clear_by_need_through_encode_batch():
    """files of noise fill most of the stride; flat images in the same slots afterwards are a few dozen bytes"""
    import cct_hip
    from oracle import oracle
    cct_hip.device_info()
    cfg = cct_hip.default_config()
    cfg["verbose"] = False
    rng = np.random.default_rng(62)
    noise = rng.integers(0, 65536, (6, 64, 64), dtype=np.uint16)
    flat = np.stack([np.full((64, 64), 100 * i, dtype=np.uint16) for i in range(6)])
    for imgs in (noise, flat, noise):
        assert cct_hip.encode_batch(imgs, cfg) == [oracle.encode(im) for im in imgs]


# ---------------------------------------------------------------------------------------------- pack
@functools.lru_cache(maxsize=None)
def _pack_reference(n):
    import cct_hip
    cfg = cct_hip.default_config()
    cfg["verbose"] = False
    rng = np.random.default_rng(70)
    imgs = rng.integers(0, 1 << 12, (300, 32, 32), dtype=np.uint16)[:n]
    # (noise of 12 bits with a random cut per image: the files have many different sizes)
    imgs = np.stack([im >> (i % 7) for i, im in enumerate(imgs)])
    return cfg, imgs, cct_hip.encode_batch(imgs, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 300])
def test_packed_archives(n):
    import cct_hip
    from cct_hip import _ffi
    cct_hip.device_info()
    L = _ffi.lib()
    cfg, imgs, files = _pack_reference(n)
    if n >= 255:  # the exact pack meets every alignment of a destination
        starts = np.cumsum([0] + [len(f) for f in files])[:-1]
        assert len({int(s) % 16 for s in starts}) >= 8 and {int(s) % 4 for s in starts} == {0, 1, 2, 3}
    _, w, h = imgs.shape
    flags, bs, eof, magic, ch, bpc = cct_hip.codec_params(cfg, imgs.dtype)
    total = sum(len(f) for f in files)
    cap = total + 64
    pin = cct_hip.PinnedArray(cap)
    try:
        for arch in (np.zeros(cap, dtype=np.uint8), pin.array):
            arch[:] = 0xA5
            offs = np.zeros(n + 1, dtype=np.uint64)
            sizes, status = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
            _ffi.check(L.cct_encode_batch_packed(imgs.ctypes.data, 0, n, w, h, bs, flags, eof, magic, ch, bpc, arch.ctypes.data,
                                                 cap, offs.ctypes.data, sizes.ctypes.data, status.ctypes.data, None, None))
            assert [int(s) for s in sizes] == [len(f) for f in files] and int(offs[n]) == total
            assert [int(o) for o in offs[:n]] == [int(x) for x in np.cumsum([0] + [len(f) for f in files])[:-1]]
            assert bytes(arch[:total]) == b"".join(files)
    finally:
        pin.free()
