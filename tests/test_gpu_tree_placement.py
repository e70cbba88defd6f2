"""dfl_tree_kernel at one and at sixteen waves per workgroup (option tree_waves): byte-identical to zlib through
cct_hip.zlib_compress_batch, on one batch whose slices have 1, 2, 15, 16, 17, 31 and 33 or more DEFLATE blocks, so that its
workgroups have full, partly filled and looping waves side by side.  The block counts are asserted on the host (no GPU), from
zlib's own streams: the coverage cannot be lost silently."""
import functools
import zlib

import numpy as np
import pytest

import deflate_blocks

BLOCK_SYMS = 16383  # symbols per block at memLevel 8 (lit_bufsize - 1)
TARGET_BLOCKS = (1, 2, 15, 16, 17, 31, 33)  # the last one: at least


@functools.lru_cache(maxsize=None)
def _noise(n, seed=5):
    """uniform bytes in 0..47: few matches, every block dynamic"""
    return np.random.default_rng(seed).integers(0, 48, size=n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def _bytes_per_block():
    """input bytes zlib spends on one full block of this noise, counted in its stream: the first three blocks of a sample"""
    sample = _noise(5 * 20000)
    bl = deflate_blocks.blocks(zlib.compress(sample, 9), max_blocks=3)
    assert [b[0] for b in bl] == [2, 2, 2]
    # a literal is one byte; a match's length is not in the histogram, only its code: bound it by the code's base length,
    # 3 + (code - 257) up to code 264 -- the matches of this noise are that short (asserted)
    nbytes = 0
    for _, lf, _, _ in bl:
        assert sum(lf[265:]) == 0
        nbytes += sum(lf[:256]) + sum((3 + k) * lf[257 + k] for k in range(8))
    assert sum(sum(lf) - 1 for _, lf, _, _ in bl) == 3 * BLOCK_SYMS
    return nbytes / 3.0


@functools.lru_cache(maxsize=None)
def _length_for(nblocks):
    """a length whose stream has `nblocks` blocks: the middle of the range of symbol counts that gives that many"""
    return 100 if nblocks == 1 else int((nblocks - 0.5) * _bytes_per_block())


@functools.lru_cache(maxsize=None)
def _blobs():
    return tuple(_noise(_length_for(b), seed=5 + i) for i, b in enumerate(TARGET_BLOCKS))


def _small_blobs(count=40):
    """2 and 3 blocks each, all different"""
    return [_noise(_length_for(2 + i % 2), seed=100 + i) for i in range(count)]


def _libz(data, level=9, strategy=0, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, mem_level, strategy)
    return c.compress(data) + c.flush()


def test_block_counts_of_the_batch():
    """(host) zlib's own streams of the blobs have the block counts the GPU cases are meant to run"""
    counts = [len(deflate_blocks.blocks(zlib.compress(b, 9))) for b in _blobs()]
    assert counts[:-1] == list(TARGET_BLOCKS[:-1]), counts
    assert counts[-1] >= 33, counts
    assert all(t == 2 for b in _blobs() for t in [deflate_blocks.blocks(zlib.compress(b, 9), max_blocks=1)[0][0]])
    assert sum(map(len, _blobs())) < 3 << 20
    small = _small_blobs()
    assert [len(deflate_blocks.blocks(zlib.compress(b, 9))) for b in small] == [2 + i % 2 for i in range(len(small))]
    assert len(set(small)) == len(small)


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    cct_hip.device_info()
    return cct_hip


@pytest.fixture(scope="module")
def expected():
    return [zlib.compress(b, 9) for b in _blobs()]


def _with_tree_waves(waves, fn):
    from cct_hip import _ffi
    L = _ffi.lib()
    _ffi.check(L.cct_set_option(b"tree_waves", waves))
    try:
        return fn()
    finally:
        _ffi.check(L.cct_set_option(b"tree_waves", 0))


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"blob {i}: {len(g)} bytes against zlib's {len(w)}"


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 16])
def test_whole_batch(hip, expected, waves):
    _same(_with_tree_waves(waves, lambda: hip.zlib_compress_batch(list(_blobs()), level=9)), expected)


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 16])
@pytest.mark.parametrize("n", [1, 3, 9])
def test_small_batches(hip, expected, n, waves):
    # 17 blocks first (a second workgroup with one wave), then 1, 16, ...
    order = [4, 0, 3, 1, 2, 5, 6, 0, 1]
    blobs = [_blobs()[i] for i in order[:n]]
    _same(_with_tree_waves(waves, lambda: hip.zlib_compress_batch(blobs, level=9)), [expected[i] for i in order[:n]])


@pytest.mark.gpu
def test_forty_small_blobs_sixteen_forced(hip):
    blobs = _small_blobs()
    _same(_with_tree_waves(16, lambda: hip.zlib_compress_batch(blobs, level=9)), [zlib.compress(b, 9) for b in blobs])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fits one round", "does not fit"])
def test_device_chooses(hip, expected, case):
    """tree_waves 0 with 128 slices or more and at most one per CU: both kernels are launched and the waves choose from the
    slices' block counts.  130 slices of 2 and 3 blocks are 130 workgroups of sixteen: they fit the CUs.  143 slices of one
    block and 57 of 17 blocks (two workgroups each) are 257: they do not fit 256 CUs"""
    if case == "fits one round":
        small = _small_blobs()
        blobs = [small[i % len(small)] for i in range(130)]
        want = [zlib.compress(b, 9) for b in small]
        want = [want[i % len(small)] for i in range(130)]
    else:
        pick = [0] * 143 + [4] * 57
        blobs, want = [_blobs()[i] for i in pick], [expected[i] for i in pick]
    _same(_with_tree_waves(0, lambda: hip.zlib_compress_batch(blobs, level=9)), want)


@pytest.mark.gpu
@pytest.mark.parametrize("strategy,mem_level", [(2, 8), (3, 8), (0, 9)])
def test_short_pass_and_mem_level_9_sixteen_forced(hip, strategy, mem_level):
    blobs = list(_blobs())
    got = _with_tree_waves(16, lambda: hip.zlib_compress_batch(blobs, level=9, strategy=strategy, mem_level=mem_level))
    _same(got, [_libz(b, 9, strategy, mem_level) for b in blobs])


@pytest.mark.gpu
def test_option_values(hip):
    from cct_hip import _ffi
    L = _ffi.lib()
    import ctypes as C
    v = C.c_int(-1)
    try:
        for good in (1, 16, 0):
            assert L.cct_set_option(b"tree_waves", good) == _ffi.OK
            assert L.cct_get_option(b"tree_waves", C.byref(v)) == _ffi.OK and v.value == good
            for bad in (8, 2, 32, -1):
                assert L.cct_set_option(b"tree_waves", bad) == _ffi.E_ARG and "tree_waves" in _ffi.last_error()
                assert L.cct_get_option(b"tree_waves", C.byref(v)) == _ffi.OK and v.value == good
    finally:
        _ffi.check(L.cct_set_option(b"tree_waves", 0))
