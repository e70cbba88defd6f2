"""Device DEFLATE on inputs whose Huffman trees stress the heap replay of dfl_tree_kernel: many equal frequencies (ties
are decided by heap position) and literal/length trees deeper than 15 bits (gen_bitlen's overflow repair walks the heap
tail that the replay wrote).  What each input is meant to exercise is checked on zlib's own stream first, so that the
coverage cannot be lost without a failure."""
import zlib

import numpy as np
import pytest

import deflate_blocks as db

FIB = [1, 1]
while len(FIB) < 20:
    FIB.append(FIB[-1] + FIB[-2])


def _counts(rng, spec):
    """a histogram over random byte values: spec = list of counts"""
    c = np.zeros(256, dtype=np.int64)
    c[rng.permutation(256)[:len(spec)]] = spec
    return c


def tie_blobs():
    """dynamic blocks whose literal histograms are full of equal counts (no match: the histogram is exactly the spec)"""
    rng = np.random.default_rng(11)
    specs = [
        [200] * 64,                                    # all equal
        [300, 700] * 32,                               # two values
        [1 << min(i // 3, 9) for i in range(48)],       # geometric, three of each
        [20 + 10 * (i // 2) for i in range(64)],       # equal pairs
        [1] * 40 + [150] * 60,                         # many ones next to a flat block
    ]
    blobs = [db.no_match_bytes(_counts(rng, s), rng) for s in specs]
    blobs.append(rng.integers(0, 2, 50000, dtype=np.uint8).tobytes())  # two symbols: ties among lengths and distances
    blobs.append(rng.integers(0, 4, 70000, dtype=np.uint8).tobytes())
    return blobs


def overflow_blobs():
    """literal/length trees deeper than MAX_BITS: a Fibonacci chain (END_BLOCK is its first 1) below a flat block"""
    out = []
    for seed, (nflat, flat, nchain) in enumerate([(32, 400, 14), (32, 400, 14), (48, 250, 14), (64, 200, 13)]):
        rng = np.random.default_rng(200 + seed)
        out.append(db.no_match_bytes(_counts(rng, FIB[1:nchain] + [flat] * nflat), rng))
    return out


def test_tie_inputs_give_dynamic_blocks():
    for i, b in enumerate(tie_blobs()):
        types = [t for t, *_ in db.blocks(zlib.compress(b, 9))]
        assert types and all(t == 2 for t in types), f"tie blob {i}: block types {types}"


def test_overflow_inputs_overflow():
    for i, b in enumerate(overflow_blobs()):
        (btype, lf, _, llen), = db.blocks(zlib.compress(b, 9))
        assert btype == 2 and db.uncapped_depth(lf) > 15 and max(llen) == 15, f"overflow blob {i}"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ties", "overflow"])
def test_device_deflate_matches_zlib(kind):
    import cct_hip
    cct_hip.device_info()
    blobs = tie_blobs() if kind == "ties" else overflow_blobs()
    got = cct_hip.zlib_compress_batch(blobs)
    for i, (b, g) in enumerate(zip(blobs, got)):
        want = zlib.compress(b, 9)
        assert g == want, f"{kind} blob {i} (len {len(b)}): {len(g)} vs {len(want)} bytes"
