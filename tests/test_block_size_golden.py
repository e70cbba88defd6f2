"""Block sizes that are not powers of two (3 to 64): the CPU oracle against the reference-generated fixtures of
tests/golden/block_sizes.json (tools/gen_block_size_golden.py), and the division by a run-time block size that
decode_kernel<0> uses (bs_divider, csrc/cct_internal.h)."""
import json
import os

import numpy as np
import pytest

import block_size_inputs as bsi
import golden_inputs as gi
from oracle import oracle

with open(os.path.join(gi.GOLDEN, "block_sizes.json")) as _f:
    _MAN = json.load(_f)
CASES = {c["name"]: c for c in _MAN["cases"]}


def oracle_args(case):
    o = case["config"]
    return dict(block_size=o["block_size"], fractal=o.get("fractal", True), segmentation=o.get("segmentation", True),
                deflate=o.get("deflate", True))


def jumps_sha1(jumps):
    return gi.sha1(np.array(sorted(jumps.items()), dtype=np.int32).reshape(-1, 2).tobytes())


def test_fixtures_cover_the_issue():
    sizes = {c["config"]["block_size"] for c in CASES.values()}
    assert sizes >= {3, 5, 6, 10, 12, 15, 20, 24, 25, 30, 40, 48, 50, 60}
    assert not sizes & {1, 2, 4, 8, 16, 32, 64}
    meshed = {c["config"]["block_size"] for c in CASES.values() if c["tokens"].get("jump", 0) >= 100 and c["config"]["block_size"] < 16}
    assert len(meshed) >= 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_encodes_like_the_reference(name):
    case = CASES[name]
    img = bsi.build_input(case["input"])
    assert gi.sha1(img.tobytes()) == case["input_sha1"], "input generator drifted"
    out, st = oracle.encode(img, return_stats=True, **oracle_args(case))
    assert len(out) == case["len"] and gi.sha1(out) == case["sha1"]
    if "file" in case:
        with open(os.path.join(gi.GOLDEN, case["file"]), "rb") as f:
            assert out == f.read()
    assert (st.n_short, st.n_full) == (case["tokens"]["short"], case["tokens"]["full"])
    if "jump" in case["tokens"]:
        assert st.n_jump == case["tokens"]["jump"]
        w, h = img.shape
        order = oracle.curve(w, h) if oracle_args(case)["fractal"] else np.arange(w * h, dtype=np.int32)
        data = img.reshape(-1)[order].astype(np.int32)
        _, jumps = oracle.partition(data, order, case["config"]["block_size"])
        assert len(jumps) == case["tokens"]["jump"]
        assert jumps_sha1(jumps) == case["jumps_sha1"]
    dec = oracle.decode(out, block_size=case["config"]["block_size"])
    assert gi.sha1(dec) == case["decoded_sha1"] and dec == img.tobytes()


def bs_divider(d):
    """Python mirror of bs_divider (csrc/cct_internal.h): ord // d == (ord * mul >> 32) >> shift for ord < 2^31."""
    shift = (d - 1).bit_length() - 1
    return -(-(1 << (32 + shift)) // d), shift


def umulhi_div(x, d):
    mul, shift = bs_divider(d)
    return ((x.astype(np.uint64) * np.uint64(mul)) >> np.uint64(32 + shift)).astype(np.int64)


@pytest.mark.parametrize("d", range(3, 65))
def test_run_time_block_size_division(d):
    mul, shift = bs_divider(d)
    assert 0 < mul < 1 << 32 and 0 <= shift <= 5
    # boundary values: every remainder next to 0, next to 2^30 (check_shape's limit on a slice) and next to 2^31 (the
    # proven range), the multiples of d and their neighbours up there, and a seeded sample in between
    near = [np.arange(0, 4 * d), np.arange((1 << 30) - 4 * d, (1 << 30) + 4 * d), np.arange((1 << 31) - 4 * d, 1 << 31)]
    q = np.arange((1 << 30) // d - 2, (1 << 31) // d + 1, max(1, (1 << 31) // d // 4096), dtype=np.int64)
    mults = [q * d - 1, q * d, q * d + d - 1]
    rnd = [np.random.default_rng(d).integers(0, 1 << 31, 100000)]
    x = np.concatenate(near + mults + rnd).astype(np.int64)
    x = x[(x >= 0) & (x < (1 << 31))]
    assert np.array_equal(umulhi_div(x, d), x // d)

