"""The inputs of tests/value_edges.py and the CPU oracle in the value domain tests/test_gpu_value_edges.py relies on: pixel
values on 0x07FF/0x0800, 0x3FFF/0x4000, 0x7FFF/0x8000 and 65535, deltas on the token, segmentation and Q7 thresholds, int16.
The oracle has to reproduce what the reference codec made of every case (tests/golden/value_edges.json, written by
oracle/gen_value_edges_golden.py), and every builder's precondition has to hold.  No device."""
import collections
import hashlib

import numpy as np
import pytest

import golden_inputs as gi
import value_edges as ve
from oracle import oracle

CASES = ve.cases()
NAMES = list(CASES)


def test_every_case_has_its_record():
    """the stored list is the list specs() describes, in its order; what needs no search is stored as described"""
    specs = ve.specs()
    assert [s["name"] for s in specs] == NAMES
    for s in specs:
        stored = CASES[s["name"]]["spec"]
        if s.get("search"):
            assert {k: v for k, v in stored.items() if k in s and k != "search"} == {k: v for k, v in s.items() if k != "search"}
        else:
            assert stored == s
        assert ("sha1" in CASES[s["name"]]) != bool(s.get("no_reference"))


@pytest.mark.parametrize("name", [s["name"] for s in ve.specs() if s.get("search")])
def test_stored_search_results_are_what_the_search_finds(name):
    spec = next(s for s in ve.specs() if s["name"] == name)
    assert ve.resolve(spec) == CASES[name]["spec"]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_reference_record(name):
    """The builder's precondition holds (build asserts it), the image is the one the reference saw, and the oracle gives the
    reference's bytes (length, SHA-1), token counts, jump table and decoder outcome; q7_violations is what the case was designed
    to have."""
    rec = CASES[name]
    spec = rec["spec"]
    bs = spec["bs"]
    img, exp = ve.built(name)
    assert exp == rec["expect"]
    assert str(img.dtype) == rec["dtype"] and list(img.shape) == spec["shape"]
    assert gi.sha1(img.tobytes()) == rec["input_sha1"], "input builder drifted"
    out, st = oracle.encode(img, block_size=bs, deflate=False, return_stats=True)
    assert st.q7_violations == exp["q7"]
    if spec["family"] == "q7":
        assert exp["q7"] == int(ve.violates(spec["delta"]))
    if spec.get("no_reference"):
        return
    assert len(out) == rec["len"] and gi.sha1(out) == rec["sha1"]
    assert (st.n_short, st.n_full, st.n_jump) == (rec["tokens"]["short"], rec["tokens"]["full"], rec["tokens"]["jump"])
    assert st.payload_len == rec["len"] - 13
    an = ve.analyse(img, bs)
    assert gi.sha1(np.array(sorted(an.jumps.items()), dtype=np.int32).tobytes()) == rec["jumps_sha1"]
    try:
        dec = oracle.decode(out, block_size=bs)
    except oracle.OracleError as e:
        assert rec["decode"].get("raises") == {oracle.E_OVERFLOW: "OverflowError"}.get(e.code, "a stream error")
    else:
        assert rec["decode"].get("sha1") == hashlib.sha1(dec).hexdigest()
        assert rec["decode"]["roundtrip"] == (dec == img.tobytes())
    if "deflate" in rec:
        z = oracle.encode(img, block_size=bs, deflate=True)
        assert (len(z), gi.sha1(z)) == (rec["deflate"]["len"], rec["deflate"]["sha1"])


def test_q7_neighbours():
    """every place and regime has its slices with exactly one violation and the neighbouring ones with none"""
    seen = collections.defaultdict(dict)
    for name, rec in CASES.items():
        s = rec["spec"]
        if s["family"] == "q7" and s["shape"] == [128, 128]:
            seen[(s["regime"], s["place"])][s["delta"]] = rec["expect"]["q7"]
    assert len(seen) == 8
    for key, by_delta in seen.items():
        assert by_delta == {-2049: 1, -2048: 1, -2047: 0, 2047: 0, 2048: 0, 2049: 1}, key


def test_the_set_covers_the_ground():
    specs = [r["spec"] for r in CASES.values()]
    assert {s["family"] for s in specs} == {"tok", "q7", "one", "fit", "full"}
    for fam in ("tok", "q7", "fit", "full"):
        sizes = {s["bs"] for s in specs if s["family"] == fam}
        assert sizes >= {16, 32, 64, 12} and (fam == "fit" or sizes >= {4, 5, 8}), (fam, sizes)
        assert {tuple(s["shape"]) for s in specs if s["family"] == fam and s["bs"] == 16} >= {(128, 128), (256, 256), (512, 512), (64, 64), (60, 64), (80, 48)}
    assert {s["bs"] for s in specs if s["family"] == "one"} >= {4, 5, 8, 12, 16, 32, 64}
    ones = [s for s in specs if s["family"] == "one" and "boundary" in s]
    for n in (256, 512):
        for value in ("v11", "v14"):
            got = {(s["place"], s["boundary"]) for s in ones if s["shape"][0] == n and s["value"] == value}
            assert got >= {(p, b) for p in ("pred_pair", "pred_lone") for b in ("tpg1", "tpg2", "tpg4")}
            assert {p for p, _ in got} == {"pred_pair", "pred_lone", "inside", "lookahead", "before"}
    assert {r["dtype"] for r in CASES.values()} == {"uint16", "int16"}
    lo = min(int(ve.built(n)[0].min()) for n in NAMES if CASES[n]["dtype"] == "uint16" and CASES[n]["spec"]["shape"][0] <= 256)
    hi = max(int(ve.built(n)[0].max()) for n in NAMES if CASES[n]["dtype"] == "uint16" and CASES[n]["spec"]["shape"][0] <= 256)
    assert (lo, hi) == (0, 65535)
    # decoder outcomes of both kinds are recorded
    outcomes = collections.Counter("raises" if "raises" in r["decode"] else ("exact" if r["decode"]["roundtrip"] else "garbage")
                                   for r in CASES.values() if "decode" in r)
    assert outcomes["raises"] >= 5 and outcomes["exact"] >= 20, outcomes
