"""The token-stream writer and judge of tests/token_streams.py against the CPU oracle, and the oracle against the
reference's recorded behaviour on hand-built and damaged streams.  No device: these are the preconditions of
tests/test_gpu_token_streams.py, checked where no GPU is involved."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

import golden_inputs as gi
import token_streams as ts
from oracle import oracle


@pytest.mark.parametrize("case", ts.WELL_FORMED, ids=lambda c: f"{c[0]}x{c[1]}-bs{c[2]}-{'fractal' if c[3] else 'raster'}-{c[4]}")
def test_writer_against_oracle(case):
    """oracle.decode(file) == the image the writer says its tokens mean, raw and behind zlib.compress"""
    W, H, bs, fr, plan = case
    blob, img, info = ts.well_formed(case)
    assert img.shape == (W, H) and img.dtype == np.uint16
    fast = ts.classify_fast(blob[13:], W * H, bs)
    assert fast is None
    if W * H <= 16384:
        assert ts.classify(blob[13:], W * H, bs) is None
    assert oracle.decode(blob, block_size=bs) == img.tobytes()
    z = ts.with_deflate(blob)
    assert z[12] == 1 and z[:12] == blob[:12]
    assert oracle.decode(z, block_size=bs) == img.tobytes()
    if plan in ("near", "far", "half") and info["NB"] % 2 == 0 and info["NB"] >= 128:
        assert info["n_jump"] == info["NB"] // 2
    if plan == "jump63" and info["NB"] > 63:
        assert info["slots"][0] == (0, 63)
    if plan == "last":
        assert any(lead + j == info["NB"] - 1 for lead, j in info["slots"] if j)


def test_well_formed_set_reaches_both_ends_of_16_bits():
    lo = min(int(ts.well_formed(c)[1].min()) for c in ts.WELL_FORMED if c[0] * c[1] <= 512 * 512)
    hi = max(int(ts.well_formed(c)[1].max()) for c in ts.WELL_FORMED if c[0] * c[1] <= 512 * 512)
    assert (lo, hi) == (0, 65535)


def test_farthest_partner_plan_fills_the_window():
    """the plan that pairs every block with the farthest free one claims all 63 blocks ahead of a leader at some point
    (the replay's window all ones behind the frontier); the random plan uses jumps of every length up to 63"""
    blob, _, info = ts.well_formed((512, 512, 16, True, "far"))
    jt = ts.jump_table(blob[13:], 512 * 512, 16)
    assert max(len(cl) for _, _, _, cl in jt) >= 62
    assert sum(1 for _, _, j, _ in jt if j == 63) > 8000
    blob, _, info = ts.well_formed((512, 512, 16, True, "rand"))
    jt = ts.jump_table(blob[13:], 512 * 512, 16)
    assert info["n_jump"] > 2048 and {j for _, _, j, _ in jt} == set(range(1, 64))


def test_steered_jump_bytes_stand_on_the_boundaries():
    """the bases of the damaged sets carry a jump byte at b-1 or b of the segment boundary and of a step boundary of every
    workgroup size their payload reaches; block sizes below 16 reach offset 15"""
    rng = np.random.default_rng(3)
    blob, img = ts.build(128, 128, 4, True, "p50", rng, jump_at=[15, 4096, 8191, 16384])
    pay = blob[13:]
    assert all((pay[t] & 0xC0) == 0x80 for t in (15, 4096, 8191, 16384))
    assert oracle.decode(blob, block_size=4) == img.tobytes()
    blob, img = ts.build(128, 128, 16, True, "p50", rng, jump_at=[16, 4095, 8192, 16383])
    assert oracle.decode(blob, block_size=16) == img.tobytes()


def _verdicts(W, H, bs):
    out = []
    for name, tag, f, base in ts.damaged_set(W, H, bs):
        c = ts.classify_fast(f[13:], W * H, bs, base)
        if W * H <= 16384:  # the 30-line judge and its fast forms agree
            assert ts.classify(f[13:], W * H, bs) == c == ts.classify_fast(f[13:], W * H, bs), (name, tag)
        out.append((name, tag, c, ts.oracle_verdict(f, bs)[0]))
    return out


def test_judge_against_oracle_and_balance_of_the_damaged_set():
    """A stream the judge calls well formed never gets E_STREAM from the oracle: it gets pixels or E_OVERFLOW.  And the
    damaged set is not lopsided: every defect name at least 20 times, well-formed/pixels and well-formed/overflow at least 200
    each, no class above 80 % of the set."""
    allv = [v for shp in ts.DAMAGED_SHAPES for v in _verdicts(*shp)]
    wrong = [(name, tag) for name, tag, c, o in allv if c is None and o == "stream"]
    assert not wrong, wrong[:10]
    by_defect = collections.Counter(c for _, _, c, _ in allv)
    classes = collections.Counter((c, o) for _, _, c, o in allv)
    print(sorted(classes.items(), key=lambda kv: -kv[1]))
    for d in ts.DEFECTS:
        assert by_defect[d] >= 20, (d, by_defect)
    assert classes[(None, "pixels")] >= 200 and classes[(None, "overflow")] >= 200, classes
    assert max(classes.values()) <= 0.8 * len(allv), classes
    # appended tokens behind pixel N-1 do not exist for the decoder: those files are well formed and decode
    app = [(c, o) for name, _, c, o in allv if name == "append"]
    assert len(app) >= 50 and all(c is None and o == "pixels" for c, o in app)
    # the aimed edits did supply the classes that bit flips do not
    aimed = collections.Counter(c for name, _, c, _ in allv if name.startswith("aim_"))
    assert aimed["two_jumps"] >= 10 and aimed["truncated"] >= 10, aimed


with open(os.path.join(gi.GOLDEN, "token_streams.json")) as _f:
    RECORDS = json.load(_f)["records"]
STREAM_EXCEPTIONS = ("TypeError", "IndexError", "ValueError")  # what the device contract maps to CorruptStreamError


@pytest.mark.parametrize("rec", RECORDS, ids=lambda r: r["file"][:-4])
def test_oracle_equals_reference_record(rec):
    """tests/golden/token_streams.json holds what the reference's Decoder did with each file (oracle/gen_token_stream_golden.py):
    the oracle returns the same raster, E_OVERFLOW where it raised OverflowError, E_STREAM where it raised one of the
    exceptions of a stream it cannot read.  Every exception recorded for a stream the judge calls malformed is one the
    device contract maps to CorruptStreamError or OverflowError."""
    with open(os.path.join(gi.GOLDEN, "token_streams", rec["file"]), "rb") as f:
        blob = f.read()
    assert len(blob) == rec["len"]
    bs = rec["block_size"]
    W, H = (blob[4] << 8) | blob[5], (blob[6] << 8) | blob[7]
    if not blob[12]:
        assert ts.classify(blob[13:], W * H, bs) == rec["judge"]
    verdict, raster = ts.oracle_verdict(blob, bs)
    if "sha1" in rec:
        assert verdict == "pixels" and hashlib.sha1(raster).hexdigest() == rec["sha1"]
    elif rec["raises"] == "OverflowError":
        assert verdict == "overflow"
    else:
        assert rec["raises"] in STREAM_EXCEPTIONS and verdict == "stream"
    if rec["judge"] is not None and "raises" in rec:
        assert rec["raises"] in STREAM_EXCEPTIONS + ("OverflowError",)
    if rec["judge"] is None:
        assert "sha1" in rec or rec["raises"] == "OverflowError"


def test_records_cover_the_ground():
    judged = collections.Counter(r["judge"] for r in RECORDS)
    assert all(judged[d] >= 2 for d in ts.DEFECTS), judged
    assert {r["block_size"] for r in RECORDS} == {4, 5, 16}
    assert sum(1 for r in RECORDS if r.get("raises") == "OverflowError") >= 3
    assert sum(1 for r in RECORDS if "sha1" in r) >= 10
