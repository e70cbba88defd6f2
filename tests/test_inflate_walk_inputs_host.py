"""The inputs of tests/inflate_walk_inputs.py against CPython's zlib and against their own preconditions.  No device: these are
the premises of tests/test_gpu_inflate_walk_edges.py.  A case zlib disagrees with is a wrong case; a case whose precondition
fails no longer reaches the path it is named for."""
import os
import re

import pytest

import deflate_streams as ds
import golden_inputs as gi
import inflate_walk_inputs as wi

NAMES = [name for name, _ in wi._CASES]
KERNEL = os.path.join(gi.ROOT, "2023-compact-image-compression_amd", "csrc", "inflate_kernels.hip")


@pytest.mark.parametrize("name", NAMES)
def test_zlib_verdict_and_precondition(name):
    c = dict(wi._CASES)[name]()
    out = ds.oracle_verdict(c.stream)
    assert (out is not None) == c.accept, "zlib's verdict"
    w = wi.host_walk(c.stream)
    assert (w["error"] is None) == c.accept, w["error"]
    if c.accept:
        assert w["out"] == out
    print(f"{name}: {'accepted, ' + str(len(out)) + ' bytes' if c.accept else 'refused'}; {c.pre(c.stream)}")


def test_case_list():
    assert len(set(NAMES)) == len(NAMES)
    assert {c.group for c in wi.cases()} == {1, 2, 3, 4, 5, 6}
    assert all(len(c.stream) < 64 * 1024 for c in wi.cases())  # tens of kilobytes at most
    assert all(not c.accept for c in wi.cases(6)) and all(c.accept for c in wi.cases() if c.group != 6)


def test_last_symbol_cases_ask_for_dwords_past_the_stream():
    """group 4: at some fill the two dwords of the pair's general step end past the last byte of the stream, trailer included"""
    reach = []
    for c in wi.cases(4):
        for nt in ds.LANES:
            for align in range(4):
                st = wi.pair_steps(c.stream, nt, align)[0]
                reach.append((st.next + 2) * 4 - (align + len(c.stream)))
    assert max(reach) >= 3 and min(reach) >= -4, (min(reach), max(reach))


def test_wrap_cases_cover_every_alignment():
    """group 5: wherever a stream of the group lies in a batch (offset modulo 16), one of them has a pair whose general step asks
    for the last dword of the staged window and the first, in both geometries"""
    for nt in ds.LANES:
        seen = set()
        for c in wi.cases(5):
            seen |= set(wi.wrap_alignments(c.stream, nt))
        assert seen == set(range(16)), (nt, sorted(seen))


def test_refusals_stand_at_every_fill():
    """group 6: both refusals on entry to the general step with the least fill, with 29 .. 32 valid bits, and with no merge due"""
    for kind in ("distance_too_far_back", "distance_code_without_symbol"):
        group = [c for c in wi.cases(6) if kind in c.name]
        assert len(group) == 32
        for nt in ds.LANES:
            fills = {wi.refusal_fill(c, nt) for c in group}
            assert fills >= {wi.WALK_MIN_BITS, 29, 30, 31, 32} and max(fills) > 32, (kind, nt, sorted(fills))


def test_run_payload_stream():
    pay = bytes([232, 227]) + bytes(40000) + bytes([5])
    stream, check = wi.run_payload_stream(pay)
    check(stream)
    assert ds.oracle_verdict(stream) == pay


def test_constants_equal_the_kernel_source():
    with open(KERNEL) as f:
        src = f.read()
    assert wi.FAST_STEPS == int(re.search(r"#define CCT_INF_FAST_STEPS (\d+)", src).group(1))
    assert ds.SEG_BITS == int(re.search(r"#define CCT_INF_SEG_BITS (\d+)", src).group(1))
    assert ds.LL_BITS == int(re.search(r"#define CCT_INF_LL_BITS (\d+)", src).group(1))
    assert ds.D_BITS == int(re.search(r"\bD_BITS = (\d+);", src).group(1))
    m = re.search(r"INF_IN = LANES >= 512 \? (\d+) : (\d+);", src)
    assert wi.INF_IN == {512: int(m.group(1)), 256: int(m.group(2))}
    assert wi.ROUND_IN_SLACK == int(re.search(r"\bROUND_IN_SLACK = (\d+);", src).group(1))
    assert "WALK_MIN_BITS = 33 - LL_BITS;" in src and wi.WALK_MIN_BITS == 33 - ds.LL_BITS
    assert "LL_SYM_BITS = 15 + 5, D_SYM_BITS = 15 + 13, SYM_BITS = LL_SYM_BITS + D_SYM_BITS;" in src and wi.SYM_BITS == 48
    # the rules device_walk() models, as the kernel states them
    assert src.count("const bool take = lb.cnt <= 32;") == 2                         # a literal-only step and merge()
    assert "const bool two = (e & K_TWO) != 0 && p + l1 < end;" in src
    assert "lb.buf = w >> sh; lb.cnt = 64 - (int)sh; lb.next = idx + 2;" in src
    assert "const bool second = !DIST && L1 && L2 && L1 + L2 <= FB;" in src
    # the staged window holds what the walks read ahead of a round's last segment
    ahead = wi.SYM_BITS - 1 + 64 + 32
    assert "WALK_AHEAD_BITS = SYM_BITS - 1 + 64 + 32;" in src and (ahead + 7) // 8 + 1 <= wi.ROUND_IN_SLACK
