"""The inputs of tests/deflate_match_queue_inputs.py do what they claim, without a GPU: every position is classified by the two
queueing rules of dfl_match_kernel, in the (hash, position) order in which the kernel's waves take them."""
import pytest

import deflate_match_inputs as dmi
import deflate_match_queue_inputs as qi


def test_queue_heavy_is_runs_of_20_to_60_with_a_new_byte_each():
    d = qi.queue_heavy(50000)
    runs, p = [], 0
    while p < len(d) - 16:
        e = p
        while e < len(d) - 16 and d[e] == d[p]:
            e += 1
        runs.append(e - p); p = e
    assert all(20 <= r <= 60 for r in runs[:-1]) and 1 <= runs[-1] <= 60  # (the last one is cut by the length)
    assert max(runs) < qi.NICE[9]


def test_share_of_queued_positions_in_queue_heavy():
    """level 9: every position of a run but its last two, that is 1 - 2 / (mean run length 40) of all; level 4 (nice_match 16):
    a run's first position, and those with 15 .. 3 equal bytes ahead, 14 of 40"""
    d = qi.queue_heavy(200000)
    assert qi.share(d, 9, 2) == pytest.approx(1 - 2 / 40, abs=0.005)
    assert qi.share(d, 4, 2) == pytest.approx(14 / 40, abs=0.005)
    assert qi.share(d, 9, 1) < 0.005  # a few strings across two runs that share a bucket


def test_share_of_queued_positions_in_heavy_chain():
    """one position in five starts a trigram, and all of them have 13 earlier ones in the window after the first 13 * 160 bytes"""
    d = qi.heavy_chain(40000)
    assert qi.share(d, 9, 2) == 0 and qi.share(d, 4, 2) == 0
    assert qi.share(d, 9, 1) == pytest.approx(0.2 * (1 - 13 * 160 / 40000), abs=0.005)


@pytest.mark.parametrize("level", [4, 9])
def test_matches_stay_short(level):
    """no run reaches nice_match at level 9 and a trigram's matches have three or four bytes: no chain walk ends early, which is
    what makes the model of the queues exact"""
    assert max(ln for _, ln, _ in dmi.libz_tokens(qi.heavy_chain(40000), level).toks) <= 4
    assert max(ln for _, ln, _ in dmi.libz_tokens(qi.queue_heavy(50000), 9).toks) < qi.NICE[9]  # (a match may run on into the next run)


def test_mix_has_both_kinds():
    d = qi.mix(100000)
    assert 0.4 < qi.share(d, 9, 2) < 0.6 and 0.05 < qi.share(d, 9, 1) < 0.15


def test_some_wave_exceeds_its_region():
    """the long slices: consecutive turns of one wave queue more than a region holds, so the wave flushes in mid-loop: with
    compact records at both levels and on both ends of the grid's range, with wide records (2048 workgroups per slice) in the
    slice made for them"""
    b = qi.batches()
    d, m, w = b["long_and_short"][0], b["many"][57], qi.wide_long()[0]
    n9, n61, longest61 = len(b["long_and_short"]), len(b["many"]), max(map(len, b["many"]))
    for data, level, parts in ((d, 4, qi.nparts(len(d), n9)), (d, 9, qi.nparts(len(d), n9)), (m, 4, qi.nparts(longest61, n61)),
                               (m, 9, qi.nparts(longest61, n61)), (w, 9, qi.nparts(len(w), 1, False))):
        fills, mid = qi.wave_fills(data, level, parts)
        assert mid > 0, (len(data), level, parts)
        assert max(f for _, f, _ in fills) <= qi.REGION
    # the long slice at level 9: a wave makes 16 turns or more of about 55 run positions, so it flushes several times
    parts = qi.nparts(len(d), n9)
    fills, mid = qi.wave_fills(d, 9, parts)
    _, kind = qi.kinds(d, 9)
    assert -(-len(kind) // (parts * qi.BLOCK)) >= 16 and (kind == 2).sum() / (4 * parts) > 2 * qi.REGION and mid > 2 * 4 * parts


def test_flush_boundaries_are_hit():
    """each boundary size: some wave's run list holds exactly one entry less than the flush threshold, the threshold itself (64
    entries stay free: no flush) and one more (flush) after a turn that is not its last"""
    batch = qi.batches()["boundaries"]
    parts = qi.nparts(max(map(len, batch)), len(batch))
    for n in qi.BOUNDARY_SIZES:
        fills, mid = qi.wave_fills(qi.mix(n, qi.BOUNDARY_SHARE), 9, parts)
        seen = {f for k, f, more in fills if k == 2 and more}
        assert {qi.FLUSH_ABOVE - 1, qi.FLUSH_ABOVE, qi.FLUSH_ABOVE + 1} <= seen
        assert mid > 0


def test_slice_lengths_sit_on_the_grid():
    b = qi.batches()
    assert sorted(len(v) for v in b.values()) == [1, 7, 9, 9, 61]
    assert [len(x) for x in b["long_and_short"][4:]] == [0, 3, 65, 66, 67]          # npos 0, 1, 63, 64, 65
    assert [len(x) for x in b["short"][:2]] == [1, 2]
    longest = max(map(len, b["long_and_short"]))
    assert qi.nparts(longest, 9, False) == qi.GRID_WIDE and qi.nparts(longest, 9) == qi.GRID_COMPACT // 2
    assert [len(x) - 2 - qi.nparts(longest, 9, False) * qi.BLOCK for x in b["long_and_short"][1:4]] == [-1, 0, 1]
    longest = max(map(len, b["boundaries"]))
    assert qi.nparts(longest, 7) == qi.GRID_COMPACT
    assert [len(x) - 2 - qi.nparts(longest, 7) * qi.BLOCK for x in b["boundaries"][:3]] == [-1, 0, 1]
    longest = max(map(len, b["many"]))
    assert qi.nparts(longest, 61) == qi.GRID_COMPACT_MIN
    assert [len(x) - 2 - qi.nparts(longest, 61) * qi.BLOCK for x in b["many"][58:]] == [-1, 0, 1]
    assert qi.nparts(max(map(len, b["short"])), 9) < qi.GRID_COMPACT // 2  # fewer workgroups than the cap: one turn each
