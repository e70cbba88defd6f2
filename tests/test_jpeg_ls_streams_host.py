"""The placed and damaged JPEG-LS files of tests/jpeg_ls_streams.py, without a device: the placements are where the module
says, and the model's verdicts come in the numbers the set was built for."""
import collections

import numpy as np

import jpeg_ls_model as m
import jpeg_ls_streams as s


def test_placements_are_where_they_should_be():
    covered = set()
    for name, x, f in s._placed():
        a, b = s.scan_of(f)[0]
        for o in map(int, name[3:].split("+")):
            assert f[a + o] == 0xFF and f[a + o + 1] < 0x80, name
            covered.add(o)
    assert covered == set(s.WANTED)
    ends = {name: [f[b - 2:b] == b"\xff\x00" for a, b in s.scan_of(f)] for name, x, f in s._end_ff()}
    assert ends["end_ff_last"][-1] and any(ends["end_ff_inner"][:-1])
    for name, x, f in s._lse():
        assert b"\xff\xf8\x00\x0d\x01" in f[:40], name
    assert m.parse(dict((n, f) for n, _, f in s._lse())["lse_maxval1000"])["params"].range == 1001


def test_placement_rasters_are_the_files():
    for name, x, p, rr, f in s.placement_rasters():
        assert m.encode_frame(x, p, rr) == f, name


def test_verdict_counts():
    v = s.verdicts()
    assert len(s.placement_files()) == 51 and len(s.damage_files()) == 122
    assert all(v[e[0]][0] == 0 and v[e[0]][1].shape == e[2:4] for e in s.placement_files())
    assert collections.Counter(k for k, _ in v.values()) == {0: 70, "STREAM": 93, "JPEGLS": 10}
    per_base = {tag: collections.Counter(v[e[0]][0] for e in s.damage_files() if e[0].startswith(tag + "/")) for tag in s.bases()}
    assert per_base == {"noise_rr2": {"STREAM": 24, 0: 8, "JPEGLS": 1}, "stripes": {"STREAM": 20, "JPEGLS": 2, 0: 1},
                        "smooth_rr3": {"STREAM": 23, 0: 7, "JPEGLS": 3}, "smooth_lse": {"STREAM": 26, "JPEGLS": 4, 0: 3}}
    for tag, (x, p, rr, lse) in s.bases().items():
        assert np.array_equal(v[f"{tag}/undamaged"][1], x)
        for kind in ("removed", "doubled", "renumbered"):
            if f"{tag}/rst_{kind}" in v:
                assert v[f"{tag}/rst_{kind}"][0] == "STREAM"
        assert all(v[n][0] == "STREAM" for n in v if n.startswith(tag + "/cut_") or "_zero_bytes_behind_" in n)
    # every shape a GPU test decodes as one batch has an accepted file, and the shapes of the damage bases a refused one too
    for shape, entries in s.shapes().items():
        assert any(v[e[0]][0] == 0 for e in entries), shape
