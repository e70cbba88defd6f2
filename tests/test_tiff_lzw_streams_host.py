"""tests/tiff_lzw_streams.py without a device: every hand-built stream gets the verdict of tests/tiff_model.py, and that verdict
is Pillow's (libtiff's), byte for byte where it is a raster; the census over the cases shows every planted item, one
assertion per item, so that a changed group size, table size or hash is noticed here and not by a silently emptier GPU
test; the planted strips run the encoder's probe several windows on and round the table's end, and nothing else does."""
import functools

import numpy as np

import tiff_lzw_streams as t
import tiff_model as m


@functools.lru_cache(maxsize=None)
def censuses():
    return {c.name: t.group_census(c.codes, c.want, 8 * len(c.data)) for c in t.cases() + t.long_cases()}


@functools.lru_cache(maxsize=None)
def merged(group=None):
    cen = censuses()
    return t.merge(cen[c.name] for c in t.cases() + t.long_cases() if group in (None, c.group))


def test_every_verdict_is_the_models_and_pillows():
    wrong = []
    for c in t.cases() + t.long_cases():
        want, got = t.expected(c), m.pillow_read(t.file_of(c))
        if isinstance(want, str):
            ok = want == "CCT_E_STREAM" and not c.accept and isinstance(got, str) and got == "OSError"
        else:
            ok = c.accept and isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
        if not ok:
            wrong.append((c.name, c.accept, want if isinstance(want, str) else "raster", got if isinstance(got, str) else "raster"))
    assert not wrong, wrong
    groups = {c.group for c in t.cases()}
    assert groups == {"border", "beyond", "ingroup", "cross", "cut", "width", "table", "random"} and len(t.cases()) >= 330
    assert sum(not c.accept for c in t.cases()) >= 50 and sum(c.group == "random" for c in t.cases()) == 120


def test_every_case_reaches_what_it_plants():
    cen = censuses()
    for c in t.cases() + t.long_cases():
        assert cen[c.name]["verdict"] == ("OK" if c.accept else "CCT_E_STREAM"), c.name   # the replay in groups agrees with the model
        assert t.holds(cen[c.name], c.planted), (c.name, c.planted, {k: cen[c.name][k] for k in c.planted})
        assert len(c.data) <= 8192 and c.codes[0] == (m.CLEAR, 9), c.name   # 4862 codes are 6942 bytes, and the filler follows


def test_census_group_borders():
    c = merged("border")
    everywhere = {(lane, where) for lane in t.LANES for where in t.WHERES}
    assert everywhere <= c["stop_clear"] and everywhere <= c["stop_eoi"]
    assert {(lane, where, 0) for lane, where in everywhere} <= c["stop_end"]             # the data ends right behind a code
    cut_codes = {(lane, where) for lane, where, missing in c["stop_end"] if missing}
    assert everywhere <= cut_codes and {missing for _, _, missing in c["stop_end"]} >= set(range(8))   # and inside one: 1 .. 7 bits short
    assert {(kind, lane) for kind in ("eoi", "end") for lane in t.LANES} <= c["ignored"]   # one code behind `want`


def test_census_codes_beyond_the_table():
    c = merged("beyond")
    assert set(t.LANES) <= c["stop_bad"] and set(t.LANES) <= c["kw_lanes"] and set(t.LANES) <= c["bad_behind_clear"]
    assert c["bad_next_to_cut"] == {"before", "after"} and ("bad", 31) in c["ignored"]


def test_census_references_inside_a_group():
    c = merged("ingroup")
    assert c["chain"] == t.GROUP - 1 == 63        # what six rounds of pointer jumping resolve, and no more
    assert c["fan_in"] == 63 and c["late_of_late"] >= 60
    cen = censuses()
    assert cen["ingroup_two_interleaved_chains"]["chain"] >= 31 and cen["ingroup_star"]["fan_in"] == 63
    assert (0, "kw") in cen["ingroup_chain_goes_on_in_the_next_group"]["border_refs"]


def test_census_references_across_the_group_border():
    c = merged("cross")
    assert {(0, "kw")} | {(lane, kind0) for lane in (1, 31, 63) for kind0 in ("lit", "par", "kw")} <= c["border_refs"]
    assert {(lane, True) for lane in (0, 1, 63)} <= c["border2_refs"]   # the source ends where the group's output starts: not late


def test_census_the_cut():
    c = merged("cut")
    assert {("par", "exact"), ("par", "inside"), ("late", "inside"), ("kw", "inside"), ("lit", "exact")} <= c["cut"]
    assert {0, 63} <= c["cut_lane"] and c["cut_len"] > 64
    lane0 = censuses()["cut_at_lane0_inside_a_kwkwk"]
    assert lane0["cut"] == {("par", "inside")} and 0 in lane0["kw_lanes"]   # a KwKwK cut short of the group's output is no late copy


def test_census_long_strings():
    c = merged("long")
    assert c["cut_len"] > 1000 and {("kw", "inside"), ("par", "inside")} <= c["cut"]
    assert c["longest_parallel"] >= 3000 and c["longest_late"] >= 3000 and c["chain"] == 63
    assert t.LONG_WANT > t.LONG_CHAIN * (t.LONG_CHAIN + 1) // 2 > t.WANT    # why these have a shape of their own


def test_census_width_borders():
    c = merged("width")
    want = {(j, kind, phase) for b in t.WIDTH_BORDERS for j in (b, b + 1) for kind in ("ref", "kw", "clear") for phase in range(8)}
    assert want <= c["border_codes"], sorted(want - c["border_codes"])[:10]
    widths = {w for case in t.cases() if case.group == "width" for code, w in case.codes if code == m.CLEAR}
    assert widths == {9, 10, 11, 12}              # a Clear as code 255 / 767 / 1791 is written in the wider width


def test_census_table_limits():
    c = merged("table")
    assert (t.TAB, t.MAX_J, t.TOP_REF) == (3904, 4862, 3838)
    assert {3838, 3839, 3903, 3904, 3905, 4861, 4862, 4863} <= c["runs"]
    assert {4862, 4863} <= c["clear_numbers"] and {4094, 4095, 258, 259} <= c["refs_beyond_tab"]
    names = {case.name for case in t.cases() if case.group == "table"}
    assert all(f"table_{n}_codes_twin_clear_is_code_4862" in names for n in (3838, 3839, 3903, 3904, 3905, 4862, 4863))
    refused = [case.name for case in t.cases() if case.group == "table" and not case.accept]
    assert refused == ["table_4863_codes"]


def test_census_random_streams():
    c = merged("random")
    assert c["chain"] >= 8 and c["stop_clear"] and c["longest_late"] >= 8 and c["longest_parallel"] >= 8
    assert len({lane for lane, _ in c["border_refs"]}) >= 8 and len(c["kw_lanes"]) == 64


def test_embedded_files_have_pillows_verdict():
    files = t.embedded_files()
    assert len(files) == 2 * len(t.EMBEDDED) and {name[-2:] for name, _, _ in files} == {"II", "MM"}
    refused = 0
    for name, f, want in files:
        assert len(m.parse(f)["offs"]) == 4 and m.parse(f)["predictor"] == 2 and m.parse(f)["bits"] == 16
        got = m.pillow_read(f)
        if isinstance(want, str):
            assert want == "CCT_E_STREAM" and isinstance(got, str), name
            refused += 1
        else:
            assert isinstance(got, np.ndarray) and np.array_equal(got, want), name
            assert not np.array_equal(want, m._fixture_raster()), name      # the middle strip is the planted one
    assert 0 < refused < len(files)


def test_probe_strips_run_the_probe_on_and_round_the_tables_end():
    assert t.SLOTS == 8192
    for name, strip in t.probe_strips():
        c = t.probe_census(strip)
        assert c["codes"] == m.lzw_codes(strip), name                        # the replay is the coder
        assert c["max_rounds"] >= 3 and c["late_inserts"] >= 100 and c["late_finds"] >= 1, (name, c["max_rounds"], c["late_inserts"], c["late_finds"])
        a = np.frombuffer(strip, np.uint8).reshape(1, -1)
        assert m.same_file(m.write_file(a, "lzw"), m.pillow_file(a, "lzw")), name
        assert len(strip) < 1000
    end = t.probe_census(dict(t.probe_strips())["end"])
    assert end["wrapped_late"] >= 10 and end["wrapped"] > end["wrapped_late"]


def test_no_other_strip_of_the_suite_goes_beyond_one_probe_round():
    """the claim that only the planted strips reach `h += 64`: if a raster case starts to, this says so"""
    strips = [s for _, s in m.edge_strips()]
    for name, a, rpss in m.raster_cases():
        for pred in (1, 2):
            for rps in rpss:
                strips += m.strips_of(a, pred, rps)[0]
    assert len(strips) > 150
    most = 0
    for s in set(strips):
        c = t.probe_census(s)
        assert c["max_rounds"] <= 1 and c["late_inserts"] == c["late_finds"] == 0 and c["codes"] == m.lzw_codes(s)
        most = max(most, c["max_rounds"])
    assert most == 1
