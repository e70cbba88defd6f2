"""The planted inputs of tests/deflate_match_inputs.py do what they are named after, checked without a GPU: the census of
every case holds on libz's own token stream, tools/deflate_level_model.c (the rules the HIP match kernels restate) equals libz
on every case at levels 4 to 9, its run rule equals its chain walk on the run cases, and one-rule mutants of the model are
told from libz by these inputs."""
import os
import sys
import time
import zlib

import numpy as np
import pytest

import deflate_blocks as db
import deflate_match_inputs as dmi
import golden_inputs as gi

sys.path.insert(0, os.path.join(gi.ROOT, "tools"))
import deflate_model_mutants as mm  # noqa: E402

_t0 = time.perf_counter()
CASES = dmi.cases()
BUILD_SECONDS = time.perf_counter() - _t0
BY_NAME = {c.name: c for c in CASES}
# cases per family; a case that is dropped or moved fails here (no case may be dropped: one whose census cannot be met is
# redesigned)
FAMILIES = {"window": 18, "nil": 12, "budget": 59, "steps": 20, "quarter": 44, "nice": 19, "lazy": 17, "far": 10, "end": 21,
            "runs": 138, "sorted": 25}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    with open(mm.SRC) as f:
        return mm.compile_model(f.read(), str(tmp_path_factory.mktemp("match_model")), "base")


def test_every_case_is_there_and_building_them_is_quick():
    print(f"\n{len(CASES)} cases, {sum(len(c.data) for c in CASES)} bytes, built in {BUILD_SECONDS:.2f} s")
    assert dmi.family_counts() == FAMILIES
    assert max(len(c.data) for c in CASES) <= 140 * 1024
    assert BUILD_SECONDS < 20


def test_filler_and_plants_keep_apart():
    f = np.frombuffer(dmi.filler(), dtype=np.uint8).astype(np.int64)
    tri = (f[:-2] << 16) | (f[1:-1] << 8) | f[2:]
    assert len(np.unique(tri)) == len(tri)                      # no 3-byte string twice
    assert 48 <= len(set(dmi.filler())) <= 64                   # small enough for dynamic blocks
    assert all((b & 31) >= 8 for b in dmi.FILL_ALPHABET) and all(1 <= (b & 31) <= 6 for b in dmi.body())
    b = np.frombuffer(dmi.body(), dtype=np.uint8).astype(np.int64)
    tri = (b[:-2] << 16) | (b[1:-1] << 8) | b[2:]
    assert len(np.unique(tri)) == len(tri)
    for c in CASES:  # the probe bucket's third byte (or the run byte) is the only byte of class 0
        zeros = {x for x in set(c.data) if x & 31 == 0}
        assert zeros <= ({dmi.RUN} if c.runs else {dmi.Z, dmi.Z ^ 0x20, dmi.Z ^ 0x40}), c.name


def test_sorted_index_is_the_stable_sort_by_hash_then_position():
    data = BY_NAME["sorted_lane_depth65_same"].data
    for bits in (15, 16):
        order = np.argsort(dmi.hashes(data, bits), kind="stable")
        for p in (0, 1, 77, len(data) // 2, len(data) - 3):
            assert order[dmi.sorted_index(data, p, bits)] == p


def test_token_reader_agrees_with_the_block_histograms():
    for name, level in (("budget_depth129_same", 6), ("run_prev300_then300_same_cont", 9), ("end_L9", 4),
                        ("nil_slide_k2_after263", 9)):
        data = BY_NAME[name].data
        stream = dmi.libz(data, level)
        toks, stored = dmi.tokens(stream)
        assert not stored and toks == dmi.libz_tokens(data, level).toks
        hist = db.blocks(stream)
        assert len(toks) == sum(sum(lf[257:]) for _, lf, _, _ in hist) == sum(sum(df) for _, _, df, _ in hist)
        assert len(data) == sum(t[1] for t in toks) + sum(sum(lf[:256]) for _, lf, _, _ in hist)
        for p, n, d in toks:
            assert data[p:p + n] == bytes(data[p - d + k % d] for k in range(n))  # a token copies what is there


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_census_holds_on_libz(name):
    c = BY_NAME[name]
    for level in c.levels:
        for strategy in c.strategies:
            assert c.holds(level, strategy), (name, level, strategy)
            assert not dmi.libz_tokens(c.data, level, strategy).stored, (name, level, "stored block")
        if c.mem9:
            assert c.holds(level, 0, 9), (name, level, "memLevel 9")


def test_the_two_sides_of_the_slide_quirk_differ():
    for k in (1, 2):
        a, b = BY_NAME[f"nil_slide_k{k}_after261"], BY_NAME[f"nil_slide_k{k}_after262"]
        p = dmi.MAX_DIST + 32768 * k
        assert a.data[:p + 9] == b.data[:p + 9]
        assert dmi.libz_tokens(a.data, 9).at(p) is None and dmi.libz_tokens(b.data, 9).at(p) == (9, dmi.MAX_DIST)


@pytest.mark.parametrize("level", dmi.LEVELS)
def test_model_equals_libz_on_every_case(lib, level):
    for c in CASES:
        assert mm.model_deflate(lib, c.data, level) == zlib.compress(c.data, level), c.name


@pytest.mark.parametrize("level", dmi.LEVELS)
def test_run_rule_equals_chain_walk_on_the_run_cases(lib, level):
    runs = [c for c in CASES if c.runs]
    assert len(runs) == FAMILIES["runs"]
    for c in runs:
        assert lib.cct_level_model_check_run_rule(c.data, len(c.data), level) == -1, c.name


# the family of cases made for the rule that each mutant of tools/deflate_model_mutants.py breaks
MUTANT_FAMILY = {"non-head `dist >= MAX_DIST` -> `>`": "window", "head `dist > MAX_DIST` -> `>=`": "window",
                 "`q == 0` NIL removed": "nil", "`nil_q` rule removed": "nil", "chain budget - 1": "budget",
                 "chain budget + 1": "budget", "quarter budget from `good + 1`": "quarter", "`best >= nice_eff` -> `>`": "nice",
                 "`prev_len >= lazy` -> `>`": "lazy", "`dist > TOO_FAR` -> `>=`": "far", "run rule `k = r`": "runs"}


def test_one_rule_mutants_of_the_model_are_caught(tmp_path):
    """each off-by-one of the model differs from libz on an input of the family planted on that rule's edge.  The one mutant
    that no input can tell from the model is named in the tool."""
    assert set(MUTANT_FAMILY) | set(mm.EQUIVALENT_MUTANTS) == {m[0] for m in mm.MUTANTS}
    missed = []
    for name, library in mm.mutant_libraries(str(tmp_path))[1:]:
        if name in mm.EQUIVALENT_MUTANTS:
            continue
        items = sorted(((c.name, c.data) for c in CASES if c.family == MUTANT_FAMILY[name]), key=lambda it: len(it[1]))
        if mm.first_caught(library, items, items, name not in mm.RUN_RULE_MUTANTS) is None:
            missed.append(name)
    assert not missed
