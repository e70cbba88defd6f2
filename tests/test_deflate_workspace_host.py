"""The DEFLATE pass's workspace as csrc/deflate_workspace.h describes it -- region sizes, which passes need a region, where
every pointer of DeflateArgs lands -- against the formulas the host code used before there was one description (restated
here, not read back from the header).  tools/deflate_workspace_probe.cpp is built with the host compiler alone: no device."""
import itertools
import os
import shutil
import subprocess

import pytest

import golden_inputs as gi

SRC = os.path.join(gi.ROOT, "tools", "deflate_workspace_probe.cpp")
IN_STRIDES = [256, 512, 3840, 70144, 4194304 - 256]
NS = [1, 3, 256]
STRATEGIES = [0, 2, 3]
MEM_LEVELS = [8, 9]
GRID = list(itertools.product(IN_STRIDES, NS, STRATEGIES, MEM_LEVELS))

RUNLEN_OUT = 2048 - 264  # positions a workgroup of dfl_run_len_kernel publishes
SORT_HIST = 512
COUNTERS = ["seg_begin", "seg_end", "total_syms", "postloop_lit", "n_blocks", "adler", "heavy_count", "deep_count", "run_end_count"]
SIZEOF_BLOCK_META = 8 + 8 * 4
SIZEOF_BLOCK_TABLES = 286 * 2 + 286 + 30 * 2 + 30 + 160 * 4
(REC_IN, REC_OUT, MATCH, RUNS, QUEUES, SYM, REC32, EXIT_POS, BLK_ENTRY, BLK_SYMBASE, SMALL, BLK_ENDS, META, TABLES, GEN) = range(15)
CHAINS, WALK = {REC_IN, REC_OUT, MATCH, RUNS, QUEUES}, {REC32, EXIT_POS, BLK_ENTRY, BLK_SYMBASE}


def expected(in_stride, n, strategy, mem_level):
    """(region sizes, needed flags, {pointer: (region, byte offset)}) by the formulas of the table in DESIGN.md 5h"""
    eb = n * in_stride
    max_blocks = in_stride // ((1 << (mem_level + 6)) - 1) + 2
    run_chunks = in_stride // 1784 + 1
    sizes = {REC_IN: 8 * eb, REC_OUT: 8 * eb, MATCH: 8 * eb, RUNS: 4 * eb, QUEUES: 4 * eb, SYM: 4 * eb, REC32: 4 * eb,
             EXIT_POS: 4 * eb, BLK_ENTRY: eb // 64 * 4, BLK_SYMBASE: eb // 64 * 4,
             SMALL: n * (9 + SORT_HIST + 2 * run_chunks) * 4, BLK_ENDS: n * max_blocks * 8,
             META: n * max_blocks * SIZEOF_BLOCK_META, TABLES: n * max_blocks * SIZEOF_BLOCK_TABLES, GEN: 256}
    chains, walk = strategy not in (2, 3), strategy != 2
    needed = {r: (chains if r in CHAINS else walk if r in WALK else True) for r in sizes}
    ptrs = {"rec_in": (REC_IN, 0), "rec_out": (REC_OUT, 0), "mr": (MATCH, 0), "run_ends": (RUNS, 0), "heavy_list": (QUEUES, 0),
            "exit_cnt": (QUEUES, 0), "sym": (SYM, 0), "run_len": (SYM, 0), "rec32": (REC32, 0), "exit_pos": (EXIT_POS, 0),
            "blk_entry": (BLK_ENTRY, 0), "blk_symbase": (BLK_SYMBASE, 0), "sort_hist": (SMALL, 9 * n * 4),
            "run_counts": (SMALL, (9 + SORT_HIST) * n * 4), "blk_end": (BLK_ENDS, 0), "blk_top": (BLK_ENDS, n * max_blocks * 4),
            "block_meta": (META, 0), "block_tables": (TABLES, 0), "gen": (GEN, 0)}
    for k, name in enumerate(COUNTERS):
        ptrs[name] = (SMALL, k * n * 4)
    return sizes, needed, ptrs, max_blocks, run_chunks


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("deflate_workspace") / "probe")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC])
    args = [str(v) for case in GRID for v in case]
    out = subprocess.check_output([exe] + args, text=True).splitlines()
    consts = dict(zip(out[0].split()[1::2], map(int, out[0].split()[2::2])))
    cases, cur = {}, None
    for line in out[1:]:
        f = line.split()
        if f[0] == "case":
            cur = {"info": dict(zip(f[5::2], map(int, f[6::2]))), "sizes": {}, "needed": {}, "ptrs": {}}
            cases[tuple(map(int, f[1:5]))] = cur
        elif f[0] == "region":
            cur["sizes"][int(f[1])], cur["needed"][int(f[1])] = int(f[2]), bool(int(f[3]))
        elif f[0] == "ptr":
            cur["ptrs"][f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "bound_args":
            cur["bound_args"] = (int(f[2]), int(f[4]))
        elif f[0] == "runs":
            cur["runs"] = dict(zip(f[1::2], map(int, f[2::2])))
    return consts, cases


def test_shared_constants(probe):
    consts = dict(probe[0])
    # DeflateArgs keeps its layout: 352 bytes, the kernel argument segment of every dfl_* kernel that takes it alone
    assert consts.pop("args") == 352
    assert consts == {"RUNLEN_OUT": RUNLEN_OUT, "SORT_HIST": SORT_HIST, "COUNTERS": len(COUNTERS), "GRAIN": 64, "REGIONS": 15,
                      "meta": SIZEOF_BLOCK_META, "tables": SIZEOF_BLOCK_TABLES}


def test_regions_and_binding_over_the_grid(probe):
    _, cases = probe
    assert sorted(cases) == sorted(GRID)
    for case in GRID:
        in_stride, n, strategy, mem_level = case
        got = cases[case]
        sizes, needed, ptrs, max_blocks, run_chunks = expected(*case)
        assert got["sizes"] == sizes, case
        assert got["needed"] == needed, case
        assert got["ptrs"] == ptrs, case
        assert got["bound_args"] == (max_blocks, run_chunks), case
        info = got["info"]
        assert (info["max_blocks"], info["run_chunks"]) == (max_blocks, run_chunks), case
        assert info["blk_words"] == in_stride // 64, case
        # a chunk per RUNLEN_OUT positions covers the slice
        assert run_chunks * RUNLEN_OUT >= in_stride, case
        # run_counts begins exactly n * SORT_HIST words after sort_hist: one kernel zeroes both, and both fit in their region
        assert got["ptrs"]["run_counts"][1] - got["ptrs"]["sort_hist"][1] == n * SORT_HIST * 4, case
        assert info["hist_words"] == n * (SORT_HIST + 2 * run_chunks), case
        assert got["ptrs"]["sort_hist"][1] + info["hist_words"] * 4 == sizes[SMALL], case
        assert got["ptrs"]["blk_top"][1] + n * max_blocks * 4 == sizes[BLK_ENDS], case
        # the four quarters of a slice's run lists and the in_stride / 8 rank words fit in its in_stride words
        runs = got["runs"]
        q = in_stride // 4
        assert (runs["starts"], runs["info"], runs["rank0"]) == (q, 2 * q, 3 * q), case
        assert runs["rank_last"] == 3 * q + (in_stride - 1) // 8 and runs["rank_last"] < in_stride, case
        assert 3 * q + in_stride // 8 <= in_stride, case
        # the deep queue starts at the last word of the slice's queue region
        assert runs["deep_top"] == in_stride - 1, case
        # the zlib bound and the strides of a pass
        bound = (in_stride + (in_stride >> 12) + (in_stride >> 14) + (in_stride >> 25) + 13 if mem_level == 8
                 else in_stride + ((in_stride + 7) >> 3) + ((in_stride + 63) >> 6) + 5 + 6)
        assert info["bound"] == bound, case
        assert info["in_stride_of"] == ((in_stride - 16) + 16 + 255) & ~255 == in_stride, case
        assert info["out_stride"] == (13 + bound + 63) & ~63, case


def test_short_passes_leave_the_chain_workspaces_alone(probe):
    _, cases = probe
    for case in GRID:
        needed = cases[case]["needed"]
        strategy = case[2]
        if strategy == 2:  # Z_HUFFMAN_ONLY: neither the chain nor the walk regions
            assert not any(needed[r] for r in CHAINS | WALK), case
        elif strategy == 3:  # Z_RLE: of those, the walk regions only
            assert not any(needed[r] for r in CHAINS) and all(needed[r] for r in WALK), case
        else:
            assert all(needed.values()), case
        assert all(needed[r] for r in (SYM, SMALL, BLK_ENDS, META, TABLES, GEN)), case
