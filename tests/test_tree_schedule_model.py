"""Pins the pipelined heap replay of dfl_tree_kernel (deflate_kernels.hip tree_heap) to trees.c: the host model
tools/tree_schedule_model.cpp runs the kernel's tick schedule and compares heap tail, dad[], freq[] and depths with a plain
sequential build_tree, for every heap size, tie-heavy histograms and the block histograms of the golden payloads."""
import os
import shutil
import subprocess
import zlib

import pytest

import deflate_blocks as db
import golden_inputs as gi

SRC = os.path.join(gi.ROOT, "tools", "tree_schedule_model.cpp")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tree_model") / "tree_schedule_model")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", exe, SRC])
    return exe


def _run(exe, args=(), stdin=""):
    p = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), p.stdout
    return lines


def _stat(line, key):
    toks = line.split()
    return float(toks[toks.index(key) + 1])


def test_every_heap_size_and_tie_heavy_histograms(model):
    lines = _run(model, ["--builtin"])
    names = [ln.split()[1] for ln in lines]
    assert names == ["sizes", "all_ones", "two_values", "geometric", "equal_pairs", "random", "small"]
    for ln in lines:
        assert _stat(ln, "max_in_flight") <= 5  # TREE_SIFTS = 8 slots, round robin, are never reused too early


@pytest.mark.parametrize("name", ["crop128_f0s0d0", "crop128_f1s1d0", "crop128_f1s1d1", "int16_signed", "int16_texture",
                                  "noise64_nodeflate", "q4_block0", "q7_spike", "phantom256_s7", "slice0671"])
def test_golden_payload_block_histograms(model, name):
    with open(os.path.join(gi.GOLDEN, name + ".cct"), "rb") as f:
        head, body = f.read(13), f.read()
    payload = zlib.decompress(body) if head[12] == 1 else body  # byte 12: the payload is stored deflated
    hists = [(lf, df) for t, lf, df, _ in db.blocks(zlib.compress(payload, 9), max_blocks=6) if t]
    assert hists
    lines = "".join(f"286 {' '.join(map(str, lf))}\n30 {' '.join(map(str, df))}\n" for lf, df in hists)
    (ln,) = _run(model, stdin=lines)
    assert _stat(ln, "cases") == 2 * len(hists)


def test_trees_deeper_than_the_limit(model):
    """Fibonacci chains below flat blocks: the trees gen_bitlen has to repair (tree_fix walks the heap tail)"""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    rows = []
    for nflat, flat, nchain in [(32, 400, 14), (48, 250, 14), (64, 200, 13), (8, 1000, 17)]:
        h = [0] * 286
        for i, f in enumerate(fib[1:nchain] + [flat] * nflat):
            h[(i * 37) % 256] = f
        h[256] = 1
        assert db.uncapped_depth(h) > 15
        rows.append("286 " + " ".join(map(str, h)) + "\n")
    (ln,) = _run(model, stdin="".join(rows))
    assert _stat(ln, "cases") == len(rows)


def test_fewer_serial_steps_than_the_sequential_replay(model):
    """a full literal/length tree: the schedule needs well under half the levels the one-lane replay ran"""
    import numpy as np
    rng = np.random.default_rng(3)
    rows = "".join(f"286 {' '.join(map(str, rng.integers(1, 120, 286)))}\n" for _ in range(8))
    (ln,) = _run(model, stdin=rows)
    assert _stat(ln, "fixed/ticks") >= 2.0
