"""The INFLATE kernel and the PNG reader kernels on host threads (tools/debug/inflate_host_emu): the kernel files compiled with the
host compiler under AddressSanitizer and UBSan, with a poisoned gap behind every LDS array, inputs and output slots allocated
exactly, and CPython's zlib as the judge of every verdict and byte.  The program is built here and run as a child process: no
device, nothing sanitized is loaded into Python.  This file runs a part of the corpora; `python
tools/debug/inflate_host_emu/drive.py` runs all of them (each hand-built stream alone as well, 400 damaged streams per geometry,
the .cct entrance, the PNG edge shapes)."""
import importlib.util
import os
import shutil
import subprocess

import pytest

import golden_inputs as gi

_spec = importlib.util.spec_from_file_location("inflate_emu_drive", os.path.join(gi.ROOT, "tools", "debug", "inflate_host_emu", "drive.py"))
drive = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(drive)

DAMAGE_N = 100  # per geometry
GRID_N = 25     # of them also as the workgroups of one launch


def _cxx():
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return cxx


def _sanitizer_link(cxx, tmp):
    """(flags, None) with which an empty sanitized program links and runs here, or (None, which of the two steps failed).  The
    runtimes are linked into the program where the compiler can do that, so that the program does not depend on what else the
    loader brings in."""
    src, exe = os.path.join(tmp, "empty.cpp"), os.path.join(tmp, "empty")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    why = "the host compiler cannot link an address-sanitizer program"
    for extra in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        if subprocess.run([cxx, *drive.SANITIZE, *extra, "-o", exe, src], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode:
            continue
        run = subprocess.run([exe], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if run.returncode == 0:
            return extra, None
        why = f"an empty address-sanitizer program links here but does not run (exit status {run.returncode}): {run.stderr.strip()[:200]}"
    return None, why


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("inflate_emu"))
    cxx = _cxx()
    extra, why = _sanitizer_link(cxx, tmp)
    if extra is None:
        pytest.skip(why)
    drive.build(os.path.join(tmp, "emu"), cxx, extra)
    old, drive.EMU = drive.EMU, os.path.join(tmp, "emu")
    yield drive
    drive.EMU = old


def test_damage_family_reaches_the_huffman_blocks():
    """the reference alone: of the full family of every geometry, zlib accepts at least 15 % and refuses at least 30 streams inside
    a Huffman block (not at a header or at the Adler-32); the part run below keeps that proportion"""
    for lanes in drive.LANES:
        items = drive.damage_family(drive.DAMAGE_SEEDS[lanes], drive.DAMAGE_N)
        accepted, in_block = drive.damage_census(items)
        assert drive.DAMAGE_N >= 400 and in_block >= 30 and accepted >= 0.15 * drive.DAMAGE_N, (lanes, accepted, in_block)
        accepted, in_block = drive.damage_census(items[:DAMAGE_N])
        assert in_block >= 30 * DAMAGE_N // 400 and accepted >= 0.15 * DAMAGE_N, (lanes, accepted, in_block)


def test_hand_built_streams_256(emu):
    emu.run_hand(256)


@pytest.mark.parametrize("lanes", drive.LANES)
def test_walk_edges(emu, lanes):
    emu.run_walk(lanes, every_batch=False)


@pytest.mark.parametrize("lanes", drive.LANES)
def test_damaged_streams(emu, lanes):
    emu.run_damage(lanes, DAMAGE_N, min_in_block=30 * DAMAGE_N // 400, grid_n=GRID_N)


def test_png_chunk_and_damaged_cases(emu):
    emu.run_png_core(256, both_orders=False)
