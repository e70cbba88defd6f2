"""Who owns which of an encode slot's two hand-off sets (csrc/handoff.h), played on host threads by tools/handoff_probe.cpp
the way encode_batch_impl uses the rule: 2, 3, 4 and 8 callers, one in four keeping the slot and borrowing the other set.
Built with the host compiler alone, once plain and once under the thread sanitizer, and run as a program: no device."""
import os
import shutil
import subprocess

import pytest

import golden_inputs as gi

SRC = os.path.join(gi.ROOT, "tools", "handoff_probe.cpp")
HANDOFFS = 20000  # per thread
VARIANTS = {"plain": ["-O1"], "tsan": ["-O1", "-g", "-fsanitize=thread"]}


def _cxx():
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return cxx


def _links_an_empty_tsan_program(cxx, tmp):
    src = os.path.join(tmp, "empty.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    return subprocess.run([cxx, "-fsanitize=thread", "-o", os.path.join(tmp, "empty"), src],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_mark_survives_and_every_handoff_finishes(variant, tmp_path):
    cxx = _cxx()
    if variant == "tsan" and not _links_an_empty_tsan_program(cxx, str(tmp_path)):
        pytest.skip("the host compiler cannot link a thread-sanitizer program")
    exe = str(tmp_path / "probe")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-pthread", *VARIANTS[variant], "-o", exe, SRC])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    run = subprocess.run([exe, str(HANDOFFS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=900)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ThreadSanitizer" not in run.stderr, run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines()]
    assert [int(f[1]) for f in lines] == [2, 3, 4, 8]
    for f in lines:
        got = dict(zip(f[0::2], map(int, f[1::2])))
        assert got == {"threads": got["threads"], "handoffs": got["threads"] * HANDOFFS, "overwritten": 0, "too_many_owners": 0}
