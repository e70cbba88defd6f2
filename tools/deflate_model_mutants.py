#!/usr/bin/env python3
"""Off-by-one mutants of tools/deflate_level_model.c, one per rule of longest_match / deflate_slow that the HIP match kernels
restate, and which inputs tell each of them from libz: the generic corpus of tests/test_deflate_level_model.py or the planted
inputs of tests/deflate_match_inputs.py.  Every mutant is compiled from a patched copy in a temporary directory; nothing
mutated is written into the tree and nothing here touches the GPU.

    python tools/deflate_model_mutants.py            # the table of DESIGN.md
"""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "deflate_level_model.c")
LEVELS = (4, 5, 6, 7, 8, 9)

# (name, text of the model, replacement, occurrences).  The last one changes run_rule(), which no stream depends on: it shows as
# a difference between the run rule and the chain walk (cct_level_model_check_run_rule).
RUN_RULE_MUTANTS = ("run rule `k = r`",)
# "nice not clamped to the lookahead" cannot be told from the model by any input: a candidate is never longer than the
# lookahead and only a strictly longer one replaces the best, so the entries walked after the one that reached the lookahead
# change nothing (in zlib itself they could: its comparison runs past the lookahead before the result is clamped).
EQUIVALENT_MUTANTS = ("nice not clamped to the lookahead",)
MUTANTS = [
    ("non-head `dist >= MAX_DIST` -> `>`", "else if (dist >= MAX_DIST) break;", "else if (dist > MAX_DIST) break;", 1),
    ("head `dist > MAX_DIST` -> `>=`", "if (count == 0) { if (dist > MAX_DIST) break; }",
     "if (count == 0) { if (dist >= MAX_DIST) break; }", 1),
    ("`q == 0` NIL removed", "if (q == 0 || q == nil_q) break;", "if (q == nil_q) break;", 1),
    ("`nil_q` rule removed", "if (q == 0 || q == nil_q) break;", "if (q == 0) break;", 1),
    ("chain budget - 1", "if (count == cf->chain) break;", "if (count == cf->chain - 1) break;", 1),
    ("chain budget + 1", "if (count == cf->chain) break;", "if (count == cf->chain + 1) break;", 1),
    ("quarter budget from `good + 1`", "(prev_len >= cf->good)", "(prev_len >= cf->good + 1)", 2),
    ("`best >= nice_eff` -> `>`", "if (best >= nice_eff) break;  ", "if (best > nice_eff) break;  ", 1),
    ("nice not clamped to the lookahead", "const int nice_eff = lookahead < cf->nice ? (int)lookahead : cf->nice;",
     "const int nice_eff = cf->nice;", 1),
    ("`prev_len >= lazy` -> `>`", "if (prev_len < cf->lazy) {", "if (prev_len <= cf->lazy) {", 1),
    ("`dist > TOO_FAR` -> `>=`", "mdist > TOO_FAR", "mdist >= TOO_FAR", 1),
    ("run rule `k = r`", "const int64_t k = r < nice_eff ? r : nice_eff;", "const int64_t k = r;", 1),
]


def compile_model(text, directory, tag):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src, so = os.path.join(directory, f"model_{tag}.c"), os.path.join(directory, f"libmodel_{tag}.so")
    with open(src, "w") as f:
        f.write(text)
    subprocess.check_call([cc, "-O2", "-fPIC", "-std=c11", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.cct_level_model_deflate.restype = C.c_size_t
    lib.cct_level_model_deflate.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.cct_level_model_check_run_rule.restype = C.c_int64
    lib.cct_level_model_check_run_rule.argtypes = [C.c_char_p, C.c_size_t, C.c_int]
    return lib


def mutate(text, old, new, count):
    assert text.count(old) == count, (old, text.count(old))
    return text.replace(old, new)


def mutant_libraries(directory):
    """[(name, library)] with the unmutated model first"""
    with open(SRC) as f:
        text = f.read()
    libs = [("(the model itself)", compile_model(text, directory, "base"))]
    for k, (name, old, new, count) in enumerate(MUTANTS):
        libs.append((name, compile_model(mutate(text, old, new, count), directory, str(k))))
    return libs


def model_deflate(lib, data, level):
    out = np.empty(len(data) * 2 + 1024, dtype=np.uint8)
    n = lib.cct_level_model_deflate(data, len(data), level, out.ctypes.data)
    return out[:n].tobytes()


def first_caught(lib, items, run_rule_items, streams=True):
    """name of the first input on which the library differs from libz (streams at levels 4 to 9) or its run rule from its own
    chain walk, or None"""
    for name, data in items if streams else ():
        for level in LEVELS:
            if model_deflate(lib, data, level) != zlib.compress(data, level):
                return f"{name} (level {level})"
    for name, data in run_rule_items:
        for level in LEVELS:
            if lib.cct_level_model_check_run_rule(data, len(data), level) != -1:
                return f"{name} (run rule, level {level})"
    return None


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deflate_match_inputs as dmi
    import test_deflate_level_model as old
    old_items = list(old.CORPUS)
    old_runs = [(n, d) for n, d in old_items if n in ("runs_nice_20000", "runs_nice_70000", "alpha2_40000", "alpha3_65800",
                                                      "zeros_100k", "slice0671_payload", "phantom256_s7_payload", "run129",
                                                      "run259")]
    new_items = [(c.name, c.data) for c in dmi.cases()]
    new_runs = [(c.name, c.data) for c in dmi.cases() if c.runs]
    with tempfile.TemporaryDirectory() as d:
        print(f"| {'mutant':40} | old corpus | planted inputs |")
        print(f"|{'-' * 42}|------------|----------------|")
        for name, lib in mutant_libraries(d):
            streams = name not in RUN_RULE_MUTANTS
            a, b = first_caught(lib, old_items, old_runs, streams), first_caught(lib, new_items, new_runs, streams)
            print(f"| {name:40} | {a or 'passes'} | {b or 'passes'} |")


if __name__ == "__main__":
    main()
