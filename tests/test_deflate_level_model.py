"""Pins tools/deflate_level_model.c -- the data-parallel restatement of zlib 1.2.11 deflate_slow with the level as a
parameter (levels 4 to 9), the rules the HIP DEFLATE kernels implement -- to the system libz: byte-identical
streams at every level, and the run rule of dfl_match_run_kernel (with the nice_match cut-off) identical to the
chain walk."""
import ctypes as C
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import golden_inputs as gi

SRC = os.path.join(gi.ROOT, "tools", "deflate_level_model.c")
LEVELS = [4, 5, 6, 7, 8, 9]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    so = str(tmp_path_factory.mktemp("level_model") / "libdeflate_level_model.so")
    subprocess.check_call([cc, "-O2", "-fPIC", "-std=c11", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.cct_level_model_deflate.restype = C.c_size_t
    L.cct_level_model_deflate.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_void_p]
    L.cct_level_model_check_run_rule.restype = C.c_int64
    L.cct_level_model_check_run_rule.argtypes = [C.c_char_p, C.c_size_t, C.c_int]
    return L


def _deflate(L, b, level):
    out = np.empty(len(b) * 2 + 1024, dtype=np.uint8)
    n = L.cct_level_model_deflate(b, len(b), level, out.ctypes.data)
    return out[:n].tobytes()


def _rng_bytes(seed, alphabet, n):
    return np.random.default_rng(seed).integers(0, alphabet, n, dtype=np.uint8).tobytes()


def _runs_beyond_nice(seed, n):
    """Runs longer than nice_match whose following bytes repeat an earlier run's continuation: with the cut-off the
    first candidate reaching nice ends the walk before the longer extension behind an older run is seen."""
    rng = np.random.default_rng(seed)
    tails = [bytes(rng.integers(0, 256, 12, dtype=np.uint8)) for _ in range(4)]
    out = bytearray()
    while len(out) < n:
        b = int(rng.integers(0, 3))
        r = int(rng.choice([3, 4, 5, 15, 16, 17, 31, 32, 33, 60, 127, 128, 129, 200, 257, 258, 259, 300]))
        out += bytes([b]) * r + tails[int(rng.integers(0, len(tails)))][: int(rng.integers(1, 12))]
        if rng.random() < 0.3:
            out += bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8))
    return bytes(out[:n])


def _golden_payload(name):
    with open(os.path.join(gi.GOLDEN, name + ".cct"), "rb") as f:
        return zlib.decompress(f.read()[13:])


def _raw_slice(name):
    with open(os.path.join(gi.GOLDEN, name + ".u16.zz"), "rb") as f:
        return zlib.decompress(f.read())


def corpus():
    """(name, bytes) pairs shared with tests/test_gpu_deflate_levels.py."""
    items = [("empty", b""), ("one", b"a"), ("two", b"ab"), ("three", b"abc"), ("abc_rep", b"abcabcabcabc" * 10)]
    for r in (2, 3, 4, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257, 258, 259, 1000):
        items.append((f"run{r}", b"q" * r + b"Z" + b"q" * (r // 2) + b"Y" + b"q" * r + b"Z"))
    items += [
        ("random256_5000", _rng_bytes(0, 256, 5000)),
        ("alpha4_70000", _rng_bytes(1, 4, 70000)),
        ("alpha16_120000", _rng_bytes(2, 16, 120000)),
        ("alpha2_40000", _rng_bytes(4, 2, 40000)),
        ("alpha3_65800", _rng_bytes(8, 3, 65800)),
        ("alpha64_33000", _rng_bytes(10, 64, 33000)),
        ("runs_nice_20000", _runs_beyond_nice(11, 20000)),
        ("runs_nice_70000", _runs_beyond_nice(12, 70000)),
        ("runs_nice_270000", _runs_beyond_nice(13, 270000)),
        ("zeros_100k", bytes(100000)),
    ]
    for name in ("slice0671", "slice3706", "phantom256_s7"):
        items.append((name + "_payload", _golden_payload(name)))
    for name in ("slice0671", "slice3706"):
        items.append((name + "_raw", _raw_slice(name)))
    return items


CORPUS = corpus()
IDS = [c[0] for c in CORPUS]


def test_zlib_version_is_the_pinned_one():
    assert zlib.ZLIB_RUNTIME_VERSION == "1.2.11"


def test_corpus_exercises_the_level_rules():
    """Most inputs compress differently at the lower levels, so equality below is not level 9 in disguise."""
    for level in (4, 5, 6):
        differ = sum(zlib.compress(x, level) != zlib.compress(x, 9) for _, x in CORPUS)
        assert differ >= len(CORPUS) * 0.6, (level, differ)
    for level in (7, 8):
        assert sum(zlib.compress(x, level) != zlib.compress(x, 9) for _, x in CORPUS) >= 8, level


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", IDS)
def test_model_equals_libz(lib, name, level):
    data = dict(CORPUS)[name]
    assert _deflate(lib, data, level) == zlib.compress(data, level)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", ["runs_nice_20000", "runs_nice_70000", "alpha2_40000", "alpha3_65800", "zeros_100k",
                                  "slice0671_payload", "phantom256_s7_payload", "run129", "run259"])
def test_run_rule_equals_chain_walk(lib, name, level):
    data = dict(CORPUS)[name]
    assert lib.cct_level_model_check_run_rule(data, len(data), level) == -1


def test_other_levels_are_refused(lib):
    for level in (-1, 0, 1, 2, 3, 10):
        assert lib.cct_level_model_deflate(b"abc", 3, level, None) == 0
        assert lib.cct_level_model_check_run_rule(b"aaaa", 4, level) == -2
