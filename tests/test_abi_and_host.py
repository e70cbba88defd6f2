"""CPU-side checks of the product: the C-ABI library loads and exports every symbol declared in
include/compact_hip.h, host-only entry points work (traversal table, sizes, header parsing), and
compute entry points fail loudly without a GPU (no CPU fallback)."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import golden_inputs as gi

ROOT = gi.ROOT


def _declared():
    text = open(os.path.join(ROOT, "include", "compact_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cct_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from cct_hip import _ffi
    L = _ffi.lib()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/compact_hip.h but not exported"
    assert sorted(_ffi.exported_symbols()) == names
    assert L.cct_version() == 1


def test_curve_table_matches_reference_known_answers(manifest):
    from codec.curve import GeneralizedHilbertCurve
    for key, ka in manifest["curves"].items():
        w, h = map(int, key.split("x"))
        t = np.asarray(GeneralizedHilbertCurve(w, h, get_index=True).generate_all(), dtype="<i4")
        if "list" in ka:
            assert t.tolist() == ka["list"]
        else:
            assert gi.sha1(t.tobytes()) == ka["sha1"], key
    assert GeneralizedHilbertCurve(4, 4).generate_all()[:3] == [(0, 0), (0, 1), (1, 1)]


def test_sizes_and_header():
    from cct_hip import _ffi
    L = _ffi.lib()
    s = L.cct_payload_stride(512, 512, 16)
    assert s % 256 == 0 and s >= 2 * 512 * 512 + 16384 // 2 + 1
    assert L.cct_file_bound(512, 512, 16) > s
    with open(os.path.join(gi.GOLDEN, "slice0671.cct"), "rb") as f:
        blob = f.read()
    hdr = _ffi.Header()
    assert L.cct_read_header(blob, len(blob), b"pact", C.byref(hdr)) == 0
    assert (hdr.width, hdr.height, hdr.channels, hdr.bytes_per_channel) == (512, 512, 1, 2)
    assert (hdr.fractal, hdr.segmentation, hdr.deflate) == (1, 1, 1)
    assert L.cct_read_header(b"nope" + blob[4:], len(blob), b"pact", C.byref(hdr)) == _ffi.E_MAGIC


def test_config_is_the_reference_default():
    from cct_hip import default_config, codec_params
    cfg = default_config()
    assert cfg["magic"] == "pact" and cfg["extension"] == "cct" and cfg["block_size"] == 16
    flags, bs, eof, magic, ch, bpc = codec_params(cfg, np.uint16)
    assert (flags, bs, eof, magic, ch, bpc) == (7, 16, 59, b"pact", 1, 2)
    assert codec_params(cfg, np.int16)[0] == 15


def test_no_cpu_fallback_without_gpu():
    """On a machine without a usable gfx950 device every compute call must raise."""
    from cct_hip import _ffi
    import cct_hip
    if _ffi.lib().cct_init(-1) == 0:
        pytest.skip("a GPU is present")
    img = np.zeros((16, 16), np.uint16)
    with pytest.raises(_ffi.DeviceError):
        cct_hip.encode_batch(img[None])
    from codec.core import Encoder
    with pytest.raises(_ffi.DeviceError):
        Encoder(cct_hip.default_config(), img).encode()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "2023-compact-image-compression_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dirpath, fn), errors="replace").read()
                # comments may cite oracle/ files; code must not import, include, link or load them
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{fn} imports the oracle"
                assert not re.search(r"#\s*include[^\n]*oracle", src), f"{fn} includes oracle code"
                assert "libcompact_oracle" not in src and "libdeflate_model" not in src, f"{fn} loads an oracle library"


def test_options_round_trip_without_a_device():
    """cct_set_option / cct_get_option are host state: they work before (and without) a device, clamp what they must and
    refuse what they do not know."""
    import ctypes as C
    from cct_hip import _ffi
    L = _ffi.lib()
    v = C.c_int(-1)
    for key, given, want in ((b"encode_slots", 2, 2), (b"encode_slots", 7, 2), (b"encode_slots", 0, 1), (b"decode_slots", 1, 1),
                             (b"decode_slots", 5, 2), (b"tile_path", 2, 2), (b"tile_path", 4, 4),
                             (b"tile_path", 9, 1), (b"device_inflate", 5, 1), (b"deflate_graph", 0, 0), (b"deflate_graph", 1, 1),
                             (b"deflate_compact_records", 0, 0), (b"deflate_compact_records", 3, 1),
                             (b"decode_yields", 0, 0), (b"decode_yields", 2, 1), (b"queue_ahead", 0, 0), (b"queue_ahead", 1, 1),
                             (b"deflate_fork", 0, 0), (b"deflate_fork", 1, 1)):
        assert L.cct_set_option(key, given) == 0
        assert L.cct_get_option(key, C.byref(v)) == 0 and v.value == want, (key, given, v.value)
    # tile_path 3 (the four-kernel pipeline) is removed: refused, and the current choice stays
    assert L.cct_set_option(b"tile_path", 4) == 0 and L.cct_set_option(b"tile_path", 3) != 0
    assert L.cct_get_option(b"tile_path", C.byref(v)) == 0 and v.value == 4
    assert L.cct_set_option(b"encode_slots", 1) == 0 and L.cct_set_option(b"tile_path", 1) == 0
    assert L.cct_set_option(b"deflate_ways", 2) != 0      # removed in round 2
    assert L.cct_set_option(b"pipe_tpw", 1) != 0          # removed with the pipeline
    assert L.cct_set_option(b"pipe_timing", 1) != 0
    assert L.cct_set_option(b"no_such_option", 1) != 0
    assert L.cct_get_option(b"no_such_option", C.byref(v)) != 0


# every key include/compact_hip.h documents: (value given, value read back) pairs and the values refused, by the rule the
# header states for the key; None: read only
OPTION_RULES = {
    "encode_slots": ([(1, 1), (2, 2), (0, 1), (-5, 1), (7, 2)], []),
    "decode_slots": ([(1, 1), (2, 2), (0, 1), (9, 2)], []),
    "device_deflate": ([(0, 0), (1, 1), (5, 1), (-1, 1)], []),
    "device_inflate": ([(0, 0), (1, 1), (5, 1), (-1, 1)], []),
    "zlib_threads": ([(1, 1), (3, 3), (64, 64)], [0, -1]),
    "png_unfilter_waves": ([(1, 1), (2, 2), (4, 4), (8, 8)], [0, 3, 16, -1]),
    "inflate_lanes": ([(256, 256), (512, 512), (0, 0)], [1, 128, 1024, -1]),
    "last_inflate_lanes": None,
    "tile_path": ([(0, 0), (1, 1), (2, 2), (4, 4), (5, 1), (-1, 1), (9, 1)], [3]),
    "stream_tpg": ([(1, 1), (2, 2), (4, 4), (3, 4), (0, 4), (8, 4)], []),
    "wg_threads": ([(256, 256), (512, 512), (1024, 1024)], [0, 64, 768, 2048]),
    "deflate_graph": ([(0, 0), (1, 1), (7, 1), (-1, 1)], []),
    "deflate_fork": ([(0, 0), (1, 1), (7, 1), (-1, 1)], []),
    "deflate_compact_records": ([(0, 0), (1, 1), (7, 1), (-1, 1)], []),
    "runtime_block_size": ([(0, 0), (1, 1), (7, 1), (-1, 1)], []),
    "decode_yields": ([(0, 0), (1, 1), (7, 1), (-1, 1)], []),
    "queue_ahead": ([(0, 0), (1, 1), (7, 1), (-1, 1)], []),
    "last_encode_path": None,
    "last_decode_path": None,
}


def _documented_options():
    text = open(os.path.join(ROOT, "include", "compact_hip.h")).read()
    text = text[text.index("/* Options."):text.index("int cct_set_option")]
    return sorted(set(re.findall(r'"([a-z_]+)"', text)))


def test_every_documented_option_follows_its_rule():
    """Every key of the header's option list goes through cct_set_option and cct_get_option: accepted values read back as
    the header says (kept or clamped), refused values return CCT_E_ARG and leave the option alone, read-only keys can be
    read and not set.  Each key gets its first value back at the end."""
    from cct_hip import _ffi
    L = _ffi.lib()
    keys = _documented_options()
    assert keys == sorted(OPTION_RULES) and len(keys) == 19
    v = C.c_int(-1)
    for key in keys:
        k = key.encode()
        assert L.cct_get_option(k, C.byref(v)) == 0, key
        first = v.value
        if OPTION_RULES[key] is None:
            assert L.cct_set_option(k, first) == _ffi.E_ARG and _ffi.last_error() == f"unknown option {key}"
            assert L.cct_get_option(k, C.byref(v)) == 0 and v.value == first
            continue
        accepted, refused = OPTION_RULES[key]
        for given, want in accepted:
            assert L.cct_set_option(k, given) == 0, (key, given)
            assert L.cct_get_option(k, C.byref(v)) == 0 and v.value == want, (key, given, v.value)
            for bad in refused:
                assert L.cct_set_option(k, bad) == _ffi.E_ARG and key in _ffi.last_error(), (key, bad)
                assert L.cct_get_option(k, C.byref(v)) == 0 and v.value == want, (key, bad, v.value)
        if L.cct_set_option(k, first) != 0:   # a default outside what can be set ("zlib_threads" 0: not chosen yet)
            assert first in refused and L.cct_shutdown() == 0   # host state back to its defaults
        assert L.cct_get_option(k, C.byref(v)) == 0 and v.value == first, key


SWITCH_NAMES = (b"CCT_STREAM_DBG", b"CCT_STREAM_STAMPS", b"CCT_INF_PROF", b"CCT_J2K_STAGES", b"CCT_J2K_DEC_STAGES", b"CCT_TRACE")
release_only = pytest.mark.skipif(bool(os.environ.get("CCT_HIP_LIB")), reason="CCT_HIP_LIB names another build of the library")


@release_only
def test_release_library_refuses_debug_skip():
    from cct_hip import _ffi
    L = _ffi.lib()
    assert L.cct_set_option(b"debug_skip", 1) == _ffi.E_ARG and _ffi.last_error() == "unknown option debug_skip"
    assert L.cct_set_option(b"debug_skip", 0) == _ffi.E_ARG


@release_only
def test_release_library_is_no_tuning_build():
    from cct_hip import _ffi
    L = _ffi.lib()
    v = C.c_int(-1)
    assert L.cct_get_option(b"tuning_build", C.byref(v)) == _ffi.E_ARG and v.value == -1
    assert _ffi.last_error() == "unknown option tuning_build"
    assert L.cct_set_option(b"tuning_build", 1) == _ffi.E_ARG


@release_only
def test_release_library_names_no_diagnostic_switch():
    """No environment variable can reach a diagnostic path of the release library: their names are not in it."""
    from cct_hip import _ffi
    with open(_ffi.LIB_PATH, "rb") as f:
        blob = f.read()
    assert len(blob) > 100000
    for name in SWITCH_NAMES:
        assert name not in blob, name.decode()


def test_shutdown_twice_and_from_threads():
    """cct_shutdown replaces the slot objects; the slot mutexes it holds meanwhile live outside them (round 2 destroyed
    them while locked).  Twice in a row, and racing threads that poll options, must leave a usable library."""
    import threading
    import ctypes as C
    from cct_hip import _ffi
    L = _ffi.lib()
    assert L.cct_shutdown() == 0 and L.cct_shutdown() == 0
    stop = threading.Event()
    def poll():
        v = C.c_int(0)
        while not stop.is_set():
            assert L.cct_get_option(b"decode_slots", C.byref(v)) == 0
    ts = [threading.Thread(target=poll) for _ in range(3)]
    for t in ts:
        t.start()
    for _ in range(50):
        assert L.cct_shutdown() == 0
    stop.set()
    for t in ts:
        t.join()
    assert L.cct_version() == 1


def test_bench_traffic_figure_is_tied_to_the_kernel_source(tmp_path, monkeypatch):
    """bench.py prints the PMC traffic of the transform+pack stage only while the SHA-1 stored with it is the SHA-1 of
    encode_stream.hip; and the summary committed under profiles/ belongs to the source committed next to it."""
    import hashlib
    import json
    sys.path.insert(0, ROOT)
    import bench
    with open(bench.PIPE_SRC, "rb") as f:
        sha = hashlib.sha1(f.read()).hexdigest()
    with open(bench.PMC_JSON) as f:
        pmc = json.load(f)
    assert pmc["source_sha1"] == sha, "encode_stream.hip changed after the PMC passes: re-run tools/gpu_round_end.sh + collect_profiles.py"
    traffic, src = bench.pmc_traffic()
    assert traffic == pmc["traffic_bytes_per_launch"] and traffic > pmc["algorithmic_read_bytes"] and "r03_pmc_encode.json" in src
    stale = tmp_path / "pmc.json"
    stale.write_text(json.dumps(dict(pmc, source_sha1="0" * 40)))
    monkeypatch.setattr(bench, "PMC_JSON", str(stale))
    traffic, src = bench.pmc_traffic()
    assert traffic is None and src.startswith("stale")
    monkeypatch.setattr(bench, "PMC_JSON", str(tmp_path / "missing.json"))
    assert bench.pmc_traffic() == (None, None)


def test_bench_dump_outputs_fit_the_budget_and_hold_the_outputs(tmp_path):
    """bench.py --dump-outputs: the sampled slices depend on the arguments only, every workload's dump stays within 64 MB at
    the file bound, and the arrays written are float32 / float64 copies of the rasters and files handed over."""
    import zlib
    sys.path.insert(0, ROOT)
    import bench
    from cct_hip import _ffi
    L = _ffi.lib()
    for edge, n in set(bench.WORKLOADS.values()):
        bound = L.cct_file_bound(edge, edge, 16)
        s = bench.dump_sample(n, edge, edge, bound)
        assert np.array_equal(s, bench.dump_sample(n, edge, edge, bound)) and len(set(s.tolist())) == len(s) >= 1
        assert len(s) * 4 * (edge * edge + bound) + 3 * 8 * n + 8 * len(s) <= bench.DUMP_BUDGET
    rng = np.random.default_rng(0)
    rasters = rng.integers(0, 4096, size=(5, 16, 16)).astype(np.uint16)
    files = [rng.integers(0, 256, size=k).astype(np.uint8).tobytes() for k in (30, 1, 77, 5, 12)]
    offs = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.uint64)
    sizes = np.array([len(f) for f in files], np.uint32)
    s = bench.dump_sample(5, 16, 16, 100)
    bench.dump_outputs(str(tmp_path / "d"), s, rasters, np.frombuffer(b"".join(files), np.uint8), offs, sizes,
                       np.zeros(5, np.uint32))
    got = {p.stem: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["decoded_sample"], rasters[s]) and np.array_equal(got["encoded_sizes"], sizes)
    assert got["encoded_sample"].astype(np.uint8).tobytes() == b"".join(files[j] for j in s)
    assert got["encoded_crc32"].tolist() == [zlib.crc32(f) for f in files]
    assert got["decoded_crc32"].tolist() == [zlib.crc32(r.tobytes()) for r in rasters]
    bench.dump_outputs(str(tmp_path / "dec"), s, rasters)  # decode only: no encoded arrays
    assert sorted(p.stem for p in (tmp_path / "dec").iterdir()) == ["decoded_crc32", "decoded_sample", "sample_slices"]


def test_bench_workloads_and_sharding_follow_baseline_json():
    """The bench configurations are BASELINE.json's configs[1], [3], [4]; the corpus of configs[2] shards as DESIGN 8 says."""
    import json
    sys.path.insert(0, ROOT)
    import bench
    from cct_hip.parallel import shard_range
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    assert len(base["configs"]) >= 5
    assert bench.WORKLOADS == {2: (512, 256), 4: (1024, 512), 5: (512, 256)}
    sizes = [shard_range(3954, r, 8) for r in range(8)]
    assert [b - a for a, b in sizes] == [495, 495, 494, 494, 494, 494, 494, 494]
    assert sizes[0][0] == 0 and sizes[-1][1] == 3954 and all(sizes[i][1] == sizes[i + 1][0] for i in range(7))
