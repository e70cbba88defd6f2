#!/usr/bin/env python3
"""Tuning harness (not part of the product): the device DEFLATE pass alone at zlib levels 4 to 9, on two workloads of
256 strings each -- the token payloads of the bench phantoms (what the codec compresses) and raw 512x512 uint16 slices
(the ZIP column of the corpus evaluation, zlib.compress(raw)).  Prints one JSON line per (workload, level): median
DEFLATE pass time from the library's HIP events (cct_last_timings[2]) and the compressed bytes, checked against libz.
--strategies adds one line per (workload, level 9, zlib strategy 1 to 4), strategy 0 being the level lines.

    python tools/bench_deflate_levels.py [--reps 7] [--slices 256] [--levels 4,5,6,7,8,9] [--strategies [1,2,3,4]]
"""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2023-compact-image-compression_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slices", type=int, default=256)
    ap.add_argument("--levels", default="4,5,6,7,8,9")
    ap.add_argument("--strategies", nargs="?", const="1,2,3,4", default="",
                    help="zlib strategies at level 9 as well (Z_FILTERED 1, Z_HUFFMAN_ONLY 2, Z_RLE 3, Z_FIXED 4)")
    args = ap.parse_args()
    n = args.slices
    from bench import make_batches
    imgs = make_batches(0, n)[0]  # (before the GPU is initialised: the phantoms come from a process pool)
    import golden_inputs as gi
    raw = [gi.load_slice("slice0671").tobytes(), gi.load_slice("slice3706").tobytes()]
    import cct_hip
    from cct_hip import _ffi
    L = _ffi.lib()
    cfg = cct_hip.default_config()
    cfg["encoder"]["deflate_compression"] = False
    payloads = [f[13:] for f in cct_hip.encode_batch(imgs, cfg)]
    workloads = {"phantom_payloads": payloads, "raw_slices": [raw[i % 2] for i in range(n)]}
    tm = (C.c_float * 6)()
    runs = [(int(x), 0) for x in args.levels.split(",")]
    runs += [(9, int(x)) for x in args.strategies.split(",") if x]

    def libz(b, level, strategy):
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
        return c.compress(b) + c.flush()
    for wname, blobs in workloads.items():
        for level, strategy in runs:
            out = cct_hip.zlib_compress_batch(blobs, level=level, strategy=strategy)
            ok = all(o == libz(b, level, strategy) for o, b in zip(out[:16], blobs[:16]))  # (libz on all 256 takes long)
            times = []
            for _ in range(args.reps):
                cct_hip.zlib_compress_batch(blobs, level=level, strategy=strategy)
                L.cct_last_timings(tm)
                times.append(tm[2])
            print(json.dumps({"workload": wname, "n": n, "level": level, "strategy": strategy,
                              "deflate_ms_median": round(float(np.median(times)), 3),
                              "deflate_ms_min": round(min(times), 3), "in_bytes": sum(len(b) for b in blobs),
                              "out_bytes": sum(len(o) for o in out), "first16_equal_libz": ok}), flush=True)


if __name__ == "__main__":
    main()
