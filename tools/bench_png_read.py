#!/usr/bin/env python3
"""Device PNG reader against Pillow, the counterpart of tools/bench_png.py: 256 phantom PNGs of 512 x 512 (value << 4, level 6,
as png_encode_batch writes them) -> rasters, shift 4.  Device: png_read_batch into host memory, median of --reps calls after a
warm-up, and the HIP-event times of its three stages (cct_last_timings: unpack = chunk CRCs + IDAT gather, INFLATE, unfilter)
from the same calls.  The unfilter kernel with 1, 2, 4 and 8 waves per image (option png_unfilter_waves), and its effective
bandwidth against the bytes it must move (rows * (1 + 2 cols) in, 2 rows cols out, per image).  Pillow, the yardstick and never
the code under test: Image.open(...).load() over the same files on a pool of 8 threads, measured in the same run.

    python tools/bench_png_read.py [--reps 5] [--pillow-files 256]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "2023-compact-image-compression_amd")]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pillow-files", type=int, default=256)
    args = ap.parse_args(argv)
    import cct_hip
    from cct_hip.synth import ct_phantom
    from PIL import Image
    L = cct_hip._ffi.lib()
    imgs = np.stack([ct_phantom(i % 32) for i in range(256)])
    files = cct_hip.png_encode_batch(imgs, level=6, shift=4)
    n, rows, cols = imgs.shape
    res = {"batch": n, "shape": [rows, cols], "file_bytes": int(sum(map(len, files))),
           "idat_chunks": int(sum(f.count(b"IDAT") for f in files))}
    tm = (C.c_float * 6)()
    moved = n * (rows * (1 + 2 * cols) + 2 * rows * cols)
    default_waves = C.c_int(0)
    L.cct_get_option(b"png_unfilter_waves", C.byref(default_waves))
    res["unfilter_waves_default"] = default_waves.value
    try:
        for waves in (1, 2, 4, 8, default_waves.value):
            assert L.cct_set_option(b"png_unfilter_waves", waves) == 0
            back = cct_hip.png_read_batch(files, shift=4)  # warm-up (allocations)
            assert np.array_equal(back, imgs), "the reader did not return the rasters"
            calls, stages = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                cct_hip.png_read_batch(files, shift=4)
                calls.append((time.perf_counter() - t0) * 1e3)
                L.cct_last_timings(tm)
                stages.append((tm[5], tm[3], tm[4]))
            unpack, inflate, unfilter = (float(np.median([s[k] for s in stages])) for k in range(3))
            entry = {"call_ms": round(float(np.median(calls)), 2), "call_ms_min": round(min(calls), 2),
                     "unpack_ms": round(unpack, 3), "inflate_ms": round(inflate, 3), "unfilter_ms": round(unfilter, 3),
                     "unfilter_GBps": round(moved / (unfilter * 1e-3) / 1e9, 1)}
            res[f"waves{waves}"] = entry
    finally:
        L.cct_set_option(b"png_unfilter_waves", default_waves.value)
    threads = 8  # the pool DESIGN 5a uses for the writer's yardstick
    k = min(args.pillow_files, n)

    def pillow(f):
        im = Image.open(io.BytesIO(f))
        im.load()
        return np.asarray(im)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        ref = list(pool.map(pillow, files[:k]))
    res["pillow_threads"] = threads
    res["pillow_pool_ms_scaled"] = round((time.perf_counter() - t0) * 1e3 * n / k, 1)
    assert all(np.array_equal(r >> 4, im) for r, im in zip(ref, imgs[:k]))
    print(json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
