#!/usr/bin/env python3
"""Device PNG writer against Pillow: ms per batch of 256 phantom slices of 512 x 512 (value << 4, the reference's preview)
at compress_level 6 and 9.  Device: png_encode_batch from host rasters, median of --reps calls after a warm-up.  Pillow:
a thread pool of tools/evaluate.py's size over --pillow-slices slices, scaled to 256.  Also the DEFLATE pass alone (the
library's HIP events) over the same 256 filtered rasters with Z_FILTERED at memLevel 9 (wide sort records, what the PNG
writer runs) and at memLevel 8 with compact and with wide records: what compact records save on this input.
Per-kernel times (filter, DEFLATE kernels, pack): tools/prof_png_pass.py under rocprofv3.

With --depth 8: the 8-bit writer (png8_encode_batch, the same uint16 rasters through --window LO HI) next to the 16-bit
writer, the two alternating in one process, and Pillow's pool on the windowed bytes.

    python tools/bench_png.py [--reps 5] [--pillow-slices 32] [--depth 8 [--window 0 2000]]
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
sys.path[:0] = [os.path.join(ROOT, "2023-compact-image-compression_amd"), os.path.join(ROOT, "tests")]


def bench8(args, cct_hip, imgs, threads):
    import png8_model as p8
    win = tuple(args.window)
    res = {"batch": 256, "shape": [512, 512], "depth": 8, "window": list(win), "pillow_threads": threads}
    for level in (6, 9):
        out8 = cct_hip.png8_encode_batch(imgs, window=win, level=level)  # warm-up (graph capture, allocations)
        cct_hip.png_encode_batch(imgs, level=level, shift=4)
        t8, t16 = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out8 = cct_hip.png8_encode_batch(imgs, window=win, level=level)
            t8.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            out16 = cct_hip.png_encode_batch(imgs, level=level, shift=4)
            t16.append((time.perf_counter() - t0) * 1e3)
        k = args.pillow_slices
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as pool:
            ref = list(pool.map(lambda im: p8.pillow8_bytes(p8.window8(im, *win), level), imgs[:k]))
        pil_ms = (time.perf_counter() - t0) * 1e3 * 256 / k
        assert ref == out8[:k], "device PNGs differ from Pillow's"
        res[f"level{level}"] = {"device8_ms": round(float(np.median(t8)), 2), "device8_ms_min": round(min(t8), 2),
                                "device16_ms": round(float(np.median(t16)), 2), "device16_ms_min": round(min(t16), 2),
                                "pillow8_pool_ms_scaled": round(pil_ms, 1), "bytes8": int(sum(map(len, out8))),
                                "bytes16": int(sum(map(len, out16)))}
    print(json.dumps(res))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pillow-slices", type=int, default=32)
    ap.add_argument("--depth", type=int, default=16, choices=(8, 16))
    ap.add_argument("--window", type=int, nargs=2, default=(0, 2000), metavar=("LO", "HI"))
    args = ap.parse_args(argv)
    import cct_hip
    from cct_hip.synth import ct_phantom
    from PIL import Image
    imgs = np.stack([ct_phantom(i % 32) for i in range(256)])
    threads = max(1, min(8, os.cpu_count() or 1))  # tools/evaluate.py's pool
    if args.depth == 8:
        return bench8(args, cct_hip, imgs, threads)

    def pillow(img, level):
        buf = io.BytesIO()
        Image.fromarray((img.astype(np.uint32) << 4).astype(np.uint16)).save(buf, "PNG", compress_level=level)
        return buf.getvalue()
    res = {"batch": 256, "shape": [512, 512], "pillow_threads": threads}
    for level in (6, 9):
        out = cct_hip.png_encode_batch(imgs, level=level, shift=4)  # warm-up (graph capture, allocations)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = cct_hip.png_encode_batch(imgs, level=level, shift=4)
            ts.append((time.perf_counter() - t0) * 1e3)
        k = args.pillow_slices
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as pool:
            ref = list(pool.map(lambda im: pillow(im, level), imgs[:k]))
        pil_ms = (time.perf_counter() - t0) * 1e3 * 256 / k
        assert ref == out[:k], "device PNGs differ from Pillow's"
        res[f"level{level}"] = {"device_ms": round(float(np.median(ts)), 2), "device_ms_min": round(min(ts), 2),
                                "pillow_pool_ms_scaled": round(pil_ms, 1), "bytes": int(sum(map(len, out)))}
    import png_model as pm
    L = cct_hip._ffi.lib()
    rows = [pm.filter_rows(im, 4)[1] for im in imgs[:32]]
    rows = [rows[i % 32] for i in range(256)]
    tm = (C.c_float * 6)()
    passes = {}
    for label, mem_level, compact in (("memLevel9_wide", 9, 1), ("memLevel8_compact", 8, 1), ("memLevel8_wide", 8, 0)):
        for level in (6, 9):
            L.cct_set_option(b"deflate_compact_records", compact)
            try:
                cct_hip.zlib_compress_batch(rows, level=level, strategy=1, mem_level=mem_level)
                ts = []
                for _ in range(args.reps):
                    cct_hip.zlib_compress_batch(rows, level=level, strategy=1, mem_level=mem_level)
                    L.cct_last_timings(tm)
                    ts.append(tm[2])
            finally:
                L.cct_set_option(b"deflate_compact_records", 1)
            passes[f"{label}_level{level}_ms"] = round(float(np.median(ts)), 2)
    res["deflate_pass_filtered_rows"] = passes
    print(json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
