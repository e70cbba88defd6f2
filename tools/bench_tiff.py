#!/usr/bin/env python3
"""Device TIFF writer and reader on 256 phantom slices of 512 x 512 uint16 resident in HBM, next to Pillow / libtiff on the host.

For every compression ("lzw", "deflate", "none") and predictor: tiff_encode_batch(DeviceBuffer) and
tiff_read_batch(files, out_dev=DeviceBuffer).  The kernel times are the library's HIP events (cct_last_timings [0]: staging,
LZW or DEFLATE, layout; [4]: LZW decode or gather + INFLATE, predictor), the call times host wall clock (they include what
crosses PCIe: files down, files up), both the median of --reps calls after a warm-up.  Pillow writes and reads the same
slices on one thread and on a 16-thread pool (--pillow-slices of them: a slice takes it tens of milliseconds), scaled to
the batch.  File sizes stand next to the device PNG writer's (level 6, shift 0).  Files are checked against Pillow's for
the first two slices, and every read against the rasters.  One JSON line at the end.

    python tools/bench_tiff.py [--reps 7] [--slices 256] [--pillow-slices 32]
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


def median_ms(fn, reps, L, slot):
    tm = (C.c_float * 6)()
    fn()  # warm-up: allocations, code objects, the DEFLATE graph
    kern, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        call.append((time.perf_counter() - t0) * 1e3)
        L.cct_last_timings(tm)
        kern.append(tm[slot])
    return float(np.median(kern)), float(np.median(call))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slices", type=int, default=256)
    ap.add_argument("--pillow-slices", type=int, default=32)
    args = ap.parse_args(argv)
    import cct_hip
    import tiff_model as model
    from PIL import Image
    from cct_hip.synth import ct_phantom
    L = cct_hip._ffi.lib()
    n = args.slices
    uniq = [ct_phantom(i) for i in range(min(n, 32))]
    imgs = np.stack([uniq[i % len(uniq)] for i in range(n)]).astype(np.uint16)
    _, rows, cols = imgs.shape
    d_img = cct_hip.DeviceBuffer.from_numpy(imgs)
    d_out = cct_hip.DeviceBuffer(imgs.nbytes)
    png_bytes = sum(map(len, cct_hip.png_encode_batch(d_img, level=6, shape=imgs.shape)))
    res = {"slices": n, "shape": [rows, cols], "raw_bytes": int(imgs.nbytes), "png_bytes": png_bytes, "runs": []}
    k = min(n, args.pillow_slices)
    for comp, pred in (("lzw", 1), ("lzw", 2), ("deflate", 1), ("deflate", 2), ("none", 1)):
        files = cct_hip.tiff_encode_batch(d_img, comp, pred, shape=imgs.shape)
        if comp != "none":
            assert all(model.same_file(f, model.pillow_file(x, comp, pred)) for f, x in zip(files[:2], imgs[:2])), "files differ from Pillow's"
        enc_k, enc_c = median_ms(lambda: cct_hip.tiff_encode_batch(d_img, comp, pred, shape=imgs.shape), args.reps, L, 0)
        dec_k, dec_c = median_ms(lambda: cct_hip.tiff_read_batch(files, rows, cols, out_dev=d_out), args.reps, L, 4)
        assert np.array_equal(d_out.download(np.uint16, imgs.size).reshape(imgs.shape), imgs), "read differs from the rasters"
        run = {"compression": comp, "predictor": pred, "file_bytes": sum(map(len, files)),
               "encode_kernels_ms": round(enc_k, 3), "encode_call_ms": round(enc_c, 3), "read_kernels_ms": round(dec_k, 3),
               "read_call_ms": round(dec_c, 3), "encode_kernels_GBs": round(imgs.nbytes / enc_k / 1e6, 1),
               "read_kernels_GBs": round(imgs.nbytes / dec_k / 1e6, 1)}
        if comp != "none":
            kw = dict(compression={"lzw": "tiff_lzw", "deflate": "tiff_adobe_deflate"}[comp], tiffinfo={317: 2} if pred == 2 else {})

            def save(x):
                buf = io.BytesIO()
                Image.fromarray(x).save(buf, "TIFF", **kw)
                return buf.getvalue()

            def load(f):
                return np.array(Image.open(io.BytesIO(f)))

            for threads in (1, 16):
                with ThreadPoolExecutor(threads) as pool:
                    t0 = time.perf_counter()
                    pf = list(pool.map(save, imgs[:k]))
                    t1 = time.perf_counter()
                    back = list(pool.map(load, pf))
                    t2 = time.perf_counter()
                assert np.array_equal(np.stack(back), imgs[:k])
                run[f"pillow_{threads}t_write_ms"] = round((t1 - t0) * 1e3 * n / k, 1)
                run[f"pillow_{threads}t_read_ms"] = round((t2 - t1) * 1e3 * n / k, 1)
        res["runs"].append(run)
        print(run, flush=True)
    d_img.free(); d_out.free()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
