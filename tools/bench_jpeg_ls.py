#!/usr/bin/env python3
"""Device JPEG-LS lossless codec, both directions, on the 256 phantom slices of 512 x 512 uint16 that
tools/bench_dicom_rle.py and tools/bench_jpeg_lossless.py code, resident in HBM.

For restart_rows 0, 16 and 64: jpeg_ls_encode_batch(DeviceBuffer, precision=16, restart_rows=..) and
jpeg_ls_decode_batch(files, out_dev=DeviceBuffer).  The kernel times are the library's HIP events (cct_last_timings [0]: the
three encode kernels, [4]: the decode kernel), median of --reps calls after a warm-up; the call times are host wall clock
and include what crosses PCIe (files down, files up).  The first two files of every setting are checked against
tests/jpeg_ls_model.py and all round trip.  The encoder codes the regular samples of a 64-sample step in as many rounds as
the step's busiest context has samples: `rounds` counts them for the first --round-slices slices, on the host, from the
same parse the kernel makes (rounds_per_step below).  One JSON line.

    python tools/bench_jpeg_ls.py [--reps 7] [--slices 256] [--round-slices 8]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "2023-compact-image-compression_amd"), os.path.join(ROOT, "tests")]
HBM_PEAK_GBS = 8000.0  # bench.py


def median_ms(fn, reps, L, slot):
    tm = (C.c_float * 6)()
    fn()  # warm-up: allocations, code objects
    kern, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        call.append((time.perf_counter() - t0) * 1e3)
        L.cct_last_timings(tm)
        kern.append(tm[slot])
    return float(np.median(kern)), float(np.median(call))


def regular_samples(img, precision, model):
    """-> (context 1 .. 364 of every sample, whether it is coded in regular mode), one restart interval.  The contexts come
    from the input samples alone; which samples are in run mode comes from the line's parse (a run starts where all
    gradients are zero and lasts while a sample equals the one to its left; the sample that ends it is coded apart)."""
    p = model.Params(precision)
    x = img.astype(np.int64)
    rows, cols = x.shape
    above = np.vstack([np.zeros((1, cols), np.int64), x[:-1]])
    rb = above
    rd = np.hstack([above[:, 1:], above[:, -1:]])
    rc = np.hstack([np.vstack([np.zeros((2, 1), np.int64), x[:-2, :1]])[:rows], above[:, :-1]])
    ra = np.hstack([rb[:, :1], x[:, :-1]])

    def quant(d):
        q = np.zeros(d.shape, np.int64)
        for t in (p.t1, p.t2, p.t3):
            q += (d >= t).astype(np.int64) - (d <= -t).astype(np.int64)
        return q + (d > 0).astype(np.int64) - (d < 0).astype(np.int64)

    q = 81 * quant(rd - rb) + 9 * quant(rb - rc) + quant(rc - ra)
    ctx = np.abs(q)
    eq = x == ra
    regular = np.zeros((rows, cols), bool)
    for r in range(rows):
        zero = np.flatnonzero(ctx[r] == 0)
        differs = np.flatnonzero(~eq[r])
        c = 0
        while c < cols:
            k = np.searchsorted(zero, c)
            s = int(zero[k]) if k < len(zero) else cols
            regular[r, c:s] = True
            if s >= cols:
                break
            k = np.searchsorted(differs, s)
            c = int(differs[k]) + 1 if k < len(differs) else cols  # behind the interruption sample
    return ctx, regular


def rounds_per_step(img, precision, model):
    """-> [rounds of every 64-sample step of the raster that has a regular sample]: the largest number of regular-mode
    samples of the step that share a context"""
    ctx, regular = regular_samples(img, precision, model)
    out = []
    for r in range(img.shape[0]):
        for c0 in range(0, img.shape[1], 64):
            cc = ctx[r, c0:c0 + 64][regular[r, c0:c0 + 64]]
            if len(cc):
                out.append(int(np.bincount(cc).max()))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slices", type=int, default=256)
    ap.add_argument("--round-slices", type=int, default=8)
    args = ap.parse_args(argv)
    import cct_hip
    import jpeg_ls_model as model
    from cct_hip.synth import ct_phantom
    L = cct_hip._ffi.lib()
    n = args.slices
    uniq = [ct_phantom(i) for i in range(min(n, 32))]
    imgs = np.stack([uniq[i % len(uniq)] for i in range(n)]).astype(np.uint16)
    _, rows, cols = imgs.shape
    res = {"slices": n, "shape": [rows, cols], "raster_bytes": int(imgs.nbytes), "reps": args.reps}
    rounds = [v for x in imgs[:args.round_slices] for v in rounds_per_step(x, 16, model)]
    if rounds:
        res["rounds"] = {"slices": min(n, args.round_slices), "steps": len(rounds), "mean": round(float(np.mean(rounds)), 2), "max": int(max(rounds))}
    d_img = cct_hip.DeviceBuffer.from_numpy(imgs)
    d_out = cct_hip.DeviceBuffer(imgs.nbytes)
    for rr in (0, 16, 64):
        files = cct_hip.jpeg_ls_encode_batch(d_img, precision=16, shape=imgs.shape, restart_rows=rr)
        assert files[:2] == [model.encode_frame(x, 16, rr) for x in imgs[:2]], "files differ from the model"
        file_bytes = sum(map(len, files))
        algo = imgs.nbytes + file_bytes
        one = {"file_bytes": int(file_bytes), "algorithmic_ms_at_8TBps": round(algo / (HBM_PEAK_GBS * 1e9) * 1e3, 4)}
        k, c = median_ms(lambda: cct_hip.jpeg_ls_encode_batch(d_img, precision=16, shape=imgs.shape, restart_rows=rr), args.reps, L, 0)
        one["encode"] = {"kernels_ms": round(k, 3), "call_ms": round(c, 1)}
        k, c = median_ms(lambda: cct_hip.jpeg_ls_decode_batch(files, rows, cols, out_dev=d_out), args.reps, L, 4)
        one["decode"] = {"kernels_ms": round(k, 3), "call_ms": round(c, 1)}
        assert np.array_equal(d_out.download(np.uint16, imgs.size).reshape(imgs.shape), imgs), "round trip"
        res[f"restart_rows_{rr}"] = one
    d_img.free()
    d_out.free()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
