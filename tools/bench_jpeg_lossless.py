#!/usr/bin/env python3
"""Device JPEG Lossless (SOF3; selection value 1 unless --jpl-predictor names another, or auto) codec, both directions, on the 256 phantom slices of 512 x 512 uint16 that
tools/bench_dicom_rle.py codes, resident in HBM.

Encode: jpeg_lossless_encode_batch(DeviceBuffer, precision=16); decode: jpeg_lossless_decode_batch(files, out_dev=DeviceBuffer).
The kernel times are the library's HIP events (cct_last_timings [0]: the five encode kernels, [4]: the decode kernels), median
of --reps calls after a warm-up; the call times are host wall clock and include what crosses PCIe (files down, files up).
Beside them: the algorithmic HBM bytes (rasters once, files once) at the 8 TB/s bench.py's roofline uses, and one core of
Pillow (libjpeg-turbo) decoding the 8-bit frames of the same slices (value >> 4, clipped to 255), which the device also codes
and decodes.  The first two files are checked against tests/jpeg_lossless_model.py and all round trip.  One JSON line.

With --jpl-predictor the encoder's kernel time and the file bytes can be taken per predictor; the JSON line names it, and
with auto how many frames chose which selection value.

    python tools/bench_jpeg_lossless.py [--reps 7] [--slices 256] [--jpl-predictor 1..7|auto]
"""
import argparse
import ctypes as C
import io
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slices", type=int, default=256)
    ap.add_argument("--jpl-predictor", choices=tuple("1234567") + ("auto",), default="1")
    args = ap.parse_args(argv)
    pred = 0 if args.jpl_predictor == "auto" else int(args.jpl_predictor)
    import cct_hip
    import jpeg_lossless_model as model
    from cct_hip.synth import ct_phantom
    L = cct_hip._ffi.lib()
    n = args.slices
    uniq = [ct_phantom(i) for i in range(min(n, 32))]
    imgs = np.stack([uniq[i % len(uniq)] for i in range(n)]).astype(np.uint16)
    _, rows, cols = imgs.shape
    res = {"slices": n, "shape": [rows, cols], "raster_bytes": int(imgs.nbytes), "reps": args.reps, "predictor": args.jpl_predictor}
    d_img = cct_hip.DeviceBuffer.from_numpy(imgs)
    d_out = cct_hip.DeviceBuffer(imgs.nbytes)
    files = cct_hip.jpeg_lossless_encode_batch(d_img, precision=16, shape=imgs.shape, predictor=pred)
    chosen = [f[f.index(b"\xff\xda") + 7] for f in files]  # Ss of the SOS
    assert files[:2] == [model.encode_frame(x, 16, predictor=s) for x, s in zip(imgs[:2], chosen)], "files differ from the model"
    assert pred == 0 or chosen == [pred] * n
    if pred == 0:
        res["frames_per_predictor"] = {str(s): chosen.count(s) for s in sorted(set(chosen))}
    file_bytes = sum(map(len, files))
    algo = imgs.nbytes + file_bytes
    res.update(frame_bytes=int(file_bytes), algorithmic_hbm_bytes=int(algo),
               algorithmic_ms_at_8TBps=round(algo / (HBM_PEAK_GBS * 1e9) * 1e3, 4))
    k, c = median_ms(lambda: cct_hip.jpeg_lossless_encode_batch(d_img, precision=16, shape=imgs.shape, predictor=pred), args.reps, L, 0)
    res["encode"] = {"kernels_ms": round(k, 3), "call_ms": round(c, 1), "GBps_algorithmic": round(algo / (k * 1e-3) / 1e9, 1)}
    k, c = median_ms(lambda: cct_hip.jpeg_lossless_decode_batch(files, rows, cols, out_dev=d_out), args.reps, L, 4)
    res["decode"] = {"kernels_ms": round(k, 3), "call_ms": round(c, 1), "GBps_algorithmic": round(algo / (k * 1e-3) / 1e9, 1)}
    assert np.array_equal(d_out.download(np.uint16, imgs.size).reshape(imgs.shape), imgs), "round trip"
    d_img.free()
    d_out.free()
    # the 8-bit frames: the device both ways, and one core of Pillow reading them
    low = np.minimum(imgs >> 4, 255).astype(np.uint8)
    files8 = cct_hip.jpeg_lossless_encode_batch(low, predictor=pred)
    res["frame_bytes_8bit"] = int(sum(map(len, files8)))
    k, c = median_ms(lambda: cct_hip.jpeg_lossless_decode_batch(files8, rows, cols, bits=8), args.reps, L, 4)
    res["decode_8bit"] = {"kernels_ms": round(k, 3), "call_ms": round(c, 1)}
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch(files8, rows, cols, bits=8), low), "8-bit round trip"
    try:
        from PIL import Image
        assert np.array_equal(np.array(Image.open(io.BytesIO(files8[0]))), low[0])
        t = []
        for _ in range(max(1, min(args.reps, 3))):
            t0 = time.perf_counter()
            for f in files8:
                Image.open(io.BytesIO(f)).load()
            t.append((time.perf_counter() - t0) * 1e3)
        res["pillow_decode_8bit_one_core_ms"] = round(float(np.median(t)), 1)
    except Exception as e:  # a Pillow whose libjpeg does not open SOF3
        res["pillow_decode_8bit_one_core_ms"] = None
        res["pillow_note"] = f"{type(e).__name__}: {e}"
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
