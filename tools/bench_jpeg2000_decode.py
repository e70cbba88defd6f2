#!/usr/bin/env python3
"""Device JPEG 2000 lossless decoder on the files tools/bench_jpeg2000.py writes: the 256 phantom slices of 512 x 512 uint16
and the two real CT slices of tests/golden tiled to the same count, at code-blocks of 64 and 32, 5 levels.

jpeg2000_decode_batch(files, out_dev=DeviceBuffer).  The kernel times are the library's HIP events (cct_last_timings [4]),
median of --reps calls after a warm-up; the stages are timed by stopping the pipeline early (CCT_J2K_DEC_STAGES = 1: packet
parse, 3: and Tier-1, 7: and the inverse transform, 15: all) and taking differences.  The call time is host wall clock and
includes the marker walk and the files crossing PCIe.  Beside them, measured in the same run: the encoder's kernel time and
its Tier-1 for the same slices (the CCT_J2K_STAGES split of tools/bench_jpeg2000.py), and one core of Pillow decoding the
same files, the CPU baseline.  The rasters are compared with the input before anything is timed.  One JSON line.

    python tools/bench_jpeg2000_decode.py [--reps 5] [--slices 256] [--cpu-slices 8]
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
sys.path[:0] = [os.path.join(ROOT, "2023-compact-image-compression_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


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


def staged(fn, reps, L, slot, var, masks):
    cum = {}
    try:
        for mask in masks:
            os.environ[var] = str(mask)
            cum[mask], call = median_ms(fn, reps, L, slot)
    finally:
        os.environ.pop(var, None)
    return cum, call


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slices", type=int, default=256)
    ap.add_argument("--cpu-slices", type=int, default=8)
    args = ap.parse_args(argv)
    import cct_hip
    import golden_inputs as gi
    from cct_hip.synth import ct_phantom
    try:
        from PIL import features
        have_pillow = bool(features.check_codec("jpg_2000"))
    except Exception:
        have_pillow = False
    from _inputs import need_tuning_build
    L = cct_hip._ffi.lib()
    split = need_tuning_build("the stage split of tools/bench_jpeg2000_decode.py", L)  # else: the whole-call figures alone
    n = args.slices
    uniq = [ct_phantom(i) for i in range(min(n, 32))]
    real = [gi.load_slice("slice0671"), gi.load_slice("slice3706")]
    sets = {"phantoms": np.stack([uniq[i % len(uniq)] for i in range(n)]).astype(np.uint16),
            "real_tiled": np.stack([real[i % 2] for i in range(n)]).astype(np.uint16)}
    res = {"slices": n, "shape": [512, 512], "reps": args.reps, "pillow_jpeg2000": have_pillow}
    d_out = cct_hip.DeviceBuffer(n * 512 * 512 * 2)
    for name, imgs in sets.items():
        d_img = cct_hip.DeviceBuffer.from_numpy(imgs)
        mpix = imgs.size / 1e6
        for cb in (64, 32):
            def enc():
                return cct_hip.jpeg2000_encode_batch(d_img, precision=16, levels=5, codeblock=cb, shape=imgs.shape)
            files = enc()

            def dec():
                return cct_hip.jpeg2000_decode_batch(files, 512, 512, out_dev=d_out)
            assert np.array_equal(cct_hip.jpeg2000_decode_batch(files, 512, 512), imgs), "the device does not decode its files to the input"
            r = {"bytes": sum(map(len, files))}
            cum, call = staged(dec, args.reps, L, 4, "CCT_J2K_DEC_STAGES", (1, 3, 7, 15) if split else (15,))
            ecum, ecall = staged(enc, args.reps, L, 0, "CCT_J2K_STAGES", (1, 3, 7) if split else (7,))
            r.update(kernel_ms=cum[15], call_ms=call, kernel_mpix_s=mpix / (cum[15] / 1e3), call_mpix_s=mpix / (call / 1e3),
                     encoder_kernel_ms=ecum[7], encoder_call_ms=ecall)
            if split:
                r.update(parse_ms=cum[1], tier1_ms=cum[3] - cum[1], idwt_ms=cum[7] - cum[3], finish_ms=cum[15] - cum[7],
                         encoder_tier1_ms=ecum[3] - ecum[1], tier1_decode_over_encode=(cum[3] - cum[1]) / max(ecum[3] - ecum[1], 1e-6))
            if have_pillow:
                from PIL import Image
                k = min(args.cpu_slices, n)
                t0 = time.perf_counter()
                back = [np.array(Image.open(io.BytesIO(f))) for f in files[:k]]
                dt = time.perf_counter() - t0
                assert all(np.array_equal(b, x) for b, x in zip(back, imgs))
                r.update(pillow_one_core_mpix_s=k * 512 * 512 / 1e6 / dt, pillow_16_threads_mpix_s_extrapolated=16 * k * 512 * 512 / 1e6 / dt)
            res[f"{name}_cb{cb}"] = r
        d_img.free()
    d_out.free()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
