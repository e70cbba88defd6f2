#!/usr/bin/env python3
"""Device JPEG 2000 lossless encoder on the 256 phantom slices of 512 x 512 uint16 that tools/bench_jpeg_lossless.py codes,
resident in HBM, and on the two real CT slices of tests/golden tiled to the same count.

jpeg2000_encode_batch(DeviceBuffer, precision=16, levels=5, codeblock=64 and 32).  The kernel times are the library's HIP
events (cct_last_timings [0]), median of --reps calls after a warm-up; the stages are timed by stopping the pipeline early
(CCT_J2K_STAGES = 1: convert and transform, 3: and Tier-1, 7: all) and taking differences: with the tuning build of the
library only (csrc/tuning.h), the release library gives the whole-call figures alone.  The call time is host wall clock
and includes the files crossing PCIe.  Beside them: the total bytes next to OpenJPEG's through Pillow for the same
parameters, and one core of Pillow encoding the same slices, the CPU baseline (times 16 for the threads a GPU job may use,
an extrapolation that assumes perfect scaling).  The first file of every set is decoded by Pillow where it has the codec.
One JSON line.

    python tools/bench_jpeg2000.py [--reps 5] [--slices 256] [--cpu-slices 8]
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


def median_ms(fn, reps, L):
    tm = (C.c_float * 6)()
    fn()  # warm-up: allocations, code objects
    kern, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        call.append((time.perf_counter() - t0) * 1e3)
        L.cct_last_timings(tm)
        kern.append(tm[0])
    return float(np.median(kern)), float(np.median(call))


def pillow_encode(img, codeblock):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG2000", irreversible=False, num_resolutions=6, codeblock_size=(codeblock, codeblock), no_jp2=True)
    return buf.getvalue()


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
    split = need_tuning_build("the stage split of tools/bench_jpeg2000.py", L)
    n = args.slices
    uniq = [ct_phantom(i) for i in range(min(n, 32))]
    real = [gi.load_slice("slice0671"), gi.load_slice("slice3706")]
    sets = {"phantoms": np.stack([uniq[i % len(uniq)] for i in range(n)]).astype(np.uint16),
            "real_tiled": np.stack([real[i % 2] for i in range(n)]).astype(np.uint16)}
    res = {"slices": n, "shape": [512, 512], "reps": args.reps, "pillow_jpeg2000": have_pillow}
    for name, imgs in sets.items():
        d_img = cct_hip.DeviceBuffer.from_numpy(imgs)
        mpix = imgs.size / 1e6
        for cb in (64, 32):
            def run():
                return cct_hip.jpeg2000_encode_batch(d_img, precision=16, levels=5, codeblock=cb, shape=imgs.shape)
            files = run()
            r = {"bytes": sum(map(len, files))}
            cum = {}
            try:
                for mask in (1, 3, 7) if split else (7,):
                    os.environ["CCT_J2K_STAGES"] = str(mask)
                    cum[mask], call = median_ms(run, args.reps, L)
            finally:
                os.environ.pop("CCT_J2K_STAGES", None)
            r.update(kernel_ms=cum[7], call_ms=call, kernel_mpix_s=mpix / (cum[7] / 1e3))
            if split:
                r.update(transform_ms=cum[1], tier1_ms=cum[3] - cum[1], tier2_ms=cum[7] - cum[3],
                         tier1_mpix_s=mpix / (max(cum[3] - cum[1], 1e-6) / 1e3))
            if have_pillow:
                from PIL import Image
                assert np.array_equal(np.array(Image.open(io.BytesIO(files[0]))), imgs[0]), "Pillow does not decode the file to the input"
                k = min(args.cpu_slices, n)
                t0 = time.perf_counter()
                ref = [pillow_encode(x, cb) for x in imgs[:k]]
                dt = time.perf_counter() - t0
                r.update(pillow_bytes_first=sum(map(len, ref)), device_bytes_first=sum(map(len, files[:k])), pillow_one_core_mpix_s=k * 512 * 512 / 1e6 / dt,
                         pillow_16_threads_mpix_s_extrapolated=16 * k * 512 * 512 / 1e6 / dt)
            res[f"{name}_cb{cb}"] = r
        d_img.free()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
