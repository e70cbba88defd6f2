"""Tuning harness (not part of the product): the device PNG writer on 256 phantom slices of 512 x 512 (value << 4), repeated,
from the package of the tree given as the first argument.  Prints the median wall time of a call; run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel split (png_filter_kernel, the dfl_* kernels, png_pack_kernel).

    python tools/prof_png_pass.py <tree root> <level> <reps>
"""
import os
import statistics
import sys
import time

ROOT = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(ROOT, "2023-compact-image-compression_amd")]
level, reps = int(sys.argv[2]), int(sys.argv[3])
import numpy as np  # noqa: E402
import cct_hip  # noqa: E402
from cct_hip.synth import ct_phantom  # noqa: E402

imgs = np.stack([ct_phantom(i % 32) for i in range(256)])
ms = []
for _ in range(reps):
    t0 = time.perf_counter()
    out = cct_hip.png_encode_batch(imgs, level=level, shift=4)
    ms.append((time.perf_counter() - t0) * 1e3)
print("ok", level, sum(map(len, out)), "call_ms_median", round(statistics.median(ms[reps // 3:]), 3))  # (the first calls allocate and capture)
