"""Tuning harness (not part of the product): one DEFLATE batch (256 phantom token payloads) at (level, strategy), repeated,
from the package of the tree given as the first argument (to compare two builds; CCT_HIP_LIB selects another library).  Prints
the median wall time of a call and of the pass inside it (cct_last_timings); run it under `rocprofv3 --kernel-trace --stats`
for per-kernel times.

    python tools/prof_deflate_pass.py <tree root> <level> <strategy> <reps>
"""
import ctypes as C
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(ROOT, "2023-compact-image-compression_amd")]
level, strategy, reps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
import numpy as np  # noqa: E402
import cct_hip  # noqa: E402
from cct_hip import _ffi  # noqa: E402
from cct_hip.synth import ct_phantom  # noqa: E402

imgs = np.stack([ct_phantom(i) for i in range(16)])
cfg = cct_hip.default_config()
cfg["verbose"] = False
cfg["encoder"]["deflate_compression"] = False
pl = [f[13:] for f in cct_hip.encode_batch(imgs, cfg)]
blobs = [pl[i % 16] for i in range(256)]
kw = {} if strategy == 0 else {"strategy": strategy}
ms, pass_ms = [], []
t6 = (C.c_float * 6)()
for _ in range(reps):
    t0 = time.perf_counter()
    out = cct_hip.zlib_compress_batch(blobs, level=level, **kw)
    ms.append((time.perf_counter() - t0) * 1e3)
    _ffi.check(_ffi.lib().cct_last_timings(t6))
    pass_ms.append(t6[2])  # the pass between its two events, without the copies of the call
c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
assert out[0] == c.compress(blobs[0]) + c.flush()
# (medians without the first third of the calls, which allocate and capture)
print("ok", level, strategy, sum(map(len, out)), "call_ms_median", round(statistics.median(ms[reps // 3:]), 3),
      "pass_ms_median", round(statistics.median(pass_ms[reps // 3:]), 3))
