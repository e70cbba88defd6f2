"""Tuning harness (not part of the product): one DEFLATE batch of n phantom token payloads at level 9 with the option
tree_waves set, repeated; run it under `rocprofv3 --kernel-trace --stats` for the time of dfl_tree_kernel at that batch size
and setting (the sweeps behind the library's automatic rule).  CCT_HIP_LIB selects another library.

    python tools/prof_tree_waves.py <slices> <tree_waves: 0, 1 or 16; -1 leaves the option alone> <reps> [bytes]

bytes: every payload is cut to that many bytes, or repeated up to them (about one DEFLATE block per 21 KB of a phantom payload).
"""
import os
import statistics
import sys
import zlib
import ctypes as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "2023-compact-image-compression_amd")]
n, waves, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
cut = int(sys.argv[4]) if len(sys.argv) > 4 else None
import numpy as np  # noqa: E402
import cct_hip  # noqa: E402
from cct_hip import _ffi  # noqa: E402
from cct_hip.synth import ct_phantom  # noqa: E402

imgs = np.stack([ct_phantom(i) for i in range(16)])
cfg = cct_hip.default_config()
cfg["verbose"] = False
cfg["encoder"]["deflate_compression"] = False
pl = [f[13:] for f in cct_hip.encode_batch(imgs, cfg)]
if cut is not None:
    pl = [(p * (cut // len(p) + 1))[:cut] for p in pl]
blobs = [pl[i % 16] for i in range(n)]
if waves >= 0:
    _ffi.check(_ffi.lib().cct_set_option(b"tree_waves", waves))
t6, pass_ms = (C.c_float * 6)(), []
for _ in range(reps):
    out = cct_hip.zlib_compress_batch(blobs, level=9)
    _ffi.check(_ffi.lib().cct_last_timings(t6))
    pass_ms.append(t6[2])
assert out[0] == zlib.compress(blobs[0], 9)
print("ok", n, waves, len(blobs[0]), sum(map(len, out)), "pass_ms_median", round(statistics.median(pass_ms[reps // 3:]), 3))
