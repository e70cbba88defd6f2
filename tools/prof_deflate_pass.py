"""Tuning harness (not part of the product): one DEFLATE batch (256 phantom token payloads) at (level, strategy), repeated,
from the package of the tree given as the first argument (to compare two builds).  Run it under
`rocprofv3 --kernel-trace --stats` for per-kernel times.

    python tools/prof_deflate_pass.py <tree root> <level> <strategy> <reps>
"""
import os
import sys
import zlib

ROOT = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(ROOT, "2023-compact-image-compression_amd")]
level, strategy, reps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
import numpy as np  # noqa: E402
import cct_hip  # noqa: E402
from cct_hip.synth import ct_phantom  # noqa: E402

imgs = np.stack([ct_phantom(i) for i in range(16)])
cfg = cct_hip.default_config()
cfg["verbose"] = False
cfg["encoder"]["deflate_compression"] = False
pl = [f[13:] for f in cct_hip.encode_batch(imgs, cfg)]
blobs = [pl[i % 16] for i in range(256)]
kw = {} if strategy == 0 else {"strategy": strategy}
for _ in range(reps):
    out = cct_hip.zlib_compress_batch(blobs, level=level, **kw)
c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
assert out[0] == c.compress(blobs[0]) + c.flush()
print("ok", level, strategy, sum(map(len, out)))
