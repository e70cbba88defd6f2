#!/usr/bin/env python3
"""Debug aid: stage (i) through the pipeline (tile_path 1) and the generic kernel (0) on a few slices; prints where the
block roles / sizes / payload bytes first differ.  DBG=mask sets option debug_skip (tuning build only)."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2023-compact-image-compression_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import golden_inputs as gi
import cct_hip
from cct_hip import _ffi, DeviceBuffer, codec_params, encode_payload_dev
from cct_hip.batch import payload_stride
from _inputs import need_tuning_build

n_px = int(sys.argv[1]) if len(sys.argv) > 1 else 256
n = 3
imgs = np.stack([gi.ct_phantom(40 + i, n_px) for i in range(n)])
L = _ffi.lib()
if not need_tuning_build("tools/debug/cmp_paths.py (option debug_skip, DBG=mask)", L):
    sys.exit(2)
cfg = cct_hip.default_config()
w = h = n_px
nb = w * h // 16
stride = payload_stride(w, h, 16)
d_img = DeviceBuffer.from_numpy(imgs)
res = {}
L.cct_set_option(b"debug_skip", int(os.environ.get("DBG", "0")))
for path in (1, 0):
    L.cct_set_option(b"tile_path", path)
    d_pay, d_sz, d_st = DeviceBuffer(n * stride), DeviceBuffer(4 * n), DeviceBuffer(4 * n)
    d_stats, d_roles = DeviceBuffer(16 * n), DeviceBuffer(n * nb)
    d_pay.zero()
    encode_payload_dev(d_img, n, w, h, codec_params(cfg, imgs.dtype), d_pay, d_sz, d_st, d_stats, d_roles)
    sizes = d_sz.download(np.uint32, n)
    res[path] = (sizes, d_st.download(np.uint32, n), d_stats.download(np.uint32, 4 * n).reshape(n, 4),
                 d_roles.download(np.uint8, n * nb).reshape(n, nb),
                 [d_pay.download(np.uint8, int(max(sizes[i], 1)), offset=i * stride) for i in range(n)])
L.cct_set_option(b"tile_path", 1)
a, b = res[1], res[0]
print("sizes", a[0], b[0]); print("status", a[1], b[1]); print("stats pipe", a[2].tolist(), "generic", b[2].tolist())
for i in range(n):
    d = np.nonzero(a[3][i] != b[3][i])[0]
    print(f"slice {i}: {len(d)} role differences; first", [(int(x), int(x) >> 8, int(a[3][i][x]), int(b[3][i][x])) for x in d[:8]])
    m = min(len(a[4][i]), len(b[4][i]))
    pd = np.nonzero(a[4][i][:m] != b[4][i][:m])[0]
    print(f"   payload: first difference at {int(pd[0]) if len(pd) else None} of {m}")
