#!/usr/bin/env python3
"""Cost of the run-time block size kernels (encode_kernel<0>, decode_kernel<0>): device-event times of the transform+pack
stage (cct_encode_payload_dev) and of decode_kernel (cct_decode_payload_dev) on 64 phantoms of 768 x 768, for

    bs16_default  block size 16, the default paths (streaming encoder, tiled decode_kernel)
    bs16          block size 16, the kernels compiled for it (encode_kernel<16>, decode_kernel<16>: option tile_path 0)
    bs16_runtime  block size 16 forced through the run-time kernels (option runtime_block_size 1)
    bs12, bs48    the run-time kernels on sizes that are not powers of two

Every decoded batch is checked against the input.  Prints one JSON line (median milliseconds per batch).
    python tools/bench_block_sizes.py [--reps 20] [--slices 64] [--size 768]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2023-compact-image-compression_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--size", type=int, default=768)
    args = ap.parse_args()
    n, w = args.slices, args.size
    from cct_hip.synth import ct_phantom
    base = [ct_phantom(s, w) for s in range(8)]
    imgs = np.stack([base[i % 8] for i in range(n)])
    import cct_hip
    from cct_hip import _ffi, DeviceBuffer, Event, codec_params, decode_payload_dev, encode_payload_dev
    from cct_hip.batch import payload_stride
    L = _ffi.lib()
    d_img = DeviceBuffer.from_numpy(imgs)
    d_out = DeviceBuffer(imgs.nbytes)
    d_sz, d_st, d_dst = DeviceBuffer(4 * n), DeviceBuffer(4 * n), DeviceBuffer(4 * n)
    e0, e1 = Event(), Event()

    def timed(fn):
        ts = []
        for it in range(args.reps + 3):
            e0.record()
            fn()
            e1.record()
            ts.append(e1.elapsed_ms_since(e0))
        return float(np.median(ts[3:]))

    runs = [("bs16_default", 16, 1, 0), ("bs16", 16, 0, 0), ("bs16_runtime", 16, 0, 1), ("bs12", 12, 1, 0), ("bs48", 48, 1, 0)]
    res = {}
    for name, bs, tile, force in runs:
        cfg = cct_hip.default_config()
        cfg["block_size"] = bs
        params = codec_params(cfg, np.uint16)
        stride = payload_stride(w, w, bs)
        d_pay = DeviceBuffer(n * stride)
        _ffi.check(L.cct_set_option(b"tile_path", tile))
        _ffi.check(L.cct_set_option(b"runtime_block_size", force))
        try:
            enc_ms = timed(lambda: encode_payload_dev(d_img, n, w, w, params, d_pay, d_sz, d_st))
            enc_path = cct_hip_option(L, "last_encode_path")
            d_out.zero()
            dec_ms = timed(lambda: decode_payload_dev(d_pay, stride, d_sz, n, w, w, bs, True, d_out, d_dst))
            dec_path = cct_hip_option(L, "last_decode_path")
        finally:
            _ffi.check(L.cct_set_option(b"tile_path", 1))
            _ffi.check(L.cct_set_option(b"runtime_block_size", 0))
        ok = np.array_equal(d_out.download(np.uint16, imgs.size).reshape(imgs.shape), imgs)
        assert ok and not d_dst.download(np.uint32, n).any(), f"{name}: decode does not restore the input"
        res[name] = {"encode_ms": round(enc_ms, 4), "decode_ms": round(dec_ms, 4), "encode_path": enc_path,
                     "decode_path": dec_path, "payload_bytes": int(d_sz.download(np.uint32, n).sum())}
        d_pay.free()
    out = {"bench": "block_sizes", "slices": n, "size": w, "reps": args.reps, "device": cct_hip.device_info()["name"],
           "results": res,
           "runtime_over_compiled_bs16": {"encode": round(res["bs16_runtime"]["encode_ms"] / res["bs16"]["encode_ms"], 3),
                                          "decode": round(res["bs16_runtime"]["decode_ms"] / res["bs16"]["decode_ms"], 3)}}
    print(json.dumps(out), flush=True)


def cct_hip_option(L, key):
    import ctypes as C
    v = C.c_int(-9)
    L.cct_get_option(key.encode(), C.byref(v))
    return v.value


if __name__ == "__main__":
    main()
