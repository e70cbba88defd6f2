#!/usr/bin/env python3
"""Fuzz run on the GPU box (test infrastructure, not collected by pytest): block sizes drawn uniformly from 3 to 64
(the run-time block size kernels for every size that is not a power of two), shapes the size divides, random images
(the generators of fuzz_gpu_vs_oracle.py) and random flags, through encode_batch / decode_batch, compared byte for byte
with the CPU oracle and decoded back.  Every few rounds the power-of-two sizes are forced through the run-time kernels
too (option "runtime_block_size").
Usage: python tests/fuzz_block_sizes.py [rounds] [seed]"""
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "2023-compact-image-compression_amd"), HERE]
import cct_hip  # noqa: E402
from cct_hip import _ffi  # noqa: E402
from fuzz_gpu_vs_oracle import image  # noqa: E402
from oracle import oracle  # noqa: E402


def shape(rng, bs):
    """w x h with bs | w * h and w * h <= 2^18."""
    w = int(rng.integers(8, 400))
    step = bs // math.gcd(w, bs)  # h must be a multiple of this
    k = int(rng.integers(1, max(2, (1 << 18) // (w * step) + 1)))
    return w, step * k


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.default_rng(seed)
    t0, nbad, ncase, sizes = time.time(), 0, 0, set()
    L = _ffi.lib()
    for r in range(rounds):
        bs = int(rng.integers(3, 65))
        w, h = shape(rng, bs)
        force = int(rng.integers(0, 4) == 0)
        cfg = cct_hip.default_config()
        cfg["block_size"] = bs
        t = cfg["encoder"]["transforms"]
        t["fractal"] = bool(rng.integers(0, 2))
        t["segmentation"] = bool(rng.integers(0, 4) > 0)
        cfg["encoder"]["deflate_compression"] = bool(rng.integers(0, 2))
        n = int(rng.integers(1, 6))
        imgs = np.stack([image(rng, w, h) for _ in range(n)])
        want = [oracle.encode(im, block_size=bs, fractal=t["fractal"], segmentation=t["segmentation"],
                              deflate=cfg["encoder"]["deflate_compression"]) for im in imgs]
        ncase += n
        sizes.add(bs)
        _ffi.check(L.cct_set_option(b"runtime_block_size", force))
        try:
            got = cct_hip.encode_batch(imgs, cfg)
            what = f"{w}x{h} bs {bs} {t} deflate {cfg['encoder']['deflate_compression']} forced {force}"
            if got != want:
                nbad += 1
                print(f"ENCODE MISMATCH round {r}: {what}", flush=True)
                continue
            back = np.asarray(cct_hip.decode_batch(got, cfg)).reshape(imgs.shape)
            if not np.array_equal(back, imgs):
                nbad += 1
                print(f"DECODE MISMATCH round {r}: {what}", flush=True)
        finally:
            _ffi.check(L.cct_set_option(b"runtime_block_size", 0))
        if r % 50 == 49:
            print(f"round {r + 1}/{rounds}  {time.time() - t0:.0f} s  slices {ncase}  mismatches: {nbad}", flush=True)
    print(("fuzz clean" if nbad == 0 else f"{nbad} MISMATCHES"), f"{rounds} rounds, {ncase} slices, {len(sizes)} block sizes,",
          f"{time.time() - t0:.0f} s", flush=True)
    sys.exit(1 if nbad else 0)


if __name__ == "__main__":
    main()
