#!/usr/bin/env python3
"""Fuzz run (not part of the product): the device PNG writer and the memLevel 9 device DEFLATE against their models.
Every round encodes 1 to 4 random rasters of one random shape (1 to 700 rows, 1 to 20000 columns, up to ~2 MB of filtered
rows: streams that cross many window slides and end anywhere relative to the 256 CRC segments of a chunk) at a random
shift and compress_level, from the host or the device, sometimes with device_deflate 0, and compares each file with
tests/png_model.py byte for byte.  It also compresses 8 random byte strings at memLevel 9 with a random (level,
strategy) pair and compares them with zlib.compressobj(level, DEFLATED, 15, 9, strategy).
With --depth 8 the rounds run the 8-bit writer instead (png8_encode_batch): uint8 rasters, or uint16 rasters under a random
window (narrow, wide, w = 1, the full range), compared with Pillow itself (tests/png8_model.py where Pillow is missing).
Usage: python tools/fuzz_png.py [rounds] [seed] [--depth 8]"""
import ctypes as C
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2023-compact-image-compression_amd"), os.path.join(ROOT, "tests"),
                os.path.dirname(os.path.abspath(__file__))]
import cct_hip  # noqa: E402
import png_model as pm  # noqa: E402
from fuzz_codec import blob  # noqa: E402

PAIRS = ([(lv, s) for s in (0, 1, 4) for lv in (-1, 4, 5, 6, 7, 8, 9)] + [(lv, s) for s in (2, 3) for lv in range(1, 10)])


def raster(rng, rows, cols):
    kind = int(rng.integers(0, 6))
    if kind == 0:  # full 16-bit noise: stored-size blocks, window slides inside blocks
        return rng.integers(0, 65536, (rows, cols), dtype=np.uint16)
    if kind == 1:  # low-amplitude noise on a level
        return (rng.integers(0, int(rng.integers(1, 64)), (rows, cols)) + int(rng.integers(0, 60000))).astype(np.uint16)
    if kind == 2:  # smooth gradient + noise
        g = np.add.outer(np.arange(rows) * int(rng.integers(0, 50)), np.arange(cols) * int(rng.integers(0, 50)))
        return ((g + rng.integers(0, 8, (rows, cols))) & 0xFFFF).astype(np.uint16)
    if kind == 3:  # constant
        return np.full((rows, cols), int(rng.integers(0, 65536)), np.uint16)
    if kind == 4:  # sparse spikes on zeros
        a = np.zeros((rows, cols), np.uint16)
        m = rng.random((rows, cols)) < 0.01
        a[m] = rng.integers(0, 65536, int(m.sum()), dtype=np.uint16)
        return a
    return rng.integers(0, 4096, (rows, cols), dtype=np.uint16)  # 12-bit CT-like range


def window(rng):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return 0, 65535
    if kind == 1:  # w = 1 or 2
        lo = int(rng.integers(0, 65534))
        return lo, lo + int(rng.integers(1, 3))
    if kind == 2:  # CT-like
        lo = int(rng.integers(0, 3000))
        return lo, lo + int(rng.integers(50, 2500))
    lo = int(rng.integers(0, 65535))
    return lo, int(rng.integers(lo + 1, 65536))


def main8(rounds, seed):
    """--depth 8: png8_encode_batch against Pillow"""
    import png8_model as p8
    try:
        import PIL  # noqa: F401
        reference, against = p8.pillow8_bytes, "Pillow"
    except ImportError:
        reference, against = p8.png8_bytes, "the model (Pillow is not installed)"
    rng = np.random.default_rng(seed)
    L = cct_hip._ffi.lib()
    files = bad = 0
    t0 = time.time()
    for r in range(rounds):
        rows = int(rng.choice([1, 2, 3, 7, 64, 255, 256, 257, 511, 512, 700]))
        cols = int(rng.choice([1, 2, 7, 8, 9, 63, 64, 65, 255, 511, 512, 513, 519, 520, 1000, 4095, 16384, 16385, 20000]))
        while rows * (1 + cols) > 2_200_000:
            rows = max(1, rows // 2)
        n = int(rng.integers(1, 5))
        imgs = np.stack([raster(rng, rows, cols) for _ in range(n)])
        win = None
        if rng.random() < 0.35:  # uint8 sources
            imgs = (imgs >> int(rng.choice([0, 4, 8]))).astype(np.uint8)
            smp = imgs
        else:
            win = window(rng)
            smp = np.stack([p8.window8(im, *win) for im in imgs])
        level = int(rng.choice([-1, 4, 5, 6, 7, 8, 9]))
        host_defl = rng.random() < 0.15
        on_dev = rng.random() < 0.3
        if host_defl:
            L.cct_set_option(b"device_deflate", 0)
        try:
            if on_dev:
                out = cct_hip.png8_encode_batch(cct_hip.DeviceBuffer.from_numpy(imgs), window=win, level=level, shape=imgs.shape,
                                                dtype=imgs.dtype)
            else:
                out = cct_hip.png8_encode_batch(imgs, window=win, level=level)
        finally:
            L.cct_set_option(b"device_deflate", 1)
        with ThreadPoolExecutor(min(16, n)) as pool:
            want = list(pool.map(lambda im: reference(im, level), smp))
        for i in range(n):
            files += 1
            if out[i] != want[i]:
                bad += 1
                print(f"PNG8 MISMATCH round {r} slice {i}: {rows}x{cols} {imgs.dtype} window {win} level {level} "
                      f"device_images {on_dev} host_deflate {host_defl}")
        if (r + 1) % 10 == 0:
            print(f"round {r + 1}/{rounds}  {time.time() - t0:.0f} s  8-bit files {files}  mismatches: {bad}", flush=True)
    print(f"fuzz clean against {against}" if bad == 0 else f"fuzz FAILED: {bad} mismatches")
    return 1 if bad else 0


def main():
    argv = sys.argv[1:]
    depth = 16
    if "--depth" in argv:
        k = argv.index("--depth")
        depth = int(argv[k + 1])
        del argv[k:k + 2]
    if depth not in (8, 16):
        sys.exit("--depth takes 8 or 16")
    rounds = int(argv[0]) if len(argv) > 0 else 40
    seed = int(argv[1]) if len(argv) > 1 else 1
    if depth == 8:
        return main8(rounds, seed)
    rng = np.random.default_rng(seed)
    L = cct_hip._ffi.lib()
    files = streams = bad = 0
    t0 = time.time()
    for r in range(rounds):
        rows = int(rng.choice([1, 2, 3, 7, 64, 255, 256, 257, 511, 512, 700]))
        cols = int(rng.choice([1, 2, 3, 63, 64, 65, 255, 512, 1000, 4095, 16384, 16385, 20000]))
        while rows * (1 + 2 * cols) > 2_200_000:
            rows = max(1, rows // 2)
        n = int(rng.integers(1, 5))
        imgs = np.stack([raster(rng, rows, cols) for _ in range(n)])
        level = int(rng.choice([-1, 4, 5, 6, 7, 8, 9]))
        shift = int(rng.integers(0, 16))
        host_defl = rng.random() < 0.15
        on_dev = rng.random() < 0.3
        if host_defl:
            L.cct_set_option(b"device_deflate", 0)
        try:
            if on_dev:
                out = cct_hip.png_encode_batch(cct_hip.DeviceBuffer.from_numpy(imgs), level=level, shift=shift, shape=imgs.shape)
            else:
                out = cct_hip.png_encode_batch(imgs, level=level, shift=shift)
        finally:
            L.cct_set_option(b"device_deflate", 1)
        with ThreadPoolExecutor(min(16, n)) as pool:  # the model's zlib runs outside the GIL
            want = list(pool.map(lambda im: pm.png_bytes(im, level, shift), imgs))
        for i in range(n):
            files += 1
            if out[i] != want[i]:
                bad += 1
                print(f"PNG MISMATCH round {r} slice {i}: {rows}x{cols} level {level} shift {shift} device_images {on_dev} "
                      f"host_deflate {host_defl}")
        level, strategy = PAIRS[int(rng.integers(0, len(PAIRS)))]
        blobs = [blob(rng) for _ in range(8)]
        zs = cct_hip.zlib_compress_batch(blobs, level=level, strategy=strategy, mem_level=9)
        for i, b in enumerate(blobs):
            streams += 1
            c = zlib.compressobj(6 if level == -1 else level, zlib.DEFLATED, 15, 9, strategy)
            if zs[i] != c.compress(b) + c.flush():
                bad += 1
                print(f"ZLIB MISMATCH round {r} blob {i}: {len(b)} bytes level {level} strategy {strategy}")
        if (r + 1) % 10 == 0:
            print(f"round {r + 1}/{rounds}  {time.time() - t0:.0f} s  files {files}  memLevel-9 streams {streams}  mismatches: {bad}",
                  flush=True)
    print("fuzz clean" if bad == 0 else f"fuzz FAILED: {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
