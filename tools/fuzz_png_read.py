#!/usr/bin/env python3
"""Random PNG files against the device PNG reader: random shapes, depths 8 and 16, a random filter type per row, random IDAT
cuts (empty chunks included), ancillary chunks, zlib levels 0 .. 9, strategies 0 .. 4 and wbits 9 .. 15, read into host memory
and into a DeviceBuffer with a random shift, and compared with the generator's input (tests/png_files.py builds the files).

    python tools/fuzz_png_read.py [--seed 1] [--batches 40] [--files 12]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "2023-compact-image-compression_amd"), os.path.join(ROOT, "tests")]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--files", type=int, default=12)
    args = ap.parse_args(argv)
    import cct_hip
    import png_files as pf
    rng = np.random.default_rng(args.seed)
    done = {"files": 0, "chunks": 0, "pixels": 0, "shapes": []}
    for b in range(args.batches):
        rows = int(rng.choice([1, 2, 3, 63, 64, 65, 127, 128, 129, int(rng.integers(1, 400))]))
        cols = int(rng.choice([1, 2, 3, 63, 64, 65, 127, 128, 129, int(rng.integers(1, 700))]))
        files, want = [], []
        for _ in range(args.files):
            depth = int(rng.choice([8, 16]))
            hi = int(rng.choice([2, 7, 1 << depth]))
            img = rng.integers(0, hi, (rows, cols), dtype=np.uint16)
            if depth == 16 and hi < 256 and rng.random() < 0.5:
                img = (img * 257).astype(np.uint16)
            types = rng.integers(0, 5, rows)
            z = pf.deflate(pf.filtered(img, depth, types), int(rng.integers(0, 10)), int(rng.integers(9, 16)), int(rng.integers(0, 5)))
            ncut = int(rng.integers(0, 6))
            cuts = sorted(int(x) for x in rng.integers(0, len(z) + 1, ncut))
            cuts = [c - p for p, c in zip([0] + cuts, cuts)] if ncut else None
            if rng.random() < 0.1:
                cuts = int(rng.integers(1, 9)) if len(z) < 3000 else cuts
            anc = [(b"tEXt", bytes(rng.integers(1, 255, int(rng.integers(0, 300)), dtype=np.uint8)))] if rng.random() < 0.4 else []
            f = pf.make_png(img, depth, types, cuts=cuts, before=anc if rng.random() < 0.5 else (), after=anc, stream=z)
            files.append(f)
            want.append(img)
            done["chunks"] += f.count(b"IDAT")
        want = np.stack(want)
        shift = int(rng.integers(0, 16))
        host = cct_hip.png_read_batch(files, shift=shift)
        d = cct_hip.DeviceBuffer(want.nbytes + 4096)
        d.upload(np.full(want.size + 2048, 0x5A5A, np.uint16))
        d.nbytes = want.nbytes
        assert cct_hip.png_read_batch(files, shift=shift, out_dev=d) == want.shape
        d.nbytes = want.nbytes + 4096
        dev = d.download(np.uint16, want.size + 2048)
        assert np.array_equal(host, want >> shift), f"batch {b}: host output differs ({rows} x {cols}, shift {shift})"
        assert np.array_equal(dev[:want.size].reshape(want.shape), want >> shift), f"batch {b}: device output differs"
        assert np.all(dev[want.size:] == 0x5A5A), f"batch {b}: bytes behind the last raster were written"
        done["files"] += len(files)
        done["pixels"] += int(want.size)
        done["shapes"].append([rows, cols])
    print(json.dumps({"seed": args.seed, "batches": args.batches, **done, "result": "all equal"}))


if __name__ == "__main__":
    sys.exit(main())
