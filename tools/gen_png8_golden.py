#!/usr/bin/env python3
"""Writes tests/golden/png8.json: length and SHA-1 of the file Pillow writes for every case of tests/png8_model.py at
compress_level 4, 6 and 9 (Image.fromarray(uint8 samples).save(f, "PNG", compress_level=level)), with the Pillow version
that wrote them.  The 8-bit PNG tests compare the model and the device writer with it, so they also hold where Pillow is
not installed.

    python tools/gen_png8_golden.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import png8_model as p8  # noqa: E402


def main():
    import PIL
    files = {}
    for name in sorted(p8.cases()):
        smp = p8.samples_of(name)
        files[name] = {}
        for level in p8.LEVELS:
            png = p8.pillow8_bytes(smp, level)
            files[name][str(level)] = {"size": len(png), "sha1": hashlib.sha1(png).hexdigest()}
    out = {"pillow": PIL.__version__, "levels": list(p8.LEVELS), "files": files}
    path = os.path.join(ROOT, "tests", "golden", "png8.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(files)} cases x {len(p8.LEVELS)} levels")


if __name__ == "__main__":
    sys.exit(main())
