#!/usr/bin/env python3
"""Generate the block-size fixtures, tests/golden/block_sizes.json (+ .cct files of the small cases under
tests/golden/block_sizes/), by running the REFERENCE codec on block sizes that are not powers of two.

Run:  python3 -B tools/gen_block_size_golden.py REFERENCE_CHECKOUT
The reference (taaha-khan/2023-CompaCT-Image-Compression, pure Python) is imported from REFERENCE_CHECKOUT/src as
oracle/gen_golden.py imports it; only DATA is written: input recipes (tests/block_size_inputs.py), the reference's
outputs (bytes, or SHA-1 + length), its token counts, its jump table and the SHA-1 of its decoded raster.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_inputs as gi  # noqa: E402
import block_size_inputs as bsi  # noqa: E402

OUT_DIR = os.path.join(gi.GOLDEN, "block_sizes")
STORE_MAX = 16 * 1024  # .cct files up to this size are stored, larger outputs as SHA-1 + length, except these:
STORE_ALSO = {"crop192x160_bs5", "crop192x160_bs15", "crop192x160_bs60", "crop192x160_bs12_f1s1d0", "crop192x160_bs12_f0s1d1",
              "noise168x180_bs3", "noise168x180_bs5", "noise168x180_bs12"}


def run_case(ref, name, inp, over, store=True):
    Encoder, Decoder, base_cfg = ref
    cfg = json.loads(json.dumps(base_cfg))
    cfg["verbose"] = False
    cfg["block_size"] = over["block_size"]
    for k in ("fractal", "segmentation"):
        if k in over:
            cfg["encoder"]["transforms"][k] = over[k]
    if "deflate" in over:
        cfg["encoder"]["deflate_compression"] = over["deflate"]
    img = bsi.build_input(inp)
    t0 = time.time()
    enc = Encoder(cfg, img, None)
    out = enc.encode()
    case = {"name": name, "input": inp, "input_sha1": gi.sha1(img.tobytes()), "shape": list(img.shape),
            "dtype": str(img.dtype), "config": over, "len": len(out), "sha1": gi.sha1(out),
            "tokens": {"short": int(enc.info["delta"]), "full": int(enc.info["full"])}}
    if cfg["encoder"]["transforms"]["segmentation"]:
        _, jumps = enc.partition.block_partition()
        case["tokens"]["jump"] = len(jumps)
        case["jumps_sha1"] = gi.sha1(np.array(sorted(jumps.items()), dtype=np.int32).reshape(-1, 2).tobytes())
    dec = Decoder(cfg, out, None).decode()
    case["decoded_sha1"] = gi.sha1(dec)
    assert dec == img.tobytes(), f"{name}: the reference does not round-trip"
    if store and (len(out) <= STORE_MAX or name in STORE_ALSO):
        fn = name + ".cct"
        with open(os.path.join(OUT_DIR, fn), "wb") as f:
            f.write(out)
        case["file"] = "block_sizes/" + fn
    print(f"{name:32s} len {len(out):8d} {case['tokens']} ({time.time() - t0:.1f}s)", flush=True)
    return case


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_root = sys.argv[1]
    sys.path.insert(0, os.path.join(ref_root, "src"))
    import warnings
    warnings.simplefilter("ignore")
    from codec.core import Encoder, Decoder  # the reference
    with open(os.path.join(ref_root, "src", "config.json")) as f:
        ref = (Encoder, Decoder, json.load(f))
    os.makedirs(OUT_DIR, exist_ok=True)

    crop96 = {"kind": "slice", "name": "slice0671", "crop": [200, 296, 200, 296]}
    crop192x160 = {"kind": "slice", "name": "slice3706", "crop": [160, 352, 176, 336]}
    noisy = lambda n, w, h, seed: {"kind": "phantom_noise", "seed": seed, "n": n, "amp": 90, "shape": [w, h]}  # noqa: E731
    cases = []
    for bs in (3, 6, 12, 24, 48):
        cases.append(run_case(ref, f"crop96_bs{bs}", crop96, {"block_size": bs}))
    for bs in (5, 10, 15, 20, 30, 40, 60):
        cases.append(run_case(ref, f"crop192x160_bs{bs}", crop192x160, {"block_size": bs}))
    for fr in (1, 0):
        for sg in (1, 0):
            for df in (1, 0):
                cases.append(run_case(ref, f"crop192x160_bs12_f{fr}s{sg}d{df}", crop192x160,
                                      {"block_size": 12, "fractal": bool(fr), "segmentation": bool(sg), "deflate": bool(df)}))
    for bs in (5, 10, 20, 25, 50):
        cases.append(run_case(ref, f"noise20x20_bs{bs}", noisy(64, 20, 20, 11), {"block_size": bs}))
    for bs in (15, 60):
        cases.append(run_case(ref, f"noise48x80_bs{bs}", noisy(96, 48, 80, 12), {"block_size": bs}))
    # meshing at small sizes: >= 100 jumps per slice
    for bs in (3, 5, 6, 7, 9, 10, 12, 14):
        cases.append(run_case(ref, f"noise168x180_bs{bs}", noisy(180, 168, 180, 13), {"block_size": bs}))
    for bs in (36, 45, 63):
        cases.append(run_case(ref, f"noise96x105_bs{bs}", noisy(128, 96, 105, 14), {"block_size": bs}))
    # difficult block 0 (Q4) at an even and an odd size
    for bs in (6, 9):
        cases.append(run_case(ref, f"q4_run_bs{bs}", {"kind": "q4_run", "shape": [36, 36], "bs": bs, "seed": 4},
                              {"block_size": bs, "fractal": False, "deflate": False}))
    # the 768^2 matrix with noise (SHA-1 only)
    for bs in (3, 12):
        cases.append(run_case(ref, f"noise768_bs{bs}", {"kind": "phantom_noise", "seed": 5, "n": 768, "amp": 90},
                              {"block_size": bs}, store=False))

    manifest = {"generator": "tools/gen_block_size_golden.py", "reference": "taaha-khan/2023-CompaCT-Image-Compression",
                "numpy": np.__version__, "cases": cases}
    with open(os.path.join(gi.GOLDEN, "block_sizes.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote", len(cases), "cases")


if __name__ == "__main__":
    main()
