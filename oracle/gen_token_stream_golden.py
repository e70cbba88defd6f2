#!/usr/bin/env python3
"""Generate tests/golden/token_streams.json by running the REFERENCE decoder on hand-built and damaged token streams.

Run:  python3 -B oracle/gen_token_stream_golden.py
A sibling of gen_golden.py: the reference (/root/reference, read-only, Python) is imported as-is and only DATA is
written: the small input files (tests/golden/token_streams/*.cct, made by tests/token_streams.py, no encoder involved) and,
per file, the SHA-1 of the raster the reference's Decoder returns or the class of the exception it raises.
tests/test_token_streams_host.py holds the CPU oracle to these records.
"""
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_inputs as gi  # noqa: E402
import token_streams as ts  # noqa: E402

sys.path.insert(0, os.path.join(REF, "src"))
warnings.simplefilter("ignore")
from codec.core import Decoder  # noqa: E402  (the reference)

OUT = os.path.join(gi.GOLDEN, "token_streams")
SHAPES = [(32, 32, 16, "p50"), (64, 64, 16, "far"), (20, 20, 5, "rand"), (32, 32, 4, "p50")]


def reference_result(blob, bs):
    cfg = json.load(open(os.path.join(REF, "src", "config.json")))
    cfg["verbose"] = False
    cfg["block_size"] = bs
    try:
        return {"sha1": gi.sha1(Decoder(cfg, blob, None).decode())}
    except Exception as e:  # noqa: BLE001
        return {"raises": type(e).__name__}


def main():
    os.makedirs(OUT, exist_ok=True)
    records = []

    def add(name, blob, bs, N):
        fn = name + ".cct"
        with open(os.path.join(OUT, fn), "wb") as f:
            f.write(blob)
        payload = blob[13:]
        rec = {"file": fn, "block_size": bs, "len": len(blob), "judge": ts.classify(payload, N, bs) if not blob[12] else None}
        rec.update(reference_result(blob, bs))
        records.append(rec)
        print(f"{fn:44s} judge {str(rec['judge']):18s} reference {rec.get('raises') or 'raster ' + rec['sha1'][:10]}")

    for (W, H, bs, plan) in SHAPES:
        N = W * H
        rng = np.random.default_rng([W, H, bs, 2024])
        blob, img = ts.build(W, H, bs, True, plan, rng, full_p=0.3, bias=0.5 if plan == "far" else 0.0)
        tag = f"{W}x{H}_bs{bs}"
        add(f"{tag}_{plan}", blob, bs, N)
        assert records[-1].get("sha1") == gi.sha1(img.tobytes()), "the reference does not decode the writer's image"
        if bs == 16 and W == 32:
            add(f"{tag}_{plan}_deflate", ts.with_deflate(blob), bs, N)
        # one damaged file per (damage kind, judge's verdict), at most five per shape
        seen, kept = set(), 0
        items = ts.damage(blob, N, bs, rng, n_flips=40, n_bytes=3, n_cuts=1, n_jump_edits=2, n_append=1)
        for name, f in items:
            if name in ("cut_second_byte_of_last_pixel", "cut_one_pixel_short") and bs != 4:
                add(f"{tag}_{name}", f, bs, N)
        for name, f in items:
            key = ts.classify(f[13:], N, bs)
            if key in seen or (name == "flip" and key is None and ("flip", None) in seen):
                continue
            seen.add(key)
            add(f"{tag}_{name}_{kept}", f, bs, N)
            kept += 1
            if kept == 5:
                break
    # the 16-bit edge: the running value touches 65535 / 0 (decodes) and leaves the range by one (OverflowError)
    for target, kind, k in ((65535, ts.SHORT, 100), (65536, ts.SHORT, 100), (0, ts.FULL, 200), (-1, ts.FULL, 200), (-1, ts.SHORT, 0)):
        blob, img, _ = ts.edge_stream(32, 32, 16, True, "p50", np.random.default_rng(5), k, target, kind)
        add(f"32x32_bs16_edge_{target}_{'short' if kind == ts.SHORT else 'full'}_k{k}".replace("-", "m"), blob, 16, 1024)
        assert (records[-1].get("sha1") == gi.sha1(img.tobytes())) if img is not None else records[-1].get("raises") == "OverflowError"
    with open(os.path.join(gi.GOLDEN, "token_streams.json"), "w") as f:
        json.dump({"generator": "oracle/gen_token_stream_golden.py", "numpy": np.__version__, "records": records}, f, indent=1)
    print("wrote", len(records), "records")


if __name__ == "__main__":
    main()
