#!/usr/bin/env python3
"""Generate tests/golden/value_edges.json by running the REFERENCE codec on the inputs of tests/value_edges.py.

Run:  python3 -B oracle/gen_value_edges_golden.py
A sibling of gen_golden.py: the reference (/root/reference, read-only, Python) is imported as-is and only DATA is written.
Per case: the resolved spec (what the seeded searches of tests/value_edges.py found: a position of the final order, or a seed
and a boundary block -- the tests never search), the builder's expectations, the SHA-1 of the input, and of what the reference's
Encoder returns with DEFLATE off: length, SHA-1, token counts, jump count and SHA-1 of the jump table; what its Decoder makes of
that file (SHA-1 of the raster and whether it is the input, or the name of the exception); for the end-to-end subset also
length and SHA-1 of the file with DEFLATE on.  No .cct file is stored.  The 1024x1024 case is left to the oracle alone.
tests/test_value_edges_host.py holds the CPU oracle to these records.
"""
import json
import multiprocessing
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_inputs as gi  # noqa: E402
import value_edges as ve  # noqa: E402

sys.path.insert(0, os.path.join(REF, "src"))
warnings.simplefilter("ignore")
from codec.core import Decoder, Encoder  # noqa: E402  (the reference)


def config(bs, deflate):
    cfg = json.load(open(os.path.join(REF, "src", "config.json")))
    cfg["verbose"] = False
    cfg["block_size"] = bs
    cfg["encoder"]["deflate_compression"] = deflate
    return cfg


def run_case(spec):
    t0 = time.time()
    spec = ve.resolve(spec)
    name, img, expect = ve.build(spec)
    bs = spec["bs"]
    rec = {"spec": spec, "expect": expect, "dtype": str(img.dtype), "input_sha1": gi.sha1(img.tobytes())}
    if spec.get("no_reference"):
        return rec
    cfg = config(bs, False)
    enc = Encoder(cfg, img, None)
    out = enc.encode()
    _, jumps = enc.partition.block_partition()   # deterministic: re-run for the jump table
    rec.update({"len": len(out), "sha1": gi.sha1(out),
                "tokens": {"short": int(enc.info["delta"]), "full": int(enc.info["full"]), "jump": len(jumps)},
                "jumps_sha1": gi.sha1(np.array(sorted(jumps.items()), dtype=np.int32).tobytes())})
    try:
        dec = Decoder(cfg, out, None).decode()
        rec["decode"] = {"sha1": gi.sha1(dec), "roundtrip": bool(dec == img.tobytes())}
    except Exception as e:  # noqa: BLE001
        rec["decode"] = {"raises": type(e).__name__}
    if spec.get("e2e"):
        z = Encoder(config(bs, True), img, None).encode()
        rec["deflate"] = {"len": len(z), "sha1": gi.sha1(z)}
    print(f"{name:48s} len {rec['len']:7d} {rec['tokens']} {rec['decode'].get('raises') or rec['decode']['roundtrip']} ({time.time() - t0:.1f}s)",
          flush=True)
    return rec


def main():
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        records = pool.map(run_case, ve.specs(), chunksize=1)
    with open(ve.GOLDEN_JSON, "w") as f:
        f.write('{"generator": "oracle/gen_value_edges_golden.py", "numpy": %s, "cases": [\n' % json.dumps(np.__version__))
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in records))
        f.write("\n]}\n")
    print("wrote", len(records), "cases,", os.path.getsize(ve.GOLDEN_JSON), "bytes")


if __name__ == "__main__":
    main()
