#!/usr/bin/env python3
"""Generate tests/golden/deflate_streams.json: what zlib does with every hand-built DEFLATE stream of tests/deflate_streams.py.

Run:  python3 -B oracle/gen_deflate_streams_golden.py
A sibling of gen_token_stream_golden.py.  Per case the record holds the name, the verdict (zlib.decompressobj with the
semantics of zlib.decompress: complete stream, nothing left over), the length of the stream, and the length and SHA-256 of the
output.  No stream bytes are stored: the tests rebuild the streams from the case list, and the recorded verdicts keep another
zlib build from moving the expectation.
"""
import hashlib
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_streams as ds  # noqa: E402


def record(name, group, stream):
    out = ds.oracle_verdict(stream)
    rec = {"name": name, "group": group, "stream_len": len(stream), "accept": out is not None}
    if out is not None:
        rec.update(out_len=len(out), sha256=hashlib.sha256(out).hexdigest())
    return rec


def main():
    records = [record(c.name, c.group, c.stream) for c in ds.cases()]
    records += [record(name, "cap", stream) for name, stream, _ in ds.cap_cases()]
    path = os.path.join(ROOT, "tests", "golden", "deflate_streams.json")
    with open(path, "w") as f:
        json.dump({"generator": "oracle/gen_deflate_streams_golden.py", "zlib": zlib.ZLIB_RUNTIME_VERSION, "records": records}, f, indent=1)
        f.write("\n")
    print("wrote", len(records), "records,", sum(r["accept"] for r in records), "accepted")


if __name__ == "__main__":
    main()
