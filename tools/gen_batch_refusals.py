#!/usr/bin/env python3
"""Write tests/golden/batch_refusals.json: what every case of tests/test_batch_args_host.py answers on this checkout (the
exception type and message, or the empty result, of each Python call; return code and cct_last_error() of each C call).
Run it on the commit whose behaviour is to be pinned, after the library is built; it needs no device.
    python tools/gen_batch_refusals.py [--check]      --check: compare with the file instead of writing it"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "2023-compact-image-compression_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_batch_args_host as t  # noqa: E402


def main(argv):
    text = json.dumps(t.record(), indent=1, sort_keys=True) + "\n"
    if "--check" in argv:
        with open(t.GOLDEN) as f:
            same = f.read() == text
        print("identical" if same else "DIFFERENT")
        return 0 if same else 1
    with open(t.GOLDEN, "w") as f:
        f.write(text)
    print(f"wrote {t.GOLDEN}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
