"""Feeds ./emu (see emu.cpp) the file sets of tests/jpeg2000_decode_model.py and compares statuses and rasters with the model:
the encoder model's files, OpenJPEG's own, the hand-built ones, the refused ones and every damaged file.  python drive.py [quick | damaged];
python drive.py edges [group] feeds it the model's files of the planted cases of tests/jpeg2000_edges.py, one call per shape."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "..", "tests"))
import jpeg2000_decode_model as d  # noqa: E402
import jpeg2000_model as m  # noqa: E402

EMU = os.path.join(HERE, "emu")
CODES = {0: "OK", 4: "CCT_E_STREAM", 10: "CCT_E_MIXED", 14: "CCT_E_J2K"}


def decode(files, rows, cols, bits, shift, tmp):
    """-> [status name or raster]"""
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    offs = np.zeros(len(files) + 1, np.uint64)
    np.cumsum([len(f) for f in files], out=offs[1:])
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(files)) + offs.tobytes() + b"".join(files))
    r = subprocess.run([EMU, *map(str, (rows, cols, bits, shift, src, dst))], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (rows, cols, bits, shift, r.stdout[-2000:], r.stderr[-6000:])
    out = open(dst, "rb").read()
    n = len(files)
    rc, status = struct.unpack_from("<i", out)[0], np.frombuffer(out, np.uint32, n, 4)
    imgs = np.frombuffer(out, np.uint8 if bits == 8 else np.uint16, n * rows * cols, 4 + 4 * n).reshape(n, rows, cols)
    assert rc == next((int(s) for s in status if s), 0), (rc, status)
    return [CODES[int(s)] if s else x for s, x in zip(status, imgs)]


def same(got, want):
    return got == want if isinstance(want, str) else not isinstance(got, str) and np.array_equal(got, want)


def edges(group):
    """The model's files of tests/jpeg2000_edges.py, mixed codings and precisions in one call per shape, forwards at 16 bits allocated and
    backwards; at 8 bits allocated what has at most 8 bits of precision (the others are CCT_E_MIXED); the shifted cases with their shift."""
    import jpeg2000_edges as e
    files, n = e.files(), 0
    with tempfile.TemporaryDirectory() as tmp:
        for rows, cols, cs in e.decode_batches():
            cs = [c for c in cs if group in (None, c.group)]
            if not cs:
                continue
            for order in (cs, cs[::-1]):
                for c, g in zip(order, decode([files[c.name] for c in order], rows, cols, 16, 0, tmp)):
                    assert same(g, c.raster.astype(np.uint16) << c.kw.get("shift", 0)), (c.name, g if isinstance(g, str) else "a raster")
            if any(c.kw["precision"] <= 8 for c in cs):
                for c, g in zip(cs, decode([files[c.name] for c in cs], rows, cols, 8, 0, tmp)):
                    want = "CCT_E_MIXED" if c.kw["precision"] > 8 else c.raster << c.kw.get("shift", 0)
                    assert same(g, want), (c.name, g if isinstance(g, str) else "a raster")
            for shift in sorted({c.kw["shift"] for c in cs if c.kw.get("shift")}):
                sel = [c for c in cs if c.kw.get("shift") == shift]
                for c, g in zip(sel, decode([files[c.name] for c in sel], rows, cols, 16, shift, tmp)):
                    assert same(g, c.raster), (c.name, shift)
            n += len(cs)
            print("ok", rows, cols, len(cs), "files", flush=True)
    print("edges ok:", n, "cases")


def main(quick):
    with tempfile.TemporaryDirectory() as tmp:
        for precision in () if quick == "damaged" else sorted(m.PRECISIONS):
            bits = 8 if precision == 8 else 16
            for rows, cols, cb, levels, names, imgs, files in m.matrix(precision):
                if quick and (levels == 1 or precision == 12 or rows * cols > 5000):
                    continue
                for name, g, x in zip(names, decode(files, rows, cols, bits, 0, tmp), imgs):
                    assert same(g, x), (rows, cols, cb, levels, precision, name)
            print("ok encoder model's files at precision", precision, flush=True)
        if quick != "damaged":
            img, kw, f = m.phantoms()[3]  # shift 4, JP2
            assert same(decode([f], 128, 128, 16, 4, tmp)[0], img)
        hand = d.handbuilt_set()
        for (name, f, x), g in zip(hand[:5], decode([f for _, f, _ in hand[:5]], 33, 65, 16, 0, tmp)):  # code-blocks of two sizes in one batch
            assert same(g, x), name
        assert same(decode([hand[5][1]], 33, 65, 16, 0, tmp)[0], hand[5][2])
        print("ok phantom with shift 4 and JP2, hand-built files", flush=True)
        if d.pillow_has_jpeg2000() and quick != "damaged":
            fs = d.foreign_set()
            refused = d.refused_set()
            batch = [f for _, f, _ in fs[:-1]] + [f for _, f in refused]  # one mixed batch: five codings, refused neighbours
            got = decode(batch, 70, 130, 16, 0, tmp)
            for (name, f, x), g in zip(fs[:-1], got):
                assert same(g, x) and same(d.decode(f, 70, 130), x), name
            assert got[len(fs) - 1:] == ["CCT_E_J2K"] * len(refused), got[len(fs) - 1:]
            assert same(decode([fs[-1][1], fs[0][1]], 70, 130, 8, 0, tmp)[0], fs[-1][2])  # 8 bits; the 16-bit neighbour is CCT_E_MIXED
            assert decode([fs[-1][1], fs[0][1]], 70, 130, 8, 0, tmp)[1] == "CCT_E_MIXED"
            print("ok OpenJPEG's files and the refused ones", flush=True)
        img, cases = d.marker_cases()
        for (name, _, want), g in zip(cases, decode([f for _, f, _ in cases], 9, 11, 16, 0, tmp)):
            assert same(g, img if want == "OK" else want), name
        print("ok", len(cases), "files with one marker segment changed", flush=True)
        dm = d.damaged_set()
        for base in sorted({b for b, *_ in dm}):
            sel = [e for e in dm if e[0] == base]
            rows, cols = sel[0][3:]
            got = decode([g for _, _, g, _, _ in sel], rows, cols, 16, 0, tmp)
            for (_, dmg, g, _, _), r in zip(sel, got):
                assert same(r, d.decode(g, rows, cols)), (base, dmg, r if isinstance(r, str) else "a raster")
            print("ok", len(sel), "damaged files of", base, flush=True)
        print("decode ok")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "edges":
        edges(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else "")
