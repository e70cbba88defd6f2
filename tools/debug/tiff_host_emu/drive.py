"""Driver of emu.cpp (see its header): files / lzw / rows compare the emulated kernels with tests/tiff_model.py over the model's
clean, foreign and damaged strips.  `python drive.py` runs all three."""
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "..", "..", "tests")]
import numpy as np
import tiff_model as m

EMU = os.path.join(HERE, "emu")
D = tempfile.mkdtemp() + os.sep
FLAG_BIG, FLAG_PRED, FLAG_FROM_FILE = 1, 2, 4


def files(imgs, comp, pred, rps):
    n, rows, cols = imgs.shape
    imgs.tofile(D + "in.bin")
    subprocess.run([EMU, "f", str(imgs.dtype.itemsize), str(rows), str(cols), str(n), str(comp), str(pred), str(rps), D + "in.bin", D + "out.bin"],
                   check=True)
    b, out, p = open(D + "out.bin", "rb").read(), [], 0
    for _ in range(n):
        s = struct.unpack_from("<I", b, p)[0]
        out.append(b[p + 4:p + 4 + s])
        p += 4 + s
    return out


def strip_rec(src, dst, ln, want, file=0, row0=0, nrows=1, flags=0):
    return struct.pack("<QQIIIIII", src, dst, ln, want, file, row0, nrows, flags)


def lzw_decode(streams, wants):
    """[(status, bytes)] of the emulated decoder"""
    recs, blob, dst = b"", b"", 0
    for s, w in zip(streams, wants):
        recs += strip_rec(len(blob), dst, len(s), w)
        blob += s
        dst += (w + 3) & ~3
    open(D + "strips.bin", "wb").write(recs)
    open(D + "files.bin", "wb").write(blob or b"\0")
    subprocess.run([EMU, "d", str(len(streams)), D + "strips.bin", D + "files.bin", str(dst), D + "dec.bin"], check=True)
    b = open(D + "dec.bin", "rb").read()
    st = struct.unpack_from(f"<{len(streams)}I", b, 0)
    out, dst = [], 4 * len(streams)
    for k, w in enumerate(wants):
        out.append((st[k], b[dst:dst + w]))
        dst += (w + 3) & ~3
    return out


def run_files():
    for name, a, rpss in m.raster_cases():
        if a.size > 4096:
            continue  # a thread per lane: small strips here, the large ones on the device
        for comp in ("none", "lzw"):
            for pred in ((1,) if comp == "none" else (1, 2)):
                for rps in rpss:
                    r = m.rows_per_strip(a.shape[0], a.shape[1], a.dtype.itemsize, rps)
                    got = files(np.stack([a, a[::-1]]), m.COMPRESSION[comp], pred, r)
                    assert got[0] == m.write_file(a, comp, pred, rps), (name, comp, pred, rps)
                    assert got[1] == m.write_file(a[::-1], comp, pred, rps), (name, comp, pred, rps)
    for name, strip in m.edge_strips():                              # one row of bytes: EOI at each new width, behind a Clear
        a = np.frombuffer(strip, np.uint8).reshape(1, -1)
        assert files(a[None], 5, 1, 1)[0] == m.write_file(a, "lzw", 1, 1), name
    print("files ok")


def run_lzw():
    streams, wants, expect = [], [], []
    for name, s in m.edge_strips():                                   # clean, with table-full Clears
        streams.append(m.lzw_encode(s)); wants.append(len(s)); expect.append(("OK", s))
    for name, f, a in m.foreign_files() + m.damaged_files():         # every LZW strip of the foreign and damaged files
        d = m.parse(f)
        if d["compression"] != 5 or a.size > 4096:
            continue
        row_bytes = d["cols"] * d["bits"] // 8
        for k, (off, cnt) in enumerate(zip(d["offs"], d["counts"])):
            want = min(d["rps"], d["rows"] - k * d["rps"]) * row_bytes
            streams.append(f[off:off + cnt]); wants.append(want); expect.append(m.lzw_decode(f[off:off + cnt], want))
    noise = np.random.default_rng(5).integers(0, 256, 1500).astype(np.uint8).tobytes()
    for k in (1, 2, 5, 64, 65, 255, 300):
        streams.append(m.lzw_encode(noise, clear_every=k)); wants.append(len(noise)); expect.append(("OK", noise))
    streams += [b"", b"\x80", b"\x80\x00", m.lzw_encode(noise)]; wants += [5, 5, 5, len(noise) + 1]
    expect += [("CCT_E_STREAM", None)] * 4
    got = lzw_decode(streams, wants)
    for k, ((st, b), (verdict, x)) in enumerate(zip(got, expect)):
        assert (st == 0) == (verdict == "OK"), (k, st, verdict)
        assert verdict != "OK" or b == x, k
    print("lzw ok:", len(streams), "strips,", sum(v != "OK" for v, _ in expect), "damaged")


def run_rows():
    r = np.random.default_rng(3)
    for dt in (np.uint8, np.uint16):
        for rows, cols in ((1, 1), (2, 65), (3, 300), (5, 3)):
            a = r.integers(0, np.iinfo(dt).max + 1, (rows, cols)).astype(dt)
            a[0, : cols // 2] = np.iinfo(dt).max
            recs, dec, want = b"", b"", []
            variants = [(0, 1, "<"), (FLAG_PRED, 2, "<"), (FLAG_BIG | FLAG_PRED, 2, ">"), (FLAG_FROM_FILE | FLAG_BIG, 1, ">")]
            for i, (flags, pred, order) in enumerate(variants):
                for s, strip in enumerate(m.strips_of(a, pred, 2)[0]):
                    if order == ">" and dt == np.uint16:
                        strip = np.frombuffer(strip, "<u2").astype(">u2").tobytes()
                    nrows = len(strip) // (cols * a.dtype.itemsize)
                    recs += strip_rec(len(dec) + 1, len(dec) + 1, len(strip), len(strip), i, 2 * s, nrows, flags)
                    dec += b"\xAA" + strip            # odd offsets
                want.append(a)
            ns = len(recs) // 40
            open(D + "strips.bin", "wb").write(recs); open(D + "dec.bin", "wb").write(dec)
            subprocess.run([EMU, "u", str(a.dtype.itemsize), str(rows), str(cols), str(len(variants)), str(ns), D + "strips.bin", D + "dec.bin",
                            D + "dec.bin", D + "img.bin"], check=True)
            back = np.fromfile(D + "img.bin", dt).reshape(len(variants), rows, cols)
            assert np.array_equal(back, np.stack(want)), (dt, rows, cols)
    print("rows ok")


for what in sys.argv[1:] or ["files", "lzw", "rows"]:
    {"files": run_files, "lzw": run_lzw, "rows": run_rows}[what]()
