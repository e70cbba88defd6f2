"""Feeds ./emu (see emu.cpp) rasters and files of tests/jpeg_ls_model.py and compares: python drive.py [enc|dec], or
python drive.py streams [part of a name ...] for the placed and damaged files of tests/jpeg_ls_streams.py"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "..", "tests"))
import jpeg_ls_model as m  # noqa: E402

EMU = os.path.join(HERE, "emu")


def run(*args):
    r = subprocess.run([EMU, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])


def params_words(p):
    return struct.pack("<9I", p.maxval, p.range, p.qbpp, p.limit, p.a0, p.reset, p.t1, p.t2, p.t3)


def encode(imgs, precision, restart_rows, tmp):
    n, rows, cols = imgs.shape
    imgs.tofile(os.path.join(tmp, "in.bin"))
    open(os.path.join(tmp, "par.bin"), "wb").write(params_words(m.Params(precision)))
    run("e", 8 * imgs.dtype.itemsize, precision, rows, cols, n, restart_rows, os.path.join(tmp, "par.bin"), os.path.join(tmp, "in.bin"),
        os.path.join(tmp, "out.bin"))
    d, out, pos = open(os.path.join(tmp, "out.bin"), "rb").read(), [], 0
    for _ in range(n):
        size, status = struct.unpack_from("<II", d, pos)
        out.append((status, d[pos + 8:pos + 8 + size]))
        pos += 8 + size
    return out


def decode(files, rows, cols, bits, tmp):
    """-> (status per file: 0, 'JPEGLS', 'MIXED' or 'STREAM'; rasters), the host's part done as api_jpeg_ls.cpp does it"""
    frames, ints, blob, status, sent = b"", b"", b"", [0] * len(files), []
    for i, f in enumerate(files):
        try:
            h = m.parse(f)
            if (h["Y"], h["X"]) != (rows, cols) or h["P"] > bits:
                raise m.JlsError("MIXED", "")
            rpi = h["ri"] if 0 < h["ri"] < rows else rows
            n_int = -(-rows // rpi)
            if len(h["intervals"]) != n_int or h["rst"] != [k % 8 for k in range(n_int - 1)]:
                raise m.JlsError("STREAM", "")
        except m.JlsError as e:
            status[i] = e.kind
        else:
            for k, (a, b) in enumerate(h["intervals"]):
                ints += struct.pack("<5I", len(blob) + a, b - a, len(sent), k * rpi, min(rpi, rows - k * rpi))
            frames += struct.pack("<I", i) + params_words(h["params"])
            sent.append(i)
        blob += f
    dt = np.uint8 if bits == 8 else np.uint16
    if not sent:
        return status, np.zeros((len(files), rows, cols), dt)
    open(os.path.join(tmp, "job.bin"), "wb").write(struct.pack("<I", len(sent)) + frames + ints)
    open(os.path.join(tmp, "files.bin"), "wb").write(blob)
    run("d", rows, cols, bits, len(files), os.path.join(tmp, "job.bin"), os.path.join(tmp, "files.bin"), os.path.join(tmp, "out.bin"))
    d = open(os.path.join(tmp, "out.bin"), "rb").read()
    st = struct.unpack_from(f"<{len(sent)}I", d, 0)
    for i, s in zip(sent, st):
        if s:
            status[i] = "STREAM"
    return status, np.frombuffer(d, dt, offset=4 * len(sent)).reshape(len(files), rows, cols)


def main(which):
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as tmp:
        if which in ("enc", "all"):
            assert encode(m.H3_RASTER[None], 8, 0, tmp)[0][1] == m.H3_FILE
            for rows, cols in ((1, 1), (2, 2), (5, 63), (2, 64), (5, 65), (17, 130)):
                for p in m.PRECISIONS:
                    c = m.raster_cases(rows, cols, p)
                    imgs = np.stack(list(c.values()))
                    for rr in m.RESTARTS:
                        got = encode(imgs, p, rr, tmp)
                        for name, (st, g), x in zip(c, got, imgs):
                            assert st == 0 and g == m.encode_frame(x, p, rr), (rows, cols, p, rr, name)
            for name, (x, p) in m.census_cases().items():
                for rr in (0, 3):
                    assert encode(x[None], p, rr, tmp)[0] == (0, m.encode_frame(x, p, rr)), (name, rr)
            ones = np.full((3, 200), 65535, np.uint16)  # one escape code far from the initial state, then runs of growing RUNindex
            assert encode(ones[None], 16, 0, tmp)[0] == (0, m.encode_frame(ones, 16))
            over = rng.integers(0, 4096, (3, 4, 9)).astype(np.uint16)
            over[1, 2, 3] = 4096
            got = encode(over, 12, 0, tmp)
            assert [s for s, _ in got] == [0, 1, 0] and got[1][1] == b"" and got[2][1] == m.encode_frame(over[2], 12)
            print("encode ok")
        if which in ("dec", "all"):
            for rows, cols, p in ((1, 1, 8), (5, 7, 8), (5, 65, 12), (3, 130, 16), (2, 64, 2)):
                bits = 8 if p <= 8 else 16
                c = m.raster_cases(rows, cols, p)
                files, want = [], []
                for x in c.values():
                    for rr in m.RESTARTS:
                        files.append(m.encode_frame(x, p, rr))
                        want.append(x)
                files.append(files[6][:-9] + b"\xff\xd9")  # ends early, or the cut leaves a marker behind
                files.append(b"junk")
                st, got = decode(files, rows, cols, bits, tmp)
                for i, w in enumerate(want):
                    assert st[i] == 0 and np.array_equal(got[i], w), (rows, cols, i, st[i])
                try:
                    m.decode_frame(files[-2], rows, cols, bits)
                    cut = 0
                except m.JlsError as e:
                    cut = e.kind
                assert st[-1] == "JPEGLS" and st[-2] == cut and cut != 0, (st[-2:], cut)
            for name, (x, p) in m.census_cases().items():
                bits = 8 if p <= 8 else 16
                st, got = decode([m.encode_frame(x, p, rr) for rr in (0, 3)], *x.shape, bits, tmp)
                assert st == [0, 0] and np.array_equal(got[0], x) and np.array_equal(got[1], x), name
            print("decode ok")
        if which == "streams":
            streams(tmp, sys.argv[2:])


def streams(tmp, only):
    """the set of tests/jpeg_ls_streams.py, a shape a batch, as tests/test_gpu_jpeg_ls_streams.py compares it; further
    arguments are substrings of the names to run"""
    import jpeg_ls_streams as s
    want = s.verdicts()
    ran = 0
    for (rows, cols, bits), entries in s.shapes().items():
        keep = [e for e in entries if not only or any(o in e[0] for o in only)]
        for at in range(0, len(keep), 16):
            part = keep[at:at + 16]
            st, got = decode([e[1] for e in part], rows, cols, bits, tmp)
            for i, e in enumerate(part):
                kind, raster = want[e[0]]
                assert st[i] == kind, (e[0], st[i], kind)
                if kind == 0:
                    assert np.array_equal(got[i], raster), e[0]
            ran += len(part)
            print(f"{rows} x {cols} x {bits}: {ran} files", flush=True)
    print(f"streams ok: {ran} files")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "all")
