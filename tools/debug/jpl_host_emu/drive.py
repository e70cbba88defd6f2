"""Feeds ./emu (see emu.cpp) rasters and files of tests/jpeg_lossless_model.py and compares: python drive.py [enc|dec], or
python drive.py streams [part of a name ...] for the placed and damaged files of tests/jpeg_lossless_streams.py"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "..", "tests"))
import jpeg_lossless_model as m  # noqa: E402
import jpeg_lossless_predictors as jp  # noqa: E402

EMU = os.path.join(HERE, "emu")


def run(*args):
    r = subprocess.run([EMU, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])


def encode(imgs, precision, restart_rows, tmp, predictor=1, with_ss=False):
    """-> (status, file) per frame, with with_ss (status, file, Ss); predictor 1 .. 7, or 0 for the frame's best"""
    n, rows, cols = imgs.shape
    imgs.tofile(os.path.join(tmp, "in.bin"))
    run("e", 8 * imgs.dtype.itemsize, precision, rows, cols, n, restart_rows, predictor, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"))
    d, out, pos = open(os.path.join(tmp, "out.bin"), "rb").read(), [], 0
    for _ in range(n):
        size, status, ss = struct.unpack_from("<III", d, pos)
        out.append((status, d[pos + 12:pos + 12 + size], ss) if with_ss else (status, d[pos + 12:pos + 12 + size]))
        pos += 12 + size
    return out


def encode_predictors(tmp, rng):
    """selection values 2 .. 7 and the frame's best against the model: files, the Ss reported, differences that leave 16 bits,
    frames of one batch that choose differently, and an overflowing frame among good ones"""
    for rows, cols in ((1, 1), (1, 65), (3, 1), (2, 3), (17, 63), (5, 257)):
        for dt, p in ((np.uint8, 8), (np.uint16, 12), (np.uint16, 16)):
            c = m.raster_cases(rows, cols, p, dt)
            imgs = np.stack(list(c.values()))
            for ss in jp.PREDICTORS[1:]:
                rr = (0, 1, 2, 5)[(ss + rows + p) % 4]
                for name, (st, g, s), x in zip(c, encode(imgs, p, rr, tmp, ss, True), imgs):
                    assert st == 0 and s == ss and g == m.encode_frame(x, p, ss, 0, rr), (rows, cols, p, rr, ss, name)
            for rr in (0, 2):
                for name, (st, g, s), x in zip(c, encode(imgs, p, rr, tmp, 0, True), imgs):
                    pick = jp.auto_pick(x, p, rr)
                    assert st == 0 and s == pick and g == m.encode_frame(x, p, pick, 0, rr), (rows, cols, p, rr, name, s, pick)
    wrap = jp.wrap_rasters()
    imgs = np.stack(list(wrap.values()))
    for ss in jp.PREDICTORS:
        for name, (st, g), x in zip(wrap, encode(imgs, 16, 0, tmp, ss), imgs):
            assert st == 0 and g == m.encode_frame(x, 16, ss), (name, ss)
    planted = jp.planted()
    imgs = np.stack([x for x, _, _ in planted.values()] + [rng.integers(0, 256, (16, 24)).astype(np.uint8)])
    got = encode(imgs, 8, 0, tmp, 0, True)
    assert [s for _, _, s in got[:3]] == [want for _, _, want in planted.values()] == [1, 2, 3]
    for (st, g, s), x in zip(got, imgs):
        assert st == 0 and s == jp.auto_pick(x, 8) and g == m.encode_frame(x, 8, s), s
    over = rng.integers(0, 4096, (3, 4, 9)).astype(np.uint16)
    over[1, 2, 3] = 4096
    for pred in (4, 0):
        got = encode(over, 12, 0, tmp, pred, True)
        assert [st for st, _, _ in got] == [0, 1, 0] and got[1][1] == b"" and all(1 <= s <= 7 for _, _, s in got)
        for i in (0, 2):
            ss = pred or jp.auto_pick(over[i], 12)
            assert got[i][2] == ss and got[i][1] == m.encode_frame(over[i], 12, ss), (pred, i)


def decode(files, rows, cols, bits, tmp):
    """-> (status per file: 0, 'JPEG', 'MIXED' or 'STREAM'; rasters)"""
    job, blob, status, sent = b"", b"", [0] * len(files), []
    for i, f in enumerate(files):
        try:
            h = m.parse(f)
            if (h["Y"], h["X"]) != (rows, cols) or h["P"] > bits:
                raise m.JpegError("MIXED", "")
        except m.JpegError as e:
            status[i] = e.kind
        else:
            b, v = h["table"]
            job += struct.pack("<8I", len(blob) + h["s0"], h["s1"] - h["s0"], i, h["ss"], h["pt"], h["P"], h["ri"], len(v))
            job += bytes(b) + bytes(v).ljust(20, b"\0")
            sent.append(i)
        blob += f
    dt = np.uint8 if bits == 8 else np.uint16
    if not sent:
        return status, np.zeros((len(files), rows, cols), dt)
    open(os.path.join(tmp, "job.bin"), "wb").write(job)
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
            for rows, cols in ((1, 1), (2, 3), (3, 65), (17, 63), (5, 257)):
                for dt, p in ((np.uint8, 8), (np.uint16, 12), (np.uint16, 16)):
                    c = m.raster_cases(rows, cols, p, dt)
                    imgs = np.stack(list(c.values()))
                    for rr in (0, 1, 2):
                        got = encode(imgs, p, rr, tmp)
                        for name, (st, g), x in zip(c, got, imgs):
                            assert st == 0 and g == m.encode_frame(x, p, restart_rows=rr), (rows, cols, p, rr, name)
            fib = m.fibonacci_raster()
            assert encode(fib[None], 16, 0, tmp)[0][1] == m.encode_frame(fib, 16)
            over = rng.integers(0, 4096, (3, 4, 9)).astype(np.uint16)
            over[1, 2, 3] = 4096
            got = encode(over, 12, 0, tmp)
            assert [s for s, _ in got] == [0, 1, 0] and got[1][1] == b"" and got[2][1] == m.encode_frame(over[2], 12)
            encode_predictors(tmp, rng)
            print("encode ok")
        if which in ("dec", "all"):
            for rows, cols, bits, p in ((1, 1, 8, 8), (5, 7, 8, 8), (5, 65, 16, 12), (3, 257, 16, 16)):
                img = rng.integers(0, 1 << p, (rows, cols)).astype(np.uint8 if bits == 8 else np.uint16)
                files, want = [], []
                for ss in range(1, 8):
                    for pt in (0, 2):
                        for rr in (0, 1, 2):
                            files.append(m.encode_frame(img, p, ss, pt, rr))
                            want.append((img >> pt) << pt)
                files.append(m.encode_frame(img, p)[:-9] + b"\xff\xd9")  # ends early
                files.append(b"junk")
                st, got = decode(files, rows, cols, bits, tmp)
                for i, w in enumerate(want):
                    assert st[i] == 0 and np.array_equal(got[i], w), (rows, cols, i, st[i])
                assert st[-1] == "JPEG" and (st[-2] == "STREAM" or rows * cols == 1), st[-2:]
            # long intervals: several subsequences, codes across their borders; a one-bit code
            img = rng.integers(0, 65536, (4, 520)).astype(np.uint16)
            zero = np.full((4, 520), 128, np.uint8)
            st, got = decode([m.encode_frame(img, 16), m.encode_frame(img, 16, 7, 0, 4)], 4, 520, 16, tmp)
            assert st == [0, 0] and np.array_equal(got[0], img) and np.array_equal(got[1], img)
            one = ([1] + [0] * 15, [0])
            f = m.encode_frame(zero, 8, table=one)
            assert len(f) < 600
            st, got = decode([f], 4, 520, 8, tmp)
            assert st == [0] and np.array_equal(got[0], zero)
            # words of one length and no extra bits: a wrong entry never resynchronises, corrections move on one subsequence a round
            f = m.encode_frame(zero, 8, table=m.FLAT5)
            assert 8 * len(f) > 10 * 1024
            st, got = decode([f], 4, 520, 8, tmp)
            assert st == [0] and np.array_equal(got[0], zero)
            print("decode ok")
        if which == "streams":
            streams(tmp, sys.argv[2:])


# The emulation runs a thread per lane: a 64 x 1000 file under the flat 5-bit table (312 subsequences that never resynchronise)
# takes minutes under the sanitizers.  Of the two const_flat5 bases these damages run, the others are dropped.
KEPT_TWO_WINDOW = ("undamaged", "word_10001_window2", "flip_code_low_bit_window1_last_sub", "flip_code_top_bit_window2", "cut_130_bytes_of_last_interval",
                   "cut_1000_bytes_of_middle_interval", "1_zero_bytes_behind_last_interval", "1_zero_bytes_behind_middle_interval",
                   "intervals_swapped", "rst_renumbered")


def streams(tmp, only):
    """the set of tests/jpeg_lossless_streams.py, a shape a batch, as tests/test_gpu_jpeg_lossless_streams.py compares it;
    further arguments are substrings of the names to run"""
    import jpeg_lossless_streams as s
    want = s.verdicts()
    ran = dropped = 0
    for (rows, cols, bits), entries in s.shapes().items():
        keep = [e for e in entries if not s.base_of(e[0]).startswith("const_flat5") or e[0].split("/")[1] in KEPT_TWO_WINDOW]
        dropped += len(entries) - len(keep)
        if only:
            keep = [e for e in keep if any(o in e[0] for o in only)]
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
    print(f"streams ok: {ran} files, {dropped} left out")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "all")
