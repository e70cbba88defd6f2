"""Driver of emu.cpp (see its header).  CPython's zlib is the judge of every verdict and byte of the INFLATE kernel; the
hand-built streams are held to tests/golden/deflate_streams.json as well, the PNG files to the expectations of tests/png_files.py.
    hand    every case of deflate_streams.cases() and cap_cases(): each alone, and all in one batch in both orders
    walk    every case of inflate_walk_inputs.py, preconditions asserted, in the batches of tests/test_gpu_inflate_walk_edges.py
    damage  seeded zlib streams of four payload kinds, left alone or damaged in one of four ways, packed back to back
    skip    the .cct entrance (skip = 13) with a stream starting at every offset modulo 16
            (a stream is a launch of its own with a slot of its own; skip and the head of damage run as one grid as well)
    png     png_unpack_kernel -> inflate_kernel -> png_unfilter_kernel on chunk_cases, damaged_cases, the small edge batches,
            IDAT cuts at every source and destination alignment, the unfilter kernel at 1, 2, 4 and 8 waves
`python drive.py` runs all of them at 256 and 512 lanes; `python drive.py hand walk --lanes 256` some of them.  emu exits
non-zero on a sanitizer report or a damaged LDS gap, which ends the run (check=True)."""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.join(HERE, "..", "..", "..", "tests")
sys.path[:0] = [TESTS]
import numpy as np
import deflate_streams as ds
import inflate_walk_inputs as wi
import png_files as pf

EMU = os.path.join(HERE, "emu")
ST_STREAM, ST_ZLIB = 8, 16                       # CCT_ST_* (include/compact_hip.h)
PNG_ST_CRC, PNG_ST_FILTER, PNG_ST_SKIP = 1, 2, 4  # cct_internal.h
PNG_CHUNK_IDAT = 1 << 31
LANES = (256, 512)
DAMAGE_SEEDS = {256: 1, 512: 2}
DAMAGE_N = 400
GRID_N = 50  # streams of the damage family that also run as one grid


SANITIZE = ["-fsanitize=address,undefined,bounds", "-fno-sanitize-recover=undefined"]


def build(exe=None, cxx="g++", extra=()):
    """the command of emu.cpp's header"""
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", *SANITIZE, *extra, "-I" + os.path.join(HERE, "..", "rle_host_emu"), "-w",
                           "-x", "c++", os.path.join(HERE, "emu.cpp"), "-o", exe or EMU, "-lpthread"])


def inflate(streams, lanes, out_stride, skip=0, one_launch=False):
    """[(status bits, size, bytes or None)] of one emulated batch; stream i is streams[i][skip:].  one_launch: the batch as one
    grid of len(streams) workgroups with the slots in one allocation (emu.cpp), instead of a launch and a slot per stream"""
    offs = [0]
    for s in streams:
        offs.append(offs[-1] + len(s))
    with tempfile.TemporaryDirectory() as d:
        d += os.sep
        with open(d + "in.bin", "wb") as f:
            f.write(struct.pack("<I", len(streams)) + struct.pack(f"<{len(offs)}Q", *offs) + b"".join(streams))
        subprocess.run([EMU, str(lanes), d + "in.bin", str(out_stride), d + "out.bin", str(skip), "grid" if one_launch else "each"], check=True)
        with open(d + "out.bin", "rb") as f:
            b = f.read()
    out, p = [], 0
    for _ in streams:
        st, size = struct.unpack_from("<II", b, p)
        p += 8
        data = None
        if st == 0:
            data = b[p:p + size]
            p += size
        out.append((st, size, data))
    assert p == len(b)
    return out


def judge(items, lanes, out_stride, skip=0, one_launch=False):
    """items: [(name, stream)].  zlib refuses -> the ZLIB bit; zlib's output longer than the slot -> the STREAM bit without the
    ZLIB bit (CCT_E_CAP); else status 0 and zlib's bytes.  -> the number of streams zlib accepts"""
    try:
        got = inflate([s for _, s in items], lanes, out_stride, skip, one_launch)
    except subprocess.CalledProcessError as e:
        raise AssertionError(f"lanes {lanes}: emu exit status {e.returncode} (its report is above) on the batch {[n for n, _ in items][:4]} ...") from None
    wrong, accepted = [], 0
    for (name, s), (st, size, data) in zip(items, got):
        want = ds.oracle_verdict(s[skip:])
        if want is None:
            ok = bool(st & ST_ZLIB)
        elif len(want) > out_stride:
            ok = bool(st & ST_STREAM) and not st & ST_ZLIB
        else:
            ok = st == 0 and data == want
            accepted += 1
        if not ok:
            wrong.append((name, st, size, None if want is None else len(want)))
    assert not wrong, f"lanes {lanes}: {len(wrong)} of {len(items)} differ from zlib: (name, status, size, zlib's size) {wrong[:8]}"
    return accepted


# ---- hand ----------------------------------------------------------------------------------------------------------------------
def hand_items():
    with open(os.path.join(TESTS, "golden", "deflate_streams.json")) as f:
        records = {r["name"]: r for r in json.load(f)["records"]}
    items = [(c.name, c.stream) for c in ds.cases()] + [(name, s) for name, s, _ in ds.cap_cases()]
    m = ds.max_out()
    for name, s in items:  # the fixture agrees with zlib here, so judge() against zlib is a check against the fixture
        rec, want = records[name], ds.oracle_verdict(s)
        assert rec["accept"] == (want is not None), name
        if want is not None:
            assert rec["out_len"] == len(want) and rec["sha256"] == hashlib.sha256(want).hexdigest(), name
    caps = {name: st for name, _, st in ds.cap_cases()}
    assert all((len(ds.oracle_verdict(s)) > ds.out_stride(m)) == (caps[name] == ds.E_CAP) for name, s in items if name in caps)
    return items


def run_hand(lanes, alone=True):
    items, stride = hand_items(), ds.out_stride(ds.max_out())
    if alone:
        for it in items:
            judge([it], lanes, stride)
    n = judge(items, lanes, stride)
    judge(items[::-1], lanes, stride)  # other neighbours, other byte alignments
    print(f"hand ok at {lanes} lanes: {len(items)} streams ({n} accepted){', each alone' if alone else ''} and in one batch in both orders")


# ---- walk ----------------------------------------------------------------------------------------------------------------------
def walk_batches():
    """the batches of tests/test_gpu_inflate_walk_edges.py, after the assertions of tests/test_inflate_walk_inputs_host.py"""
    cases = wi.cases()
    for c in cases:
        out = ds.oracle_verdict(c.stream)
        assert (out is not None) == c.accept, c.name
        w = wi.host_walk(c.stream)
        assert (w["error"] is None) == c.accept and (not c.accept or w["out"] == out), c.name
        c.pre(c.stream)
    group = lambda gs: [(c.name, c.stream) for c in cases if c.group in gs]
    items, good = group((1, 2, 3, 4, 5)), group((4,))
    for k, bad in enumerate(group((6,))):  # every refusal between accepted neighbours
        items += [bad, good[k % len(good)]]
    batches = [group((1, 2, 3, 4, 5, 6)), items, items[::-1]]  # every case once; then as the device test packs them
    for tail in (b"", b"\0", b"\0\0\0\0"):  # group 4 as the last stream of the input, and one byte and one dword before its end
        for item in group((4,)):
            batches.append(group((2,)) + [item] + ([("tail", tail)] if tail else []))
    stride = ds.out_stride(max(len(ds.oracle_verdict(c.stream)) for c in cases if c.accept))
    return batches, stride


def run_walk(lanes, every_batch=True):
    """every_batch=False: every case once, in one batch (a stream is a launch of its own here, so what the other batches add is
    other byte alignments)"""
    batches, stride = walk_batches()
    batches = batches if every_batch else batches[:1]
    for b in batches:
        judge(b, lanes, stride)
    print(f"walk ok at {lanes} lanes: {len(batches)} batches, {sum(len(b) for b in batches)} streams")


# ---- damage --------------------------------------------------------------------------------------------------------------------
IN_BLOCK = ("literal/length code", "distance code", "distance too far back")  # refusals of deflate_streams.walk inside a Huffman block


def damage_family(seed, n):
    """[(name, stream)]: payloads of 1 .. 6000 bytes (noise, 2-bit noise, a random walk, a period-7 pattern), levels 1 .. 9, left
    alone (one in four) or damaged: bit flips, a cut, a byte overwritten, 1 .. 8 bytes inserted"""
    rng = np.random.default_rng(seed)
    items = []
    for k in range(n):
        size, kind = int(rng.integers(1, 6001)), int(rng.integers(0, 4))
        if kind == 0:
            pay = rng.integers(0, 256, size, dtype=np.uint8)
        elif kind == 1:
            pay = rng.integers(0, 4, size, dtype=np.uint8)
        elif kind == 2:
            pay = (np.cumsum(rng.integers(-2, 3, size)) & 255).astype(np.uint8)
        else:
            pay = np.resize(rng.integers(0, 256, 7, dtype=np.uint8), size)
            pay[rng.integers(0, size, size // 50)] ^= 1
        z = bytearray(zlib.compress(pay.tobytes(), int(rng.integers(1, 10))))
        how = int(rng.integers(0, 16))
        if how >= 12:
            how = "intact"
        elif how % 4 == 0:
            for _ in range(int(rng.integers(1, 4))):
                z[int(rng.integers(0, len(z)))] ^= 1 << int(rng.integers(0, 8))
            how = "flips"
        elif how % 4 == 1:
            del z[int(rng.integers(0, len(z))):]
            how = "cut"
        elif how % 4 == 2:
            z[int(rng.integers(0, len(z)))] = int(rng.integers(0, 256))
            how = "byte"
        else:
            at = int(rng.integers(0, len(z) + 1))
            z[at:at] = rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tobytes()
            how = "insert"
        items.append((f"damage-{seed}-{k}-{'nqwp'[kind]}{size}-{how}", bytes(z)))
    return items


def damage_census(items):
    """(accepted by zlib, refused inside a Huffman block) -- the reference alone says what the family reaches"""
    accepted = sum(ds.oracle_verdict(s) is not None for _, s in items)
    in_block = sum(ds.oracle_verdict(s) is None and ds.walk(s)["error"] in IN_BLOCK for _, s in items)
    return accepted, in_block


def run_damage(lanes, n=DAMAGE_N, min_in_block=30, grid_n=GRID_N):
    items = damage_family(DAMAGE_SEEDS[lanes], n)
    accepted, in_block = damage_census(items)
    assert in_block >= min_in_block and accepted >= 0.15 * n, (accepted, in_block)
    assert {len(b"".join(s for _, s in items[:k])) % 16 for k in range(len(items))} == set(range(16))  # every byte alignment
    assert judge(items, lanes, ds.out_stride(6000)) == accepted
    grid = items[:grid_n]  # the same streams as the workgroups of one launch: blockIdx.x > 0, offsets[s], s * out_stride
    assert judge(grid, lanes, ds.out_stride(6000), one_launch=True) == sum(ds.oracle_verdict(s) is not None for _, s in grid)
    print(f"damage ok at {lanes} lanes: seed {DAMAGE_SEEDS[lanes]}, {n} streams, {accepted} accepted by zlib, {in_block} refused inside a Huffman block")


# ---- skip ----------------------------------------------------------------------------------------------------------------------
def skip_items():
    """16 .cct-like files (13 bytes of header, then a zlib stream) of 1 modulo 16 bytes: the streams start at every offset modulo
    16; then the same with every other stream cut by 16 bytes"""
    rng = np.random.default_rng(77)
    files = []
    while len(files) < 16:
        pay = (np.cumsum(rng.integers(-1, 2, int(rng.integers(200, 3000)))) & 255).astype(np.uint8).tobytes()
        f = bytes(rng.integers(0, 256, 13, dtype=np.uint8)) + zlib.compress(pay, int(rng.integers(1, 10)))
        if len(f) % 16 == 1:
            files.append(f)
    items = [(f"skip-{k}", f) for k, f in enumerate(files)]
    cut = [(f"skip-cut-{k}", f[:-16] if k % 2 else f) for k, f in enumerate(files)]
    for batch in (items, cut):
        starts, p = set(), 0
        for _, f in batch:
            starts.add((p + 13) % 16)
            p += len(f)
        assert starts == set(range(16))
    return [items, cut]


def run_skip(lanes):
    for batch in skip_items():
        n = judge(batch, lanes, ds.out_stride(3000), skip=13)
        assert judge(batch, lanes, ds.out_stride(3000), skip=13, one_launch=True) == n  # blockIdx.x > 0: offsets[s], s * out_stride
    assert n == 8
    print(f"skip ok at {lanes} lanes: streams at every offset modulo 16 behind 13 bytes, whole and cut, a launch each and as one grid")


# ---- png -----------------------------------------------------------------------------------------------------------------------
def png_walk(f, base, index, rows, cols, tab, zoff):
    """api.cpp png_walk_file: the chunk heads of one file -> PngChunk records (src, dst, len, file); -> (status, depth, zoff)"""
    head = pf.SIGNATURE + b"\0\0\0\x0dIHDR"
    if len(f) < 33 or f[:16] != head:
        return pf.E_PNG, 0, zoff
    w, h, depth = struct.unpack_from(">IIB", f, 16)
    if w == 0 or h == 0 or w > 0x7FFFFFFF or h > 0x7FFFFFFF or depth not in (8, 16) or f[25:29] != b"\0\0\0\0":
        return pf.E_PNG, 0, zoff
    mine, z, p = [(base + 12, 0, 13, index)], zoff, 33
    idat = idat_over = iend = False
    while p < len(f) and not iend:
        if len(f) - p < 12:
            return pf.E_PNG, 0, zoff
        L = struct.unpack_from(">I", f, p)[0]
        t = f[p + 4:p + 8]
        if L > 0x7FFFFFFF or L > len(f) - p - 12 or not t.isalpha() or not t.isascii():
            return pf.E_PNG, 0, zoff
        if t == b"IDAT":
            if idat_over:
                return pf.E_PNG, 0, zoff
            idat = True
            mine.append((base + p + 4, z, L, index | PNG_CHUNK_IDAT))
            z += L
        else:
            idat_over = idat_over or idat
            if t == b"IEND":
                if L:
                    return pf.E_PNG, 0, zoff
                iend = True
            elif not t[0] & 0x20:
                return pf.E_PNG, 0, zoff
            mine.append((base + p + 4, 0, L, index))
        p += 12 + L
    if not iend or p != len(f) or not idat:
        return pf.E_PNG, 0, zoff
    if (h, w) != (rows, cols):
        return pf.E_MIXED, 0, zoff
    tab += mine
    return 0, depth, z


def png_read(files, rows, cols, lanes, waves=8, shift=0):
    """[(status, raster or None)] as cct_png_read_batch gives them: the walk above, the three emulated kernels, and the status
    rules of png_read_pass; also the chunk table, for the callers that assert what it holds"""
    tab, zoffs, fst, bpp, status, base, zoff = [], [0], [], [], [], 0, 0
    for i, f in enumerate(files):
        st, depth, zoff = png_walk(f, base, i, rows, cols, tab, zoff)
        status.append(st)
        zoffs.append(zoff)
        fst.append(PNG_ST_SKIP if st else 0)
        bpp.append(depth // 8 if not st else 2)
        base += len(f)
    if all(status):
        return [(st, None) for st in status], tab
    blob = b"".join(files)
    with tempfile.TemporaryDirectory() as d:
        d += os.sep
        with open(d + "png_in.bin", "wb") as f:
            f.write(struct.pack("<IIQ", len(files), len(tab), len(blob)) + struct.pack(f"<{len(zoffs)}Q", *zoffs) + struct.pack(f"<{len(fst)}I", *fst)
                    + bytes(bpp) + b"".join(struct.pack("<QQII", *c) for c in tab) + blob)
        subprocess.run([EMU, "png", str(lanes), str(waves), str(rows), str(cols), str(shift), d + "png_in.bin", d + "png_out.bin"], check=True)
        with open(d + "png_out.bin", "rb") as f:
            b = f.read()
    words = struct.unpack_from(f"<{3 * len(files)}I", b, 0)
    img = np.frombuffer(b, np.uint16, offset=12 * len(files)).reshape(len(files), rows, cols)
    out = []
    for i, f in enumerate(files):
        st, (f_st, z_st, size) = status[i], words[3 * i:3 * i + 3]
        want = rows * (1 + cols * bpp[i])
        if not st:
            if f_st & PNG_ST_CRC:
                st = pf.E_CRC
            elif z_st & ST_ZLIB:  # png_valid_stream_of_wrong_length
                z = ds.oracle_verdict(b"".join(blob[c[0] + 4:c[0] + 4 + c[2]] for c in tab if c[3] == i | PNG_CHUNK_IDAT))
                st = pf.E_STREAM if z is not None and len(z) != want else pf.E_ZLIB
            elif z_st & ST_STREAM or size != want or f_st & PNG_ST_FILTER:
                st = pf.E_STREAM
        out.append((st, img[i] if not st else None))
    return out, tab


def png_expect(cases, rows, cols, lanes, waves=8, shift=0):
    """cases: [(name, file, samples or None, status)]"""
    try:
        got, tab = png_read([c[1] for c in cases], rows, cols, lanes, waves, shift)
    except subprocess.CalledProcessError as e:
        raise AssertionError(f"lanes {lanes}, waves {waves}: emu exit status {e.returncode} (its report is above) on the files {[c[0] for c in cases][:4]} ...") from None
    for (name, _, img, want), (st, raster) in zip(cases, got):
        assert st == want, (name, st, want, lanes, waves)
        assert want or np.array_equal(raster, np.asarray(img) >> shift), (name, lanes, waves)
    return tab


def edge_shapes():
    """the shapes of png_files.ROWS x COLS of at most 4096 samples; (129, 1) and (129, 2) are among them: three bands, the band
    hand-off"""
    shapes = [(r, c) for r in pf.ROWS for c in pf.COLS if r * c <= 4096]
    assert (129, 1) in shapes
    return shapes


def alignment_cases():
    """(24 x 21) files whose IDAT chunks of 8 bytes and more lie at every (source, destination) alignment modulo 4"""
    out = []
    for t in range(4):
        for c in range(4):
            img = pf._img((24, 21), 100 + 4 * t + c)
            out.append((f"align-{t}-{c}", pf.make_png(img, 16, 4, cuts=[9 + c, 50, 51, 52, 53], before=[(b"tEXt", b"k\0" + b"x" * t)]), img, 0))
    return out


def run_png_core(lanes, both_orders=True):
    """chunk_cases and damaged_cases"""
    png_expect([c + (0,) for c in pf.chunk_cases()], 24, 21, lanes)
    png_expect(list(pf.damaged_cases()), *pf.DAMAGED_SHAPE, lanes)
    if both_orders:
        png_expect(list(pf.damaged_cases())[::-1], *pf.DAMAGED_SHAPE, lanes)
    print(f"png chunk_cases and damaged_cases ok at {lanes} lanes")


def run_png(lanes):
    run_png_core(lanes)
    al = alignment_cases()
    tab = png_expect(al, 24, 21, lanes, shift=4)
    assert {(c[0] + 4) % 4 * 4 + c[1] % 4 for c in tab if c[3] & PNG_CHUNK_IDAT and c[2] >= 8} == set(range(16))
    shapes = edge_shapes()
    for r, c in shapes:
        png_expect([e + (0,) for e in pf.edge_batch(r, c)], r, c, lanes)
    for waves in (1, 2, 4, 8):  # a raster of three bands at every number of waves
        png_expect([e + (0,) for e in pf.edge_batch(129, 1)], 129, 1, lanes, waves)
    print(f"png ok at {lanes} lanes: alignments, {len(shapes)} edge shapes, 129 rows at 1, 2, 4 and 8 waves")


RUNS = {"hand": run_hand, "walk": run_walk, "damage": run_damage, "skip": run_skip, "png": run_png}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("corpora", nargs="*", default=list(RUNS))
    ap.add_argument("--lanes", type=int, action="append")
    ap.add_argument("--no-build", action="store_true")
    a = ap.parse_args()
    if not a.no_build:
        build()
    for what in a.corpora:
        for lanes in a.lanes or LANES:
            RUNS[what](lanes)
