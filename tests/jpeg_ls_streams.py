"""Placed and damaged JPEG-LS files for the decoder, and what tests/jpeg_ls_model.py says of each.

Plain numpy and the model: no device, no golden file, fixed seeds.  Every entry is (name, file, rows, cols, bits); the
expectation of a file is verdicts()[name]: the raster of jpeg_ls_model.decode_frame, or the kind of JlsError it raises.

PLACEMENT FILES (placement_files) are well formed.  A JPEG-LS code adapts with every sample, so a 0xFF byte cannot be put on an
offset by construction as under a fixed Huffman table; it is found: noise rasters of PLACED_SHAPE are coded seed after seed,
and a file is kept when its scan has a 0xFF data byte (the byte behind it then carries 7 bits) on an offset of WANTED that
no file before it had.  WANTED covers 2 and 5 .. 15 (the decoder's reader loads eight bytes at a time at most; offsets 0, 1, 3 and 4
are not among the first 1500 seeds of this family: an interval of noise opens with the 0 bit of an empty run), and the bytes
around 64 and 128 (the encoder's stuffing takes 64 bytes a round, from wherever the round before ended).  placement_rasters()
are the rasters of those files: the device's encoder has to write the same bytes.  Further files end an interval in FF 00
(END_FF: found the same way among files of one line an interval), and state preset parameters in an LSE segment: MAXVAL
below 2^P - 1 (a RANGE that is no power of two among them), thresholds and RESET of the caller's.

DAMAGE FAMILIES (damage_files) apply named damages to the base files: flipped bits, cuts and spare zero bytes behind the
last interval and behind one that is not the last, an RST removed, doubled or renumbered, two intervals swapped, a byte
turned into 0xFF (which makes a marker of it when the byte behind it is 0x80 or more)."""
import functools

import numpy as np

import jpeg_ls_model as m

WANTED = (2,) + tuple(range(5, 16)) + tuple(range(56, 72)) + tuple(range(120, 136))
PLACED_SHAPE = (1, 72)
CUTS = (1, 2, 3, 20)


def scan_of(f):
    h = m.parse(f)
    return h["intervals"]


# ---- placement ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _placed():
    """[(name, raster, file)]"""
    out, missing, seed = [], set(WANTED), 0
    while missing:
        x = np.random.default_rng(seed).integers(0, 65536, PLACED_SHAPE).astype(np.uint16)
        f = m.encode_frame(x, 16)
        a, b = scan_of(f)[0]
        hit = sorted(o for o in missing if a + o < b - 1 and f[a + o] == 0xFF)
        if hit:
            missing -= set(hit)
            out.append((f"ff@{'+'.join(map(str, hit))}", x, f))
        seed += 1
        assert seed <= 1500
    return out


@functools.lru_cache(maxsize=None)
def _end_ff():
    """rasters of one line an interval, with an interval that ends in FF 00: the last one of the file, and an earlier one"""
    out, want, seed = [], {"last", "inner"}, 0
    while want:
        x = np.random.default_rng(1000 + seed).integers(0, 4096, (6, 40)).astype(np.uint16)
        f = m.encode_frame(x, 12, 1)
        iv = scan_of(f)
        ends = [k for k, (a, b) in enumerate(iv) if f[b - 2:b] == b"\xff\x00"]
        kind = "last" if ends and ends[-1] == len(iv) - 1 else "inner" if ends else None
        if kind in want:
            want.discard(kind)
            out.append((f"end_ff_{kind}", x, f))
        seed += 1
        assert seed < 20000
    return out


@functools.lru_cache(maxsize=None)
def _lse():
    rng = np.random.default_rng(55)
    rr, cc = np.mgrid[0:9, 0:70]
    smooth = (100 + 60 * np.sin(rr / 2.0) * np.cos(cc / 6.0) + rng.integers(0, 4, (9, 70))).astype(np.int64)
    smooth[4:6, 10:50] = 77
    out = []
    for tag, x, p, rst, lse in (
            ("maxval200", np.minimum(smooth, 200).astype(np.uint8), 8, 2, dict(maxval=200)),
            ("maxval1000", (smooth * 5).astype(np.uint16), 12, 0, dict(maxval=1000)),
            ("maxval1", (smooth & 1).astype(np.uint8), 2, 3, dict(maxval=1)),
            ("thresholds", smooth.astype(np.uint8), 8, 0, dict(t1=5, t2=9, t3=30)),
            ("thresholds_1_1_1", smooth.astype(np.uint8), 8, 4, dict(t1=1, t2=1, t3=1)),
            ("reset3", smooth.astype(np.uint8), 8, 0, dict(reset=3)),
            ("reset255_noise", rng.integers(0, 4096, (9, 70)).astype(np.uint16), 12, 0, dict(reset=255)),
            ("reset4095", (smooth * 16).astype(np.uint16), 12, 0, dict(reset=4095, maxval=4095, t1=18, t2=67, t3=276))):
        out.append((f"lse_{tag}", x, m.encode_frame(x, p, rst, lse=lse)))
    return out


def placement_rasters():
    """[(name, raster, precision, restart rows, file)]: what the device's encoder has to write byte for byte"""
    return [(n, x, 16, 0, f) for n, x, f in _placed()] + [(n, x, 12, 1, f) for n, x, f in _end_ff()]


@functools.lru_cache(maxsize=None)
def placement_files():
    return [(n, f, *x.shape, 8 if x.dtype == np.uint8 else 16) for n, x, f in _placed() + _end_ff() + _lse()]


# ---- damage ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bases():
    """tag -> (raster, precision, restart rows, lse or None)"""
    rng = np.random.default_rng(41)
    stripes = np.zeros((12, 70), dtype=np.uint16)
    stripes[:, ::7] = 4095
    rr, cc = np.mgrid[0:9, 0:64]
    smooth = (128 + 90 * np.sin(rr / 3.0) * np.cos(cc / 5.0) + rng.integers(0, 3, (9, 64))).astype(np.uint8)
    return {
        "noise_rr2": (rng.integers(0, 65536, (6, 70)).astype(np.uint16), 16, 2, None),
        "stripes": (stripes, 12, 0, None),
        "smooth_rr3": (smooth, 8, 3, None),
        "smooth_lse": (np.minimum(smooth, 200), 8, 3, dict(maxval=200, t1=4, t2=8, t3=20, reset=32)),
    }


def base_file(tag):
    x, p, rst, lse = bases()[tag]
    return m.encode_frame(x, p, rst, lse=lse)


def _damages_of(tag):
    x, p, rst, lse = bases()[tag]
    rows, cols = x.shape
    bits = 8 if x.dtype == np.uint8 else 16
    good = base_file(tag)
    iv = scan_of(good)
    n_int = len(iv)
    rng = np.random.default_rng(sum(tag.encode()))
    out = []

    def put(name, f):
        out.append((f"{tag}/{name}", bytes(f), rows, cols, bits))

    put("undamaged", good)
    s0, s1 = iv[0][0], iv[-1][1]
    for at in sorted(rng.choice(8 * (s1 - s0), 12, replace=False)):
        f = bytearray(good)
        f[s0 + at // 8] ^= 0x80 >> (at & 7)
        put(f"flip_bit{at}", f)
    where = [("last", n_int - 1)] + ([("middle", n_int - 2)] if n_int > 1 else [])
    for wname, k in where:
        a, b = iv[k]
        for c in CUTS:
            if b - c > a:
                put(f"cut_{c}_bytes_of_{wname}_interval", good[:b - c] + good[b:])
        for c in (1, 3):
            put(f"{c}_zero_bytes_behind_{wname}_interval", good[:b] + bytes(c) + good[b:])
    if n_int > 1:
        r = iv[-1][0] - 2  # the last RST
        put("rst_removed", good[:r] + good[r + 2:])
        put("rst_doubled", good[:r + 2] + good[r:])
        put("rst_renumbered", good[:r + 1] + bytes([0xD0 + (good[r + 1] + 1) % 8]) + good[r + 2:])
        (a0, b0), (a1, b1) = iv[-2], iv[-1]
        put("intervals_swapped", good[:a0] + good[a1:b1] + good[b0:a1] + good[a0:b0] + good[b1:])
    a, b = iv[n_int // 2]
    for j, at in enumerate(sorted(rng.choice(np.arange(a, b - 1), 4, replace=False))):
        put(f"byte_to_ff_{j}", good[:at] + b"\xff" + good[at + 1:])
    return out


@functools.lru_cache(maxsize=None)
def damage_files():
    return [e for tag in bases() for e in _damages_of(tag)]


# ---- the model's word ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_files():
    out = placement_files() + damage_files()
    assert len({e[0] for e in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def verdicts():
    """name -> (0, raster) or (kind of the JlsError, None)"""
    out = {}
    for name, f, rows, cols, bits in all_files():
        try:
            out[name] = (0, m.decode_frame(f, rows, cols, bits))
        except m.JlsError as e:
            out[name] = (e.kind, None)
    return out


def shapes():
    """(rows, cols, bits) -> the entries of that shape, in order"""
    out = {}
    for e in all_files():
        out.setdefault(e[2:], []).append(e)
    return out
