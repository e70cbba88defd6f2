"""Hand-placed and damaged JPEG Lossless files for the decoder, and what tests/jpeg_lossless_model.py says of each.

Plain numpy and the model: no device, no golden file, fixed seeds.  Every entry is (name, file, rows, cols, bits); the
expectation of a file is verdicts()[name]: the raster of jpeg_lossless_model.decode_frame, or the kind of JpegError it
raises.

PLACEMENT FILES (placement_files) are well formed.  Their table, ALIGNED8, gives each of the 17 categories an 8-bit word, so
a zero difference is one byte (00) and a difference of category 8 is two (08, then its 8 extra bits: FF for +255).  The number
of two-byte samples in a row of 1100 therefore puts a 0xFF extra byte, or the RST marker behind the row, on any chosen offset
of the scan.  The decoder's unstuff kernel walks the scan 2048 bytes a step, 8 bytes a lane, every lane looking one byte back
and one ahead: each pattern below is built with its first byte on every offset 2040 .. 2056 (the step border) and on
1500 .. 1507 (the lane border 1504 inside a step).
    ff00       FF 00            a stuffed byte inside an interval
    rst        FF Dn            the marker behind row 0
    fill1_rst  FF FF Dn         one fill byte (T.81 B.1.1.2) in front of it
    fill2_rst  FF FF FF Dn      two
    ff00_rst   FF 00 FF Dn      a stuffed 0xFF as the last data byte of an interval
    ff00ff00   FF 00 FF 00 FF Dn  precision 16: no word of ALIGNED8 starts with a one bit, so sixteen ones in a row exist
                                only as the 15 extra bits of +32767 and one pad bit, at the end of an interval
Differences of category 8 move an 8-bit sample across 128, so a 0xFF extra byte (0 -> 255) needs an odd number of them before
it; where the wanted offset has the other parity a second 0xFF early in the row shifts the scan by its stuffed byte.  Further
files put fill bytes in front of EOI (one fill starts on the last byte of a step) and, at 3 rows, the second RST on 4096 - 2
.. 4096 + 2, where the kept-byte and RST counts carried between steps have been carried twice.

DAMAGE FAMILIES (damage_files) apply named damages to six base files: bit flips aimed at magnitude bits and at code words,
truncations and spare zero bytes behind the last interval and behind one that is not the last, an RST removed, doubled or
renumbered, a byte turned into 0xFF, two intervals swapped, and under the flat 5-bit table words outside the table in the
first and second window of 256 subsequences.  DAMAGE_SUB[name] is the subsequence (1024 bits of unstuffed data) of the
interval in which the damage begins: no fault can show before it.
"""
import functools

import numpy as np

import jpeg_lossless_model as m

ALIGNED8 = ([0] * 7 + [17] + [0] * 8, list(range(17)))  # every category an 8-bit word: 00 .. 10
CODE16 = ([1] * 14 + [0, 3], list(range(17)))           # categories 14 .. 16 get 16-bit words: about 31 bits a sample of noise
SUB = 1024                                              # bits of a subsequence (csrc/cct_internal.h JPL_SUB)
STEP_OFFSETS = tuple(range(2040, 2057))                 # the first byte of a pattern, around the step border 2048
LANE_OFFSETS = tuple(range(1500, 1508))                 # and around the lane border 1504
PCOLS = 1100
EARLY_FF = 301                                          # where the parity-fixing 0xFF goes


# ---- placement ---------------------------------------------------------------------------------------------------------

def aligned_row(cols, length, ffs, rng):
    """Differences of one row of 8-bit samples that opens an interval (so it starts from 128) whose stuffed scan bytes under
    ALIGNED8 number `length`, with the extra byte 0xFF at every scan offset of ffs and at no other.  ValueError where the
    parity of the two-byte samples does not work out."""
    ffs = sorted(ffs)
    k = len(ffs)
    gaps, at = [], 0  # bytes in front of the 08 of each 0xFF sample, then the bytes behind the last
    for f in ffs:
        gaps.append(f - 1 - at)
        at = f + 2
    gaps.append(length - at)
    rest = length - 2 * k - cols - k  # two-byte samples that are not 0xFF ones, less one for each gap in front of a 0xFF
    if min(gaps) < 0 or rest < 0 or any(g < 2 for g in gaps[:k]):
        raise ValueError("no room")
    steps = [1] * k + [min(rest, gaps[k] // 2)]
    rest -= steps[k]
    if rest & 1:
        if not steps[k]:
            raise ValueError("parity")
        steps[k] -= 1
        rest += 1
    for i in range(k):
        add = min((gaps[i] // 2 - steps[i]) // 2 * 2, rest)
        steps[i] += add
        rest -= add
    if rest:
        raise ValueError("parity")
    d, v = [], 128
    for i, (g, t) in enumerate(zip(gaps, steps)):
        order = rng.permutation(np.arange(g - t) < t)  # g - t samples, t of them two bytes long
        j = 0
        for two in order:
            if not two:
                d.append(0)
                continue
            j += 1
            if v >= 128:
                w = 0 if (i < k and j == t) else int(rng.integers(0, v - 127))
            else:
                w = int(rng.integers(v + 128, min(255, v + 254) + 1))
            d.append(w - v)
            v = w
        if i < k:
            assert v == 0
            d.append(255)
            v = 255
    assert len(d) == cols, (len(d), cols)
    return d


def placed_row(cols, length, ffs, rng):
    try:
        return aligned_row(cols, length, ffs, rng)
    except ValueError:
        return aligned_row(cols, length, [EARLY_FF] + list(ffs), rng)


def aligned_file(rows_of_diffs, precision):
    """rows of differences, every row an interval of its own -> (file, scan offset, scan)"""
    d = np.array(rows_of_diffs, dtype=np.int64)
    x = (1 << (precision - 1)) + np.cumsum(d, axis=1)
    if precision == 8:
        assert x.min() >= 0 and x.max() <= 255
    img = (x & 0xFFFF).astype(np.uint8 if precision == 8 else np.uint16)
    f = m.encode_frame(img, precision, restart_rows=1, table=ALIGNED8)
    h = m.parse(f)
    return f, h["s0"], f[h["s0"]:h["s1"]]


def _filler(rng, cols=PCOLS):
    """a later row: some two-byte samples and one stuffed byte"""
    return placed_row(cols, cols + int(rng.integers(100, 900)), [int(rng.integers(400, 900))], rng)


@functools.lru_cache(maxsize=None)
def placement_files():
    out = []
    rng = np.random.default_rng(1100)
    for p in STEP_OFFSETS + LANE_OFFSETS:
        # FF 00 inside row 0
        f, s0, scan = aligned_file([placed_row(PCOLS, 2150, [p], rng), _filler(rng)], 8)
        assert scan[p:p + 2] == b"\xff\x00" and scan[p - 1] == 8 and scan[2150:2152] == b"\xff\xd0"
        out.append((f"ff00@{p}", f, 2, PCOLS, 8))
        # the RST on p, bare and behind one and two fill bytes
        f, s0, scan = aligned_file([placed_row(PCOLS, p, [], rng), _filler(rng)], 8)
        assert scan[p:p + 2] == b"\xff\xd0" and scan[p - 1] != 0xFF
        out.append((f"rst@{p}", f, 2, PCOLS, 8))
        for n in (1, 2):
            f, s0, scan = aligned_file([placed_row(PCOLS, p, [], rng), _filler(rng)], 8)
            assert scan[p:p + 2] == b"\xff\xd0"
            f = f[:s0 + p] + b"\xff" * n + f[s0 + p:]
            out.append((f"fill{n}_rst@{p}", f, 2, PCOLS, 8))
        # a stuffed 0xFF ends row 0
        f, s0, scan = aligned_file([placed_row(PCOLS, p + 2, [p], rng), _filler(rng)], 8)
        assert scan[p:p + 4] == b"\xff\x00\xff\xd0"
        out.append((f"ff00_rst@{p}", f, 2, PCOLS, 8))
        # precision 16: +32767 and a pad bit end row 0
        f, s0, scan = aligned_file([placed_row(PCOLS - 1, p - 1, [], rng) + [32767], _filler(rng)], 16)
        assert scan[p - 1:p + 6] == b"\x0f\xff\x00\xff\x00\xff\xd0"
        out.append((f"ff00ff00@{p}", f, 2, PCOLS, 16))
    # fill bytes in front of EOI: anywhere, and from the last byte of the second step on
    for tag, l0, l1 in (("", 1500, 1300), ("@4095", 2046, 2047)):
        for n in (1, 2):
            f, s0, scan = aligned_file([placed_row(PCOLS, l0, [], rng), placed_row(PCOLS, l1, [], rng)], 8)
            assert len(scan) == l0 + 2 + l1 and f[-2:] == b"\xff\xd9"
            out.append((f"fill{n}_eoi{tag}", f[:-2] + b"\xff" * n + f[-2:], 2, PCOLS, 8))
    # three intervals: the first RST across the first step border, the second around the second
    for delta in (-2, -1, 0, 1, 2):
        at = 4096 + delta
        f, s0, scan = aligned_file([placed_row(PCOLS, 2047, [], rng), placed_row(PCOLS, at - 2049, [1000], rng), _filler(rng)], 8)
        assert scan[2047:2049] == b"\xff\xd0" and scan[at:at + 2] == b"\xff\xd1"
        out.append((f"second_rst@{at}", f, 3, PCOLS, 8))
    return out


# ---- damage ------------------------------------------------------------------------------------------------------------

def scan_map(scan):
    """a well-formed scan without fill bytes -> ([scan positions of the data bytes of each interval], [positions of the RSTs])"""
    pos, rst, cur, i = [], [], [], 0
    while i < len(scan):
        if scan[i] == 0xFF and scan[i + 1] != 0:
            assert 0xD0 <= scan[i + 1] <= 0xD7
            rst.append(i)
            pos.append(np.array(cur, dtype=np.int64))
            cur = []
            i += 2
            continue
        cur.append(i)
        i += 2 if scan[i] == 0xFF else 1
    pos.append(np.array(cur, dtype=np.int64))
    return pos, rst


@functools.lru_cache(maxsize=None)
def bases():
    """tag -> (raster, precision, predictor, restart rows, table or None, bits)"""
    rng = np.random.default_rng(41)
    noise = rng.integers(0, 65536, (8, 300)).astype(np.uint16)
    const = np.full((64, 1000), 128, np.uint8)
    big = rng.integers(0, 65536, (24, 520)).astype(np.uint16)
    return {
        "noise_rr2": (noise, 16, 1, 2, None, 16),
        "noise_p4": (noise, 16, 4, 0, None, 16),
        "noise_flat5": (noise, 16, 1, 2, m.FLAT5, 16),
        "const_flat5": (const, 8, 1, 0, m.FLAT5, 8),
        "const_flat5_rr32": (const, 8, 1, 32, m.FLAT5, 8),
        "noise_code16": (big, 16, 1, 12, CODE16, 16),
    }


def base_file(tag):
    img, precision, ss, rr, table, bits = bases()[tag]
    return m.encode_frame(img, precision, ss, 0, rr, table=table)


DAMAGE_SUB = {}
TRUNCATIONS = (1, 2, 3, 130, 1000)


def _damages_of(tag):
    img, precision, ss, rr, table, bits = bases()[tag]
    rows, cols = img.shape
    rng = np.random.default_rng(sum(tag.encode()))
    d, rpi = m.differences(img, precision, ss, 0, rr)
    cat, _ = m.categories(d)
    if table is None:
        table = m.huffman_table(np.bincount(cat.ravel(), minlength=17))
    good = m.encode_frame(img, precision, ss, 0, rr, table=table)
    assert good == base_file(tag)
    h = m.parse(good)
    head, scan, tail = good[:h["s0"]], good[h["s0"]:h["s1"]], good[h["s1"]:]
    dpos, rpos = scan_map(scan)
    n_int = len(dpos)
    assert n_int == -(-rows // rpi)
    size = np.zeros(17, dtype=np.int64)
    for s, (_, ln) in m.codes_of(*table).items():
        size[s] = ln
    per = rpi * cols  # samples of a whole interval
    csize, nx = size[cat].ravel(), np.where(cat == 16, 0, cat).ravel()
    start = [np.cumsum((csize + nx)[k * per:(k + 1) * per]) - (csize + nx)[k * per:(k + 1) * per] for k in range(n_int)]
    first = [0] + [r + 2 for r in rpos]   # the scan range of every interval
    last = rpos + [len(scan)]
    out = []

    def put(name, s, sub):
        out.append((f"{tag}/{name}", head + bytes(s) + tail, rows, cols, bits))
        DAMAGE_SUB[f"{tag}/{name}"] = int(sub)

    def flip(name, k, *bits_at):
        s = bytearray(scan)
        for b in bits_at:
            s[dpos[k][b >> 3]] ^= 0x80 >> (b & 7)
        put(name, s, min(bits_at) // SUB)

    def word_in(k, sub):
        """a sample of interval k whose code word starts in subsequence `sub`, or the last one before it"""
        return int(min(np.searchsorted(start[k], sub * SUB) + 3, len(start[k]) - 1))

    put("undamaged", scan, 0)
    flat = table == m.FLAT5
    if not (flat and img.min() == img.max()):  # magnitude bits: the file stays valid, the raster changes
        with_bits = np.flatnonzero(nx > 0)
        for g in sorted(rng.choice(with_bits, 8, replace=False)):
            k, q = divmod(int(g), per)
            j = int(rng.integers(0, nx[g]))
            flip(f"flip_magnitude_bit{j}_of_sample{g}", k, int(start[k][q] + csize[g] + j))
    if flat:  # the top bit of a word makes it 1xxxx (outside the table unless it was 00000), the low bit another category
        k = n_int - 1
        nsub = -(-8 * len(dpos[k]) // SUB)
        aims = (("first_word", 0, 0), ("window1_last_sub", k, word_in(k, min(255, nsub - 2))),
                ("window2", k, word_in(k, min(280, nsub - 1))), ("last_word", k, len(start[k]) - 1))
        for name, kk, q in aims:
            flip(f"flip_code_top_bit_{name}", kk, int(start[kk][q]))
        for name, kk, q in aims[1:3]:
            flip(f"flip_code_low_bit_{name}", kk, int(start[kk][q]) + 4)
            if img.min() == img.max():
                flip(f"word_10001_{name}", kk, int(start[kk][q]), int(start[kk][q]) + 4)
    else:
        for g in sorted(rng.choice(rows * cols, 3, replace=False)):
            k, q = divmod(int(g), per)
            j = int(rng.integers(0, csize[g]))
            flip(f"flip_code_bit{j}_of_sample{g}", k, int(start[k][q] + j))
    where = [("last", n_int - 1)] + ([("middle", n_int - 2)] if n_int > 1 else [])
    for wname, k in where:
        for c in TRUNCATIONS:
            if last[k] - c > first[k]:
                put(f"cut_{c}_bytes_of_{wname}_interval", scan[:last[k] - c] + scan[last[k]:], 8 * np.searchsorted(dpos[k], last[k] - c) // SUB)
        for c in (1, 3):
            put(f"{c}_zero_bytes_behind_{wname}_interval", scan[:last[k]] + bytes(c) + scan[last[k]:], 8 * len(dpos[k]) // SUB)
    if n_int > 1:
        r = rpos[-1]
        put("rst_removed", scan[:r] + scan[r + 2:], 0)
        put("rst_doubled", scan[:r + 2] + scan[r:], 0)
        put("rst_renumbered", scan[:r + 1] + bytes([0xD0 + (scan[r + 1] + 1) % 8]) + scan[r + 2:], 0)
        a, b = n_int - 2, n_int - 1
        put("intervals_swapped", scan[:first[a]] + scan[first[b]:last[b]] + scan[last[a]:first[b]] + scan[first[a]:last[a]] + scan[last[b]:], 0)
    k = n_int // 2
    at = int(dpos[k][len(dpos[k]) // 2])
    put("byte_to_ff", scan[:at] + b"\xff" + scan[at + 1:], 8 * (len(dpos[k]) // 2) // SUB)
    return out


@functools.lru_cache(maxsize=None)
def damage_files():
    return [e for tag in bases() for e in _damages_of(tag)]


def base_of(name):
    return name.split("/")[0]


# ---- the model's word ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_files():
    out = placement_files() + damage_files()
    assert len({e[0] for e in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def verdicts():
    """name -> (0, raster) or (kind of the JpegError, None)"""
    out = {}
    for name, f, rows, cols, bits in all_files():
        try:
            out[name] = (0, m.decode_frame(f, rows, cols, bits))
        except m.JpegError as e:
            out[name] = (e.kind, None)
    return out


@functools.lru_cache(maxsize=None)
def base_rasters():
    """tag -> what the model decodes from the undamaged file"""
    return {tag: m.decode_frame(base_file(tag), *v[0].shape, v[5]) for tag, v in bases().items()}


def shapes():
    """(rows, cols, bits) -> the entries of that shape, in order"""
    out = {}
    for e in all_files():
        out.setdefault(e[2:], []).append(e)
    return out
