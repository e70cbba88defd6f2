"""CPU model of the TIFF writer and reader (cct_hip.tiff_encode_batch / tiff_info / tiff_read_batch), in plain Python.

    lzw_encode(strip)                     libtiff's LZW coder: greedy, Clear when the next free entry is 4094, codes MSB first
    lzw_decode(data, want)                -> (verdict, bytes): the reader's rules, each stated where it is applied
    strips_of(raster, predictor, rps)     the strip payloads: little-endian samples, horizontal differences for predictor 2
    write_file(raster, compression, ..)   the whole file in the layout Pillow / libtiff write
    parse(file)                           the first IFD with every refusal (Refused("CCT_E_TIFF"))
    read(file, rows, cols, bits)          a status name, or the raster
    foreign_files() / damaged_files() / refused_files() / raster_cases() / census()

LZW numbering: after a Clear the codes, Clear and EOI included, are counted from 1.  Code j has 9 bits for j <= 254, 10 for
j <= 766, 11 for j <= 1790, 12 beyond; code j >= 2 defines table entry 256 + j (the string of code j - 1 plus the first byte
of code j's).  The coder's Clear is code 3837.  Pillow (libtiff) is the oracle of tests/test_tiff_host.py.
"""
import io
import struct
import zlib

import numpy as np

STRIP_SIZE = 65536     # TiffImagePlugin.STRIP_SIZE
CLEAR, EOI = 256, 257
MAX_J = 4862           # code 4862 defines entry 5118, the last of libtiff's table (CSIZE = 5119)
COMPRESSION = {"none": 1, "lzw": 5, "deflate": 8}


class Refused(Exception):
    pass


def width(j):
    return 9 + (j > 254) + (j > 766) + (j > 1790)


# ---- LZW ------------------------------------------------------------------------------------------------------------

CHECK_GAP = 10000      # libtiff's LZWEncode looks at the compression ratio every so many input bytes


def lzw_codes(s, clear_every=0, eoi=True, trace=None):
    """[(code, bits)] of the strip bytes s, as libtiff's LZWEncode / LZWPostEncode write them: the greedy parse, a Clear when
    the next free entry is 4094, and a Clear when the compression ratio has fallen.  The ratio rule: the coder counts input
    bytes and output bits since the last Clear; after a code that neither filled the table nor widened the codes, once the
    input count has reached the checkpoint (10000 at the start of the strip), the checkpoint becomes the count + 10000 and
    the ratio (bytes << 8) // bits is taken: if it is not above the last one noted, a Clear follows and the counts and the
    noted ratio return to 0 (the checkpoint stays), else it is noted.  Only strips that compress well get that far: at
    fewer than 2.6 bytes a code the table fills first and resets the counts.
    clear_every=k: a foreign coder that also clears after every k codes.
    trace (a list): trace[L - 1] becomes the number, counted from the last Clear, of the LAST data code of the prefix s[:L]."""
    out = [(CLEAR, 9)]
    w, nxt, table, since = 9, 258, {}, 0
    incount, outcount, checkpoint, ratio = 1, 9, CHECK_GAP, 0
    omega = s[0]
    if trace is not None:
        trace.append(1)

    def clear():
        nonlocal w, nxt, table, since, incount, outcount, ratio
        out.append((CLEAR, w))
        incount, outcount, ratio = 0, w, 0
        table, nxt, w, since = {}, 258, 9, 0

    def wrote_data(at_end=False):
        nonlocal w, nxt, since, checkpoint, ratio
        nxt += 1
        since += 1
        if nxt == 4094 or (clear_every and since == clear_every):
            clear()
        elif nxt == 1 << w:
            w += 1
        elif incount >= checkpoint and not at_end:
            checkpoint = incount + CHECK_GAP
            rat = (incount << 8) // outcount if incount <= 0x7FFFFF else (incount // (outcount >> 8) if outcount >> 8 else 0x7FFFFFFF)
            if rat <= ratio:
                clear()
            else:
                ratio = rat

    for b in s[1:]:
        incount += 1
        key = omega << 8 | b
        if key in table:
            omega = table[key]
        else:
            out.append((omega, w))
            outcount += w
            table[key] = nxt
            wrote_data()
            omega = b
        if trace is not None:
            trace.append(since + 1)
    out.append((omega, w))
    wrote_data(at_end=True)
    if eoi:
        out.append((EOI, w))
    return out


def pack_codes(codes):
    acc = n = 0
    for c, w in codes:
        acc = acc << w | c
        n += w
    pad = -n % 8
    return (acc << pad).to_bytes((n + pad) // 8, "big")


def lzw_encode(s, **kw):
    return pack_codes(lzw_codes(s, **kw))


def lzw_decode(data, want):
    """("OK", bytes) or ("CCT_E_STREAM", None)"""
    nbits, pos = 8 * len(data), 0
    big = int.from_bytes(data, "big")

    def get(w):
        nonlocal pos
        if pos + w > nbits:
            return None
        pos += w
        return big >> (nbits - pos) & ((1 << w) - 1)

    if get(9) != CLEAR:
        return "CCT_E_STREAM", None                 # a strip opens with a Clear
    out, j, start, length = bytearray(), 0, [], []
    while len(out) < want:                          # decoding stops once the strip's bytes are out: the rest is ignored
        j += 1
        c = get(width(j))
        if c is None or c == EOI:
            return "CCT_E_STREAM", None             # the data or an EOI ends the strip early
        if c == CLEAR:                              # repeated Clears are allowed
            j, start, length = 0, [], []
            continue
        if j > MAX_J:
            return "CCT_E_STREAM", None             # the table is full and no Clear came: code 4863 may still be that Clear
        if c < 256:
            s = bytes([c])
        else:
            ref = c - 257                           # entry c = the string of code `ref` plus the first byte of code ref + 1
            if ref >= j:
                return "CCT_E_STREAM", None         # beyond the next free entry; for j = 1: not a literal after a Clear
            a = start[ref - 1]
            s = bytes(out[a:a + length[ref - 1]])
            s += s[:1] if ref + 1 == j else bytes(out[start[ref]:start[ref] + 1])   # ref + 1 == j: KwKwK
        start.append(len(out))
        length.append(len(s))
        out += s
    return "OK", bytes(out[:want])                  # a last string longer than what is left is cut; no EOI is needed


# ---- predictor and strips ---------------------------------------------------------------------------------------------

def rows_per_strip(rows, cols, itemsize, rps=None):
    if rps is None:
        rps = max(1, STRIP_SIZE // (cols * itemsize))
    return min(rows, rps)


def predict(raster, predictor):
    """the rows as the strips hold them, little-endian"""
    a = np.ascontiguousarray(raster)
    if predictor == 2:
        d = a.copy()
        d[:, 1:] = a[:, 1:] - a[:, :-1]             # modulo 2^bits: the dtype wraps
        a = d
    return a.astype(a.dtype.newbyteorder("<"))


def strips_of(raster, predictor=1, rps=None):
    rows, cols = raster.shape
    rps = rows_per_strip(rows, cols, raster.dtype.itemsize, rps)
    p = predict(raster, predictor)
    return [p[r:r + rps].tobytes() for r in range(0, rows, rps)], rps


def unpredict(rowbytes, rows, cols, bits, big, predictor):
    dt = np.dtype(np.uint8 if bits == 8 else (">u2" if big else "<u2"))
    a = np.frombuffer(rowbytes, dtype=dt).reshape(rows, cols).astype(np.uint8 if bits == 8 else np.uint16)
    if predictor == 2:
        a = np.cumsum(a, axis=1, dtype=np.uint64).astype(a.dtype)
    return a


def code_strip(strip, compression, level=6):
    if compression == 5:
        return lzw_encode(strip)
    if compression == 8:
        return zlib.compress(strip, level)
    return strip


# ---- files ------------------------------------------------------------------------------------------------------------

def write_file(raster, compression="lzw", predictor=1, rps=None, level=6):
    """Pillow's layout: II, strips from offset 8 back to back, a zero byte if they end on an odd offset, the IFD, then
    StripByteCounts and StripOffsets (inline for a single strip)."""
    comp = COMPRESSION[compression]
    rows, cols = raster.shape
    strips, rps = strips_of(raster, predictor, rps)
    coded = [code_strip(s, comp, level) for s in strips]
    body = b"".join(coded)
    offs, at = [], 8
    for c in coded:
        offs.append(at)
        at += len(c)
    pad = at & 1
    ifd = at + pad
    tags = [(256, 3, cols), (257, 3, rows), (258, 3, 8 * raster.dtype.itemsize), (259, 3, comp), (262, 3, 1), (273, 4, None), (278, 3, rps),
            (279, 4, None), (284, 3, 1)] + ([(317, 3, 2)] if predictor == 2 else [])
    n = len(coded)
    # libtiff (tif_dirwrite.c, WriteAsLong4) types the byte counts of several strips before it knows them: SHORT (two of them
    # inline) when ten times a full strip's bytes stay below 65535, taking a coded strip for ten times its rows at worst;
    # uncompressed, when the strip's bytes do
    full = rps * cols * raster.dtype.itemsize
    short = n > 1 and (full <= 0xFFFF if comp == 1 else full < 0xFFFF // 10)
    csize = 2 if short else 4
    counts_at = ifd + 2 + 12 * len(tags) + 4
    offs_at = counts_at + (csize * n if csize * n > 4 else 0)
    cfmt = f"<{n}{'H' if short else 'I'}"
    e = struct.pack("<H", len(tags))
    for tag, typ, val in tags:
        if tag == 273:
            e += struct.pack("<HHII", tag, typ, n, offs_at if n > 1 else 8)
        elif tag == 279 and csize * n <= 4:
            e += struct.pack("<HHI", tag, 3 if short else 4, n) + struct.pack(cfmt, *[len(c) for c in coded]).ljust(4, b"\0")
        elif tag == 279:
            e += struct.pack("<HHII", tag, 3 if short else 4, n, counts_at)
        else:
            e += struct.pack("<HHIHH", tag, typ, 1, val, 0)
    e += struct.pack("<I", 0)
    if csize * n > 4:
        e += struct.pack(cfmt, *[len(c) for c in coded])
    if n > 1:
        e += struct.pack(f"<{n}I", *offs)
    return b"II*\0" + struct.pack("<I", ifd) + body + b"\0" * pad + e


def pillow_file(raster, compression="lzw", predictor=1, rps=None):
    """the same raster through Pillow / libtiff (level 6 for Deflate)"""
    from PIL import Image, TiffImagePlugin
    rows, cols = raster.shape
    old = TiffImagePlugin.STRIP_SIZE
    if rps is not None:
        TiffImagePlugin.STRIP_SIZE = min(rows, rps) * cols * raster.dtype.itemsize
    try:
        buf = io.BytesIO()
        Image.fromarray(raster).save(buf, "TIFF", compression={"lzw": "tiff_lzw", "deflate": "tiff_adobe_deflate"}[compression],
                                     tiffinfo={317: 2} if predictor == 2 else {})
        return buf.getvalue()
    finally:
        TiffImagePlugin.STRIP_SIZE = old


def same_file(ours, pillows):
    """byte for byte, but for the pad byte in front of an IFD that follows an odd number of strip bytes: libtiff seeks over it,
    and Pillow's in-memory file then holds whatever its buffer held there (mostly 0, not always); the writer stores 0"""
    d = parse(ours)
    end = max(a + c for a, c in zip(d["offs"], d["counts"]))
    if end & 1 and len(ours) == len(pillows) and ours[end] == 0:
        pillows = pillows[:end] + b"\0" + pillows[end + 1:]
    return ours == pillows


def pillow_read(file):
    """the raster, or "OSError" """
    from PIL import Image
    try:
        im = Image.open(io.BytesIO(file))
        im.load()
    except (OSError, SyntaxError, ValueError, struct.error, EOFError):
        return "OSError"
    return np.array(im)


def parse(file):
    """dict(rows, cols, bits, compression (1 / 5 / 8), predictor, rps, big, offs, counts) or Refused("CCT_E_TIFF")"""
    f, ln = bytes(file), len(file)

    def no():
        raise Refused("CCT_E_TIFF")

    if ln < 8 or f[:2] not in (b"II", b"MM"):
        no()
    big = f[:2] == b"MM"
    o = ">" if big else "<"
    if struct.unpack_from(o + "H", f, 2)[0] != 42:                # 43: BigTIFF
        no()
    ifd = struct.unpack_from(o + "I", f, 4)[0]
    if ifd < 8 or ifd > ln or ln - ifd < 2:
        no()
    ntags = struct.unpack_from(o + "H", f, ifd)[0]
    if ntags == 0 or 12 * ntags > ln - ifd - 2:
        no()
    seen, d = {}, dict(compression=1, predictor=1, rps=0xFFFFFFFF, big=big)
    for k in range(ntags):
        e = ifd + 2 + 12 * k
        tag, typ, count = struct.unpack_from(o + "HHI", f, e)
        single = tag in (256, 257, 258, 259, 262, 266, 277, 278, 284, 317, 339)
        if tag in (322, 323, 324, 325):                             # tiles
            no()
        if not single and tag not in (273, 279):
            continue                                                # unknown tags are ignored
        if typ not in (3, 4) or count == 0 or count > 0x10000000:
            no()
        size = 2 if typ == 3 else 4
        at = e + 8
        if count * size > 4:
            at = struct.unpack_from(o + "I", f, e + 8)[0]
            if at > ln or count * size > ln - at:
                no()
        v = list(struct.unpack_from(o + str(count) + ("H" if typ == 3 else "I"), f, at))
        if single and count != 1:
            no()
        seen[tag] = v
    for tag in (256, 257, 258, 262, 273, 279):
        if tag not in seen:
            no()
    for tag, must in ((262, 1), (266, 1), (277, 1), (284, 1), (339, 1)):
        if tag in seen and seen[tag][0] != must:
            no()
    d.update(cols=seen[256][0], rows=seen[257][0], bits=seen[258][0])
    d["compression"] = seen.get(259, [1])[0]
    d["predictor"] = seen.get(317, [1])[0]
    rps = seen.get(278, [0xFFFFFFFF])[0]
    if d["bits"] not in (8, 16) or not 1 <= d["rows"] <= 65535 or not 1 <= d["cols"] <= 65535:
        no()
    if d["compression"] == 32946:
        d["compression"] = 8
    if d["compression"] not in (1, 5, 8):
        no()
    if d["predictor"] != 1 and not (d["predictor"] == 2 and d["compression"] != 1):
        no()
    if rps == 0:
        no()
    d["rps"] = min(rps, d["rows"])
    n = -(-d["rows"] // d["rps"])
    d["offs"], d["counts"] = seen[273], seen[279]
    if len(d["offs"]) != n or len(d["counts"]) != n:
        no()
    for a, c in zip(d["offs"], d["counts"]):
        if a > ln or c > ln - a:                                    # a strip outside the file
            no()
    return d


def info(file):
    d = parse(file)
    return d["rows"], d["cols"], d["bits"]


def read(file, rows=None, cols=None, bits=None):
    """the raster, or "CCT_E_TIFF" / "CCT_E_STREAM" / "CCT_E_ZLIB" """
    try:
        d = parse(file)
    except Refused as r:
        return str(r)
    if (rows, cols, bits) != (None, None, None) and (d["rows"], d["cols"], d["bits"]) != (rows, cols, bits):
        return "CCT_E_TIFF"
    row_bytes = d["cols"] * d["bits"] // 8
    got, status = [], None
    for s, (a, c) in enumerate(zip(d["offs"], d["counts"])):
        want = min(d["rps"], d["rows"] - s * d["rps"]) * row_bytes
        data = file[a:a + c]
        if d["compression"] == 1:
            if c < want:
                return "CCT_E_STREAM"                               # decided on the host, before the others are looked at
            got.append(data[:want])
            continue
        if c == 0:
            return "CCT_E_STREAM"
        if d["compression"] == 5:
            verdict, b = lzw_decode(data, want)
            if verdict != "OK":
                status = status or verdict
                continue
        else:
            try:
                z = zlib.decompressobj()
                b = z.decompress(data, want + 1)
                if len(b) != want or not z.eof:                     # a strip is one whole zlib stream of exactly its rows
                    status = status or ("CCT_E_STREAM" if len(b) != want and z.eof else "CCT_E_ZLIB")
                    continue
            except zlib.error:
                status = status or "CCT_E_ZLIB"
                continue
        got.append(b)
    if status:
        return status
    return unpredict(b"".join(got), d["rows"], d["cols"], d["bits"], d["big"], d["predictor"])


def build_file(raster, compression=5, predictor=1, rps=None, order="II", short_tables=False, spp=False, unknown=False, pad_odd=False,
               reverse=False, code=None, trailing=b"", compression_tag=None, counts_delta=None, tags_extra=(), drop=(), override=None):
    """A file another writer could have made: IFD entries sorted by tag, out-of-line values behind the IFD.  code(strip,
    index) -> coded bytes replaces the coder; trailing bytes follow every strip inside its byte count; counts_delta =
    {index: d} states a byte count that is off by d; override = {tag: (type, [values])}."""
    o = "<" if order == "II" else ">"
    rows, cols = raster.shape
    bits = 8 * raster.dtype.itemsize
    strips, rps = strips_of(raster, predictor, rps)
    if order == "MM" and bits == 16:
        strips = [np.frombuffer(s, "<u2").astype(">u2").tobytes() for s in strips]
    coded = [(code(s, i) if code else code_strip(s, compression)) + trailing for i, s in enumerate(strips)]
    n = len(coded)
    body, offs, at = b"", [0] * n, 8
    for i in (reversed(range(n)) if reverse else range(n)):
        if pad_odd and at & 1:
            body += b"\0"
            at += 1
        offs[i] = at
        body += coded[i]
        at += len(coded[i])
    if at & 1:
        body += b"\0"
        at += 1
    counts = [len(c) + (counts_delta or {}).get(i, 0) for i, c in enumerate(coded)]
    tt = 3 if short_tables else 4
    tags = {256: (3, [cols]), 257: (3, [rows]), 258: (3, [bits]), 259: (3, [compression_tag or compression]), 262: (3, [1]),
            273: (tt, offs), 278: (3, [rps]), 279: (tt, counts), 284: (3, [1])}
    if predictor == 2:
        tags[317] = (3, [2])
    if spp:
        tags[277] = (3, [1])
    if unknown:
        tags[305] = (2, b"a writer\0")              # Software, ASCII, out of line
        tags[65000] = (4, [1, 2, 3])                # private
    for t in tags_extra:
        tags[t[0]] = (t[1], t[2])
    for t, v in (override or {}).items():
        tags[t] = v
    for t in drop:
        del tags[t]
    ifd = at
    extra_at = ifd + 2 + 12 * len(tags) + 4
    e, extra = struct.pack(o + "H", len(tags)), b""
    for tag in sorted(tags):
        typ, vals = tags[tag]
        if typ == 2:
            raw, count = bytes(vals), len(vals)
        else:
            raw, count = struct.pack(o + str(len(vals)) + ("H" if typ == 3 else "I"), *vals), len(vals)
        e += struct.pack(o + "HHI", tag, typ, count)
        if len(raw) <= 4:
            e += raw.ljust(4, b"\0")
        else:
            e += struct.pack(o + "I", extra_at + len(extra))
            extra += raw + b"\0" * (len(raw) & 1)
    e += struct.pack(o + "I", 0)
    return (b"II*\0" if order == "II" else b"MM\0*") + struct.pack(o + "I", ifd) + body + e + extra


# ---- rasters ------------------------------------------------------------------------------------------------------------

def _rng(seed):
    return np.random.default_rng(seed)


def raster_cases():
    """[(name, raster, rows_per_strip values)]: the smallest shapes that reach the edges"""
    r = _rng(317)
    smooth = (np.add.outer(np.arange(37), np.arange(50)) * 9 + r.integers(0, 3, (37, 50))).astype(np.uint16)
    wrap16 = np.zeros((4, 9), np.uint16); wrap16[:, ::2] = 65535
    wrap8 = np.zeros((4, 9), np.uint8); wrap8[:, 1::2] = 255
    ratio = r.integers(0, 2, (48, 512)).astype(np.uint8); ratio[:22] = 9    # flat, then coin flips: a Clear at the second checkpoint
    periodic = np.tile(np.arange(7, dtype=np.uint16) * 1000, (64, 74))[:, :512]
    return [
        ("1x1_u8", np.array([[200]], np.uint8), [None]),
        ("1x2_u8", np.array([[3, 250]], np.uint8), [None]),
        ("3x7_u8", r.integers(0, 256, (3, 7)).astype(np.uint8), [None, 1, 2]),
        ("5x3_u8", r.integers(0, 4, (5, 3)).astype(np.uint8), [None, 1, 7]),
        ("1x1_u16", np.array([[40000]], np.uint16), [None]),
        ("9x1_u16", r.integers(0, 65536, (9, 1)).astype(np.uint16), [None, 1, 7]),       # one column: no differences
        ("2x65_u16", r.integers(0, 65536, (2, 65)).astype(np.uint16), [None, 1]),        # a row crosses a wave's span
        ("3x300_u8", r.integers(0, 256, (3, 300)).astype(np.uint8), [None, 2]),
        ("wrap_u16", wrap16, [None]),
        ("wrap_u8", wrap8, [None]),
        ("smooth_37x50", smooth, [None, 1, 7, 37]),                                      # rows % 7 != 0
        ("noise_16x512", r.integers(0, 65536, (16, 512)).astype(np.uint16), [16]),      # 16 KiB in one strip: table-full Clears
        ("flat_64x512", np.full((64, 512), 1234, np.uint16), [None]),                    # long strings, KwKwK chains
        ("periodic_64x512", periodic, [None]),
        ("ratio_48x512_u8", ratio, [48]),
        ("2x6552_u8", np.tile(np.arange(6552, dtype=np.uint16) // 9 % 251, (2, 1)).astype(np.uint8), [1]),   # byte counts still SHORT
        ("2x6553_u8", np.tile(np.arange(6553, dtype=np.uint16) // 9 % 251, (2, 1)).astype(np.uint8), [1]),   # LONG from here on                                                # 24 KiB in one strip: the ratio falls
    ]


def trim_for_last_code(s, target):
    """the shortest prefix length of s whose LAST data code is code `target` after a Clear"""
    trace = []
    lzw_codes(s, trace=trace)
    return trace.index(target) + 1


def edge_strips():
    """[(name, strip bytes)]: strips whose last data code is exactly the 254th, 766th, 1790th and 3836th after a Clear (EOI
    at the new width, or behind a Clear), and one that ends with the first code after a Clear"""
    noise = _rng(9).integers(0, 256, 9000).astype(np.uint8).tobytes()
    out = [(f"last_code_{t}", noise[:trim_for_last_code(noise, t)]) for t in (254, 766, 1790, 3836)]
    trace = []
    lzw_codes(noise, trace=trace)
    first_after_clear = next(L for L in range(4000, len(trace)) if trace[L - 1] == 1) if 1 in trace[4000:] else None
    out.append(("one_code_after_clear", noise[:first_after_clear]))
    return out


def census(strips):
    """what the LZW streams of `strips` (bytes objects) reach"""
    c = dict(ratio_clears=0, last_code=set(), eoi_after_clear=0, one_code_after_clear=0, clears=0, bit_residues=set(), dword_straddles=0, eoi_widths=set())
    for s in strips:
        codes = lzw_codes(s)
        pos, since = 0, 0
        for k, (code, w) in enumerate(codes):
            c["bit_residues"].add(pos % 8)
            if pos // 32 != (pos + w - 1) // 32:
                c["dword_straddles"] += 1
            pos += w
            if code == CLEAR:
                c["clears"] += k > 0
                c["ratio_clears"] += k > 0 and since != 3836
                since = 0
            elif code == EOI:
                c["eoi_widths"].add(w)
                if codes[k - 1][0] == CLEAR:
                    c["eoi_after_clear"] += 1
                    c["last_code"].add(3836)
                else:
                    c["last_code"].add(since)
                if since == 1:
                    c["one_code_after_clear"] += k > 2
            else:
                since += 1
        verdict, back = lzw_decode(pack_codes(codes), len(s))
        assert verdict == "OK" and back == s
    return c


# ---- foreign, damaged and refused files ----------------------------------------------------------------------------------

def _fixture_raster():
    r = _rng(42)
    return (np.add.outer(np.arange(23), np.arange(40)) * 30 + r.integers(0, 40, (23, 40))).astype(np.uint16)


def foreign_files():
    """[(name, file, raster)]: files another writer could have made, all taken"""
    a = _fixture_raster()
    a8 = (a >> 4).astype(np.uint8)
    noise = _rng(5).integers(0, 65536, (16, 512)).astype(np.uint16)
    out = []
    for order in ("II", "MM"):
        for comp in (1, 5, 8):
            for pred in ((1,) if comp == 1 else (1, 2)):
                for rps in (23, 7, 1):
                    for arr, dn in ((a, "u16"), (a8, "u8")):
                        out.append((f"{order}_c{comp}_p{pred}_rps{rps}_{dn}", build_file(arr, comp, pred, rps, order, spp=True, pad_odd=True), arr))
    out += [
        ("deflate_32946", build_file(a, 8, 2, 7, compression_tag=32946), a),
        ("short_tables", build_file(a, 5, 2, 7, short_tables=True), a),
        ("short_tables_mm", build_file(a8, 8, 1, 5, order="MM", short_tables=True), a8),
        ("unknown_tags", build_file(a, 5, 1, 7, unknown=True, spp=True), a),
        ("fillorder_sampleformat", build_file(a, 5, 2, 7, tags_extra=[(266, 3, [1]), (339, 3, [1])]), a),
        ("no_rows_per_strip", build_file(a, 5, 1, 23, drop=(278,)), a),
        ("long_dimensions", build_file(a, 5, 1, 7, override={256: (4, [40]), 257: (4, [23]), 278: (4, [7])}), a),
        ("rps_beyond_rows", build_file(a, 5, 2, 23, override={278: (4, [1 << 20])}), a),
        ("out_of_order", build_file(a, 5, 2, 4, reverse=True, pad_odd=True), a),
        ("out_of_order_deflate", build_file(a, 8, 2, 4, reverse=True), a),
        ("no_eoi", build_file(a, 5, 2, 7, code=lambda s, i: lzw_encode(s, eoi=False)), a),
        ("trailing_bytes", build_file(a, 5, 1, 7, trailing=b"\xff\x00\x80"), a),
        ("trailing_bytes_none", build_file(a8, 1, 1, 7, trailing=b"\xff\x00\x80"), a8),
    ]
    for k in (1, 2, 5, 64, 65, 255, 300, 1000):
        out.append((f"clear_every_{k}", build_file(noise, 5, 1, 16, code=lambda s, i, k=k: lzw_encode(s, clear_every=k)), noise))
    out.append(("repeated_clears", build_file(a, 5, 2, 7, code=lambda s, i: pack_codes([(CLEAR, 9)] * 3 + lzw_codes(s)[1:])), a))
    return out


def _recode(s, at, value=None, insert=None):
    """the strip's code list with the data code at position `at` (counted over the data codes, negative from the end)
    replaced by value(j) -- j its number after the Clear -- or with `insert` put before it"""
    codes = lzw_codes(s)
    data = [k for k, (c, w) in enumerate(codes) if c not in (CLEAR, EOI)]
    k = data[at]
    j = k - max(q for q in range(k) if codes[q][0] == CLEAR)
    if insert is not None:
        # the codes behind the insertion keep their widths: only what comes before it matters to a reader that stops there
        return pack_codes(codes[:k] + [(insert, codes[k][1])] + codes[k:])
    return pack_codes(codes[:k] + [(value(j), codes[k][1])] + codes[k + 1:])


def damaged_files():
    """[(name, file, raster)]: what read() says of each is what Pillow must say (OSError for a status name)"""
    a = _fixture_raster()
    a8 = (a >> 4).astype(np.uint8)
    out = []

    def lzw_case(name, coder, only=1, **kw):
        out.append((name, build_file(a, 5, 2, 7, code=lambda s, i: coder(s) if i == only else lzw_encode(s), **kw), a))

    lzw_case("truncated_strip", lambda s: lzw_encode(s)[:len(lzw_encode(s)) // 2])
    lzw_case("truncated_by_3_bytes", lambda s: lzw_encode(s)[:-3])
    lzw_case("early_eoi", lambda s: _recode(s, 40, insert=EOI))
    lzw_case("beyond_table_first", lambda s: _recode(s, 1, value=lambda j: 257 + j))
    lzw_case("beyond_table_middle", lambda s: _recode(s, 100, value=lambda j: 257 + j))
    lzw_case("beyond_table_last", lambda s: _recode(s, -1, value=lambda j: 257 + j))
    lzw_case("beyond_table_far", lambda s: _recode(s, 100, value=lambda j: 511))
    lzw_case("kwkwk_forged_middle", lambda s: _recode(s, 100, value=lambda j: 256 + j))      # legal: decodes to other bytes
    lzw_case("non_literal_after_clear", lambda s: _recode(s, 0, value=lambda j: 258))
    lzw_case("non_literal_after_clear_last_strip", lambda s: _recode(s, 0, value=lambda j: 300), only=3)
    lzw_case("no_opening_clear_eoi_first", lambda s: pack_codes([(EOI, 9)] + lzw_codes(s)[1:]))
    # (an uncompressed strip whose byte count is one too small is not in this list: Pillow returns a raster for it, the
    # missing byte being whatever its buffer held; the reader refuses it: short_uncompressed_files())
    for comp, arr, dn in ((5, a, "lzw"), (1, a8, "none")):
        for d in (-1, 1):
            for which in (0, 3):
                if comp == 1 and d < 0:
                    continue
                out.append((f"count_{'minus' if d < 0 else 'plus'}_1_{dn}_strip{which}", build_file(arr, comp, 2 if comp == 5 else 1, 7, counts_delta={which: d}), arr))

    def flip(s, at, bit):
        z = bytearray(zlib.compress(s, 6))
        z[at] ^= 1 << bit
        return bytes(z)

    # (no flip in the last bits of the DEFLATE data: libtiff stops inflating once the rows are out, so Pillow returns the raster
    # where zlib, and the reader, which read a stream to its end, report the stream)
    for at, bit in ((0, 3), (1, 0), (2, 1), (20, 5), (-1, 0)):
        out.append((f"deflate_flip_{at}_{bit}", build_file(a, 8, 2, 7, code=lambda s, i, at=at, bit=bit: flip(s, at % len(zlib.compress(s, 6)), bit) if i == 2 else zlib.compress(s, 6)), a))
    out.append(("deflate_truncated", build_file(a, 8, 2, 7, code=lambda s, i: zlib.compress(s, 6)[:-9] if i == 1 else zlib.compress(s, 6)), a))
    out.append(("deflate_short_rows", build_file(a, 8, 1, 7, code=lambda s, i: zlib.compress(s[:-2] if i == 1 else s, 6)), a))
    return out


def short_uncompressed_files():
    """[(name, file)]: CCT_E_STREAM by the host's own check; Pillow is no judge of these (see damaged_files)"""
    a8 = (_fixture_raster() >> 4).astype(np.uint8)
    return [(f"count_minus_1_none_strip{which}", build_file(a8, 1, 1, 7, counts_delta={which: -1})) for which in (0, 3)]


def refused_files():
    """[(name, file)]: CCT_E_TIFF, every one, decided by the structure alone"""
    a = _fixture_raster()
    good = build_file(a, 5, 2, 7)
    big = bytearray(good); big[2] = 43
    return [
        ("empty", b""),
        ("short_header", good[:7]),
        ("not_tiff", b"\x89PNG\r\n\x1a\n" + good[8:]),
        ("bigtiff", bytes(big)),
        ("ifd_outside", good[:4] + struct.pack("<I", len(good) + 10) + good[8:]),
        ("ifd_cut", good[:struct.unpack_from("<I", good, 4)[0] + 30]),
        ("packbits", build_file(a, 5, 1, 7, compression_tag=32773)),
        ("jpeg", build_file(a, 5, 1, 7, compression_tag=7)),
        ("predictor_on_uncompressed", build_file(a, 1, 1, 7, tags_extra=[(317, 3, [2])])),
        ("predictor_3", build_file(a, 5, 1, 7, tags_extra=[(317, 3, [3])])),
        ("min_is_white", build_file(a, 5, 1, 7, override={262: (3, [0])})),
        ("rgb", build_file(a, 5, 1, 7, override={262: (3, [2])})),
        ("two_samples", build_file(a, 5, 1, 7, tags_extra=[(277, 3, [2])])),
        ("twelve_bits", build_file(a, 5, 1, 7, override={258: (3, [12])})),
        ("signed_samples", build_file(a, 5, 1, 7, tags_extra=[(339, 3, [2])])),
        ("fill_order_2", build_file(a, 5, 1, 7, tags_extra=[(266, 3, [2])])),
        ("planar_2", build_file(a, 5, 1, 7, override={284: (3, [2])})),
        ("tiles", build_file(a, 5, 1, 7, tags_extra=[(322, 3, [16]), (323, 3, [16])])),
        ("no_strip_offsets", build_file(a, 5, 1, 7, drop=(273,))),
        ("no_strip_byte_counts", build_file(a, 5, 1, 7, drop=(279,))),
        ("no_photometric", build_file(a, 5, 1, 7, drop=(262,))),
        ("too_few_strips", build_file(a, 5, 1, 7, override={278: (3, [5])})),
        ("strip_outside", build_file(a, 5, 1, 7, counts_delta={3: 4000})),
        ("rows_per_strip_0", build_file(a, 5, 1, 7, override={278: (3, [0])})),
        ("ascii_dimension", build_file(a, 5, 1, 7, override={256: (2, b"40\0")})),
    ]
