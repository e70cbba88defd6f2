"""PNG files built by hand for the device PNG reader (cct_png_read_batch / png_read_batch): a generator with a chosen filter
type per row, depth 8 or 16, arbitrary IDAT cut points, extra chunks, zlib parameters and an override for the raw zlib stream,
and the seeded case lists that tests/test_png_read_host.py (Pillow reads every file) and tests/test_gpu_png_read.py (the device
reads every file) share.  Test infrastructure only: the product never imports it.  Pure Python + numpy + zlib."""
import functools
import struct
import zlib

import numpy as np

import png_model as pm

SIGNATURE = pm.SIGNATURE
chunk = pm.chunk
ROWS = (1, 2, 63, 64, 65, 129)
COLS = (1, 2, 63, 64, 65, 300)
SHIFTS = (0, 4, 15)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def raw_rows(img, depth):
    """(rows, cols) samples -> (rows, cols * depth/8) bytes as they stand in an unfiltered PNG row"""
    img = np.asarray(img)
    if depth == 16:
        return img.astype(">u2").view(np.uint8).reshape(img.shape[0], 2 * img.shape[1])
    assert depth == 8 and int(img.max(initial=0)) < 256
    return img.astype(np.uint8)


def filtered(img, depth, types):
    """filter byte + filtered row for every row (PNG spec 9.2), filter types[r] for row r (0 .. 4, anything else is written as
    it is with an unfiltered row)"""
    raw = raw_rows(img, depth).astype(np.int32)
    bpp = depth // 8
    rows, nb = raw.shape
    prev = np.vstack([np.zeros((1, nb), np.int32), raw[:-1]])
    left = np.hstack([np.zeros((rows, bpp), np.int32), raw[:, :-bpp]])[:, :nb]
    upleft = np.hstack([np.zeros((rows, bpp), np.int32), prev[:, :-bpp]])[:, :nb]
    pred = {1: left, 2: prev, 3: (left + prev) >> 1, 4: _paeth(left, prev, upleft)}
    out = np.empty((rows, 1 + nb), np.uint8)
    for r in range(rows):
        f = int(types[r])
        out[r, 0] = f
        out[r, 1:] = (raw[r] - pred[f][r]) & 255 if f in pred else raw[r]
    return out.tobytes()


def deflate(data, level=6, wbits=15, strategy=0):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(data) + c.flush()


def ihdr(rows, cols, depth=16, color=0, compression=0, method=0, interlace=0):
    return struct.pack(">IIBBBBB", cols, rows, depth, color, compression, method, interlace)


def cut(stream, cuts):
    """the IDAT payloads of a stream: cuts = a list of lengths (the rest goes into one last chunk), or an int for chunks of
    that many bytes, or None for one chunk"""
    if cuts is None:
        return [stream]
    if isinstance(cuts, int):
        return [stream[i:i + cuts] for i in range(0, len(stream), cuts)] or [b""]
    parts, p = [], 0
    for n in cuts:
        parts.append(stream[p:p + n])
        p += n
    parts.append(stream[p:])
    return parts


def assemble(chunks):
    """[(type, data)] -> file"""
    return SIGNATURE + b"".join(chunk(t, d) for t, d in chunks)


def make_png(img, depth=16, filters=4, cuts=None, before=(), between=None, after=(), level=6, wbits=15, strategy=0, stream=None,
             header=None, end=True):
    """A grayscale PNG of the samples img.  filters: one type for every row or a sequence; before / after: chunks around the
    IDATs; between: (k, type, data) puts a chunk in front of IDAT k; stream: the raw zlib stream instead of the real one;
    header: IHDR data instead of the real one; end=False leaves IEND out."""
    img = np.asarray(img)
    rows, cols = img.shape
    types = [filters] * rows if isinstance(filters, (int, np.integer)) else list(filters)
    if stream is None:
        stream = deflate(filtered(img, depth, types), level, wbits, strategy)
    chunks = [(b"IHDR", header if header is not None else ihdr(rows, cols, depth))] + list(before)
    for k, part in enumerate(cut(stream, cuts)):
        if between is not None and between[0] == k:
            chunks.append((between[1], between[2]))
        chunks.append((b"IDAT", part))
    chunks += list(after)
    if end:
        chunks.append((b"IEND", b""))
    return assemble(chunks)


def flip(data, pos, bit=1):
    b = bytearray(data)
    b[pos] ^= bit
    return bytes(b)


# ---- unfilter edges ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_batch(rows, cols):
    """One shape's files: depths 8 and 16 x (each filter type alone, a seeded random type per row) x (values 0 .. 6, so that
    Paeth ties and Average carries occur, and the full range).  -> [(name, file, samples uint16)]"""
    out = []
    for depth in (8, 16):
        for small in (True, False):
            for fsel in (0, 1, 2, 3, 4, "mix"):
                rng = np.random.default_rng([rows, cols, depth, int(small), 9 if fsel == "mix" else fsel])
                img = rng.integers(0, 7 if small else 1 << depth, (rows, cols), dtype=np.uint16)
                if small and depth == 16:  # small differences in both bytes of a sample
                    img = (img * 257 + rng.integers(0, 3, (rows, cols)).astype(np.uint16) * 256).astype(np.uint16)
                types = rng.integers(0, 5, rows) if fsel == "mix" else [fsel] * rows
                name = f"{rows}x{cols}-d{depth}-{'small' if small else 'full'}-f{fsel}"
                out.append((name, make_png(img, depth, types, level=1 if small else 6), img))
    return out


# ---- chunk layer -------------------------------------------------------------------------------------------------------------
def _img(shape, seed, depth=16, hi=None):
    rng = np.random.default_rng(seed)
    return rng.integers(0, hi or (1 << depth), shape, dtype=np.uint16)


@functools.lru_cache(maxsize=None)
def chunk_cases():
    """[(name, file, samples)] of one shape (24 x 21): what the chunk walk and png_unpack_kernel must take"""
    shape = (24, 21)
    out = []

    def add(name, seed, depth=16, **kw):
        img = _img(shape, seed, depth)
        out.append((name, make_png(img, depth, kw.pop("filters", 4), **kw), img))
    add("one-byte-idats", 1, cuts=1)
    add("empty-idats-start-middle-end", 2, cuts=[0, 0, 100, 0, 0, 50])
    z = deflate(filtered(_img(shape, 3), 16, [1] * 24))
    out.append(("empty-idat-last", make_png(_img(shape, 3), 16, 1, cuts=[len(z)]), _img(shape, 3)))
    add("cut-in-zlib-header", 4, cuts=[1, 0, 1, 3])
    z = deflate(filtered(_img(shape, 5), 16, [2] * 24))
    out.append(("cut-in-adler", make_png(_img(shape, 5), 16, 2, cuts=[len(z) - 2]), _img(shape, 5)))
    out.append(("cut-in-adler-bytewise", make_png(_img(shape, 5), 16, 2, cuts=[len(z) - 4, 1, 1, 1]), _img(shape, 5)))
    anc = [(b"tEXt", b"k\0" + bytes(range(n - 2)) if n >= 2 else b"x" * n) for n in (0, 1, 2, 3, 255, 256, 257)]
    add("ancillary-lengths-before", 6, before=anc)
    add("ancillary-lengths-after", 7, after=anc, depth=8)
    add("text-and-phys", 8, before=[(b"tEXt", b"Title\0x"), (b"pHYs", struct.pack(">IIB", 2835, 2835, 1))])
    add("stored-blocks", 9, level=0)
    add("fixed-huffman", 10, strategy=zlib.Z_FIXED)
    add("wbits-9", 11, wbits=9, filters=0, depth=8)
    add("huffman-only-8bit", 12, strategy=zlib.Z_HUFFMAN_ONLY, depth=8, filters=3)
    return out


@functools.lru_cache(maxsize=None)
def big_idat_case():
    """one IDAT chunk larger than 64 KiB (incompressible samples)"""
    img = _img((200, 300), 21)
    f = make_png(img, 16, 0, level=1)
    assert max(len(d) for t, d in pm.chunks(f) if t == b"IDAT") > 65536
    return "idat-above-64k", f, img


# ---- refusals ----------------------------------------------------------------------------------------------------------------
E_ZLIB, E_STREAM, E_MIXED, E_PNG, E_CRC = 2, 4, 10, 11, 12
DAMAGED_SHAPE = (33, 40)


@functools.lru_cache(maxsize=None)
def damaged_cases():
    """[(name, file, samples or None, status)] of one shape: good files and one file of each damaged kind.  status is the
    CCT_E_* code the reader must give the file (0: samples must come back exactly)."""
    rows, cols = DAMAGED_SHAPE
    img = _img(DAMAGED_SHAPE, 31)
    img8 = _img(DAMAGED_SHAPE, 32, 8)
    types = np.random.default_rng(33).integers(0, 5, rows)
    rowbytes = filtered(img, 16, types)
    z = deflate(rowbytes)
    good = make_png(img, 16, types, before=[(b"tEXt", b"Comment\0fine")])
    parts = pm.chunks(good)
    out = [("good-16", good, img, 0), ("good-8", make_png(img8, 8, types, cuts=7), img8, 0)]

    def bad(name, f, status):
        out.append((name, f, None, status))
    idat_at = good.index(b"IDAT")
    bad("data-byte-flipped", flip(good, idat_at + 4 + 20), E_CRC)
    bad("ancillary-byte-flipped", flip(good, good.index(b"tEXt") + 4 + 3), E_CRC)
    tail = make_png(img, 16, types, after=[(b"tEXt", b"Comment\0fine")])
    bad("ancillary-byte-flipped-behind-the-idats", flip(tail, tail.index(b"tEXt") + 4 + 3), E_CRC)
    bad("ihdr-crc-flipped", flip(good, 8 + 8 + 13), E_CRC)
    bad("adler-flipped", make_png(img, 16, types, stream=flip(z, len(z) - 1)), E_ZLIB)
    bad("stream-61-short", make_png(img, 16, types, stream=deflate(rowbytes[:-61])), E_STREAM)
    bad("stream-61-long", make_png(img, 16, types, stream=deflate(rowbytes + bytes(61))), E_STREAM)
    bad("stream-one-row-short", make_png(img, 16, types, stream=deflate(rowbytes[:-(1 + 2 * cols)])), E_STREAM)
    five = bytearray(rowbytes)
    five[7 * (1 + 2 * cols)] = 5
    bad("filter-byte-5", make_png(img, 16, types, stream=deflate(bytes(five))), E_STREAM)
    bad("truncated", good[:idat_at + 30], E_PNG)
    bad("truncated-in-a-head", good[:idat_at - 2], E_PNG)
    bad("no-iend", make_png(img, 16, types, end=False), E_PNG)
    bad("bytes-after-iend", good + b"\0", E_PNG)
    bad("idats-separated", make_png(img, 16, types, cuts=[40], between=(1, b"tEXt", b"k\0v")), E_PNG)
    bad("no-idat", assemble([p for p in parts if p[0] != b"IDAT"]), E_PNG)
    bad("bad-signature", b"\x89PNX" + good[4:], E_PNG)
    bad("ihdr-not-first", assemble([(b"tEXt", b"k\0v")] + parts), E_PNG)
    bad("chunk-length-past-the-file", good[:idat_at - 4] + struct.pack(">I", len(good)) + good[idat_at:], E_PNG)
    for color in (2, 3, 4, 6):
        bad(f"colour-type-{color}", make_png(img, 16, types, header=ihdr(rows, cols, 8, color)), E_PNG)
    bad("depth-4", make_png(img, 16, types, header=ihdr(rows, cols, 4)), E_PNG)
    bad("interlace-1", make_png(img, 16, types, header=ihdr(rows, cols, 16, interlace=1)), E_PNG)
    bad("unknown-critical-chunk", make_png(img, 16, types, before=[(b"ABCd", b"1234")]), E_PNG)
    bad("plte", make_png(img, 16, types, before=[(b"PLTE", bytes(6))]), E_PNG)
    bad("other-size", make_png(_img((rows, cols + 1), 34), 16, 4), E_MIXED)
    out.append(("good-16-again", make_png(img[::-1], 16, 3, cuts=[0, 5]), np.ascontiguousarray(img[::-1]), 0))
    return out
