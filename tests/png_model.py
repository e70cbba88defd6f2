"""CPU model of the 16-bit grayscale PNG that Pillow writes (PngImagePlugin + ZipEncode.c), the reference the device
PNG writer (csrc/png_kernels.hip, cct_png_encode_batch) is tested against.  Test infrastructure only: the product never
imports it.

    rows    samples (v << shift) & 0xFFFF, big-endian (bpp = 2), row -1 = zeros.  Per row the filter whose bytes have the
            least sum of min(v, 256 - v): None first, then Up, Sub, Paeth, each tried only while the best sum is > 0 and
            taken only when strictly smaller (Average only under optimize=True).
    stream  zlib.compressobj(level, DEFLATED, 15, memLevel 9, Z_FILTERED) of the filtered rows, one shot
    file    signature, IHDR (depth 16, color type 0), IDAT chunks of max(65536, 4 * cols) bytes (the last one shorter), IEND
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MEM_LEVEL, Z_FILTERED = 9, 1


def samples(img, shift):
    return ((np.asarray(img).astype(np.uint32) << shift) & 0xFFFF).astype(np.uint16)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img, shift=0):
    """(rows, cols) uint16 -> (filter types, filtered bytes of rows * (1 + 2 cols))"""
    s = samples(img, shift)
    rows, cols = s.shape
    raw = s.astype(">u2").view(np.uint8).reshape(rows, 2 * cols).astype(np.int32)
    prev = np.vstack([np.zeros((1, 2 * cols), np.int32), raw[:-1]])
    left = np.hstack([np.zeros((rows, 2), np.int32), raw[:, :-2]])
    upleft = np.hstack([np.zeros((rows, 2), np.int32), prev[:, :-2]])
    cand = {0: raw, 2: raw - prev, 1: raw - left, 4: raw - _paeth(left, prev, upleft)}
    cand = {f: v & 255 for f, v in cand.items()}
    cost = {f: np.where(v < 128, v, 256 - v).sum(axis=1) for f, v in cand.items()}
    out = np.empty((rows, 1 + 2 * cols), np.uint8)
    types = np.zeros(rows, np.uint8)
    for r in range(rows):
        best, f = int(cost[0][r]), 0
        for g in (2, 1, 4):
            if best > 0 and int(cost[g][r]) < best:
                best, f = int(cost[g][r]), g
        types[r] = f
        out[r, 0] = f
        out[r, 1:] = cand[f][r]
    return types, out.tobytes()


def zlib_stream(filtered, level):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, MEM_LEVEL, Z_FILTERED)
    return c.compress(filtered) + c.flush()


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_bytes(img, level=6, shift=0):
    """What Image.fromarray(samples(img, shift)).save(f, "PNG", compress_level=level) writes"""
    level = 6 if level == -1 else level
    rows, cols = np.asarray(img).shape
    z = zlib_stream(filter_rows(img, shift)[1], level)
    size = max(65536, 4 * cols)
    parts = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 16, 0, 0, 0, 0))]
    parts += [chunk(b"IDAT", z[i:i + size]) for i in range(0, len(z), size)]
    parts.append(chunk(b"IEND", b""))
    return b"".join(parts)


def pillow_bytes(img, level=6, shift=0):
    import io

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(samples(img, shift)).save(buf, "PNG", compress_level=6 if level == -1 else level)
    return buf.getvalue()


def chunks(png):
    """[(type, data)] of a PNG file"""
    assert png[:8] == SIGNATURE
    out, p = [], 8
    while p < len(png):
        n = struct.unpack(">I", png[p:p + 4])[0]
        out.append((png[p + 4:p + 8], png[p + 8:p + 8 + n]))
        p += 12 + n
    return out


def idat_stream(png):
    return b"".join(d for t, d in chunks(png) if t == b"IDAT")


def cases():
    """Seeded shapes the tests run on both sides: name -> (rows, cols) uint16"""
    rng = np.random.default_rng(2026)
    smooth = np.add.outer(np.arange(97) * 300, np.arange(131) * 7).astype(np.uint16)
    return {
        "1x1": rng.integers(0, 65536, (1, 1), dtype=np.uint16),
        "1xN": rng.integers(0, 4096, (1, 777), dtype=np.uint16),
        "Nx1": rng.integers(0, 4096, (613, 1), dtype=np.uint16),
        "odd": rng.integers(0, 2000, (37, 51), dtype=np.uint16),
        "wide": rng.integers(0, 65536, (3, 16500), dtype=np.uint16),  # chunks of 4 * cols bytes
        "zero": np.zeros((64, 80), np.uint16),
        "const": np.full((50, 60), 1234, np.uint16),
        "random": rng.integers(0, 65536, (300, 257), dtype=np.uint16),
        "smooth": smooth,
    }
