"""CPU model of the 8-bit grayscale PNG that Pillow writes, the reference the 8-bit device PNG writer (png_filter8_kernel,
cct_png_encode8_batch) is tested against; the 16-bit model's rules (tests/png_model.py, imported) at bpp = 1.  Test
infrastructure only: the product never imports it.

    samples window8: a uint16 value through the window (lo, hi) to a byte, in integers only; uint8 rasters as they are
    rows    bpp = 1: the left neighbour is the previous pixel, row -1 = zeros; Pillow's costs, order and rule as in png_model
    stream  png_model.zlib_stream: memLevel 9, Z_FILTERED
    file    IHDR of depth 8, color type 0; IDAT chunks of max(65536, 4 * cols) bytes
"""
import os
import struct
import zlib

import numpy as np

import png_model as pm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEVELS = (4, 6, 9)


def window8(img, lo, hi):
    """y = ((clamp(v, lo, hi) - lo) * 510 + w) // (2 w), w = hi - lo: round((v - lo) * 255 / w), halves up.  No floats."""
    lo, hi = int(lo), int(hi)
    assert 0 <= lo < hi <= 65535
    w = hi - lo
    c = np.clip(np.asarray(img).astype(np.int64), lo, hi)
    return (((c - lo) * 510 + w) // (2 * w)).astype(np.uint8)


def filter_rows8(samples):
    """(rows, cols) uint8 -> (filter types, filtered bytes of rows * (1 + cols))"""
    raw = np.asarray(samples)
    assert raw.dtype == np.uint8 and raw.ndim == 2
    rows, cols = raw.shape
    raw = raw.astype(np.int32)
    prev = np.vstack([np.zeros((1, cols), np.int32), raw[:-1]])
    left = np.hstack([np.zeros((rows, 1), np.int32), raw[:, :-1]])
    upleft = np.hstack([np.zeros((rows, 1), np.int32), prev[:, :-1]])
    cand = {0: raw, 2: raw - prev, 1: raw - left, 4: raw - pm._paeth(left, prev, upleft)}
    cand = {f: v & 255 for f, v in cand.items()}
    cost = {f: np.where(v < 128, v, 256 - v).sum(axis=1) for f, v in cand.items()}
    out = np.empty((rows, 1 + cols), np.uint8)
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


def png8_bytes(samples, level=6):
    """What Image.fromarray(samples).save(f, "PNG", compress_level=level) writes for a (rows, cols) uint8 array"""
    level = 6 if level == -1 else level
    rows, cols = np.asarray(samples).shape
    z = pm.zlib_stream(filter_rows8(samples)[1], level)
    size = max(65536, 4 * cols)
    parts = [pm.SIGNATURE, pm.chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, 0, 0, 0, 0))]
    parts += [pm.chunk(b"IDAT", z[i:i + size]) for i in range(0, len(z), size)]
    parts.append(pm.chunk(b"IEND", b""))
    return b"".join(parts)


def pillow8_bytes(samples, level=6):
    import io

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(samples, dtype=np.uint8)).save(buf, "PNG", compress_level=6 if level == -1 else level)
    return buf.getvalue()


def load_slice(name):
    with open(os.path.join(GOLDEN, name + ".u16.zz"), "rb") as f:
        return np.frombuffer(zlib.decompress(f.read()), dtype="<u2").reshape(512, 512).copy()


_CASES = None


def cases():
    """name -> (source raster, window or None).  uint8 sources are written as they are; uint16 sources go through their window.
    Built once and shared: callers must not write into the arrays."""
    global _CASES
    if _CASES is None:
        rng = np.random.default_rng(2027)
        ramp = np.add.outer(np.arange(97) * 300, np.arange(131) * 7).astype(np.uint16)  # png_model's smooth ramp
        s671 = load_slice("slice0671")
        u8 = lambda shape: rng.integers(0, 256, shape, dtype=np.uint8)  # noqa: E731
        _CASES = {
            "u8_1x1": (u8((1, 1)), None),
            "u8_1x67": (u8((1, 67)), None),  # no row above
            "u8_37x1": (u8((37, 1)), None),  # no left neighbour
            "u8_5x65": ((np.add.outer(np.arange(5) * 9, np.arange(65) * 3) + rng.integers(0, 3, (5, 65))).astype(np.uint8), None),
            "u8_7x129": ((np.arange(7)[:, None] * 31 + rng.integers(0, 4, (1, 129)) * 40 + rng.integers(0, 2, (7, 129))).astype(np.uint8), None),
            "u8_zeros16": (np.zeros((16, 16), np.uint8), None),  # cost 0: the search stops at None
            "u8_noise300x401": (u8((300, 401)), None),
            "u8_3x20000": (u8((3, 20000)), None),
            "u8_4x520": (u8((4, 520)) // 16 * 16, None),  # the writer's 8-pixel groups: a lane's second step, whole group
            "u16_3x515": (rng.integers(900, 1300, (3, 515), dtype=np.uint16), (864, 1264)),  # second step, 3 pixels left over
            "u16_9x8": (rng.integers(0, 65536, (9, 8), dtype=np.uint16), (0, 65535)),  # one whole group per row
            "u16_ramp": (ramp, (1000, 20000)),
            "slice0671_w0_1600": (s671, (0, 1600)),
            "slice0671_w864_1264": (s671, (864, 1264)),
            "slice0671_w1000_1001": (s671, (1000, 1001)),
            "slice0671_w0_65535": (s671, (0, 65535)),
        }
        for src, _ in _CASES.values():
            src.setflags(write=False)
    return _CASES


def samples_of(name):
    src, window = cases()[name]
    return src if window is None else window8(src, *window)


TWO_IDAT = ("slice0671_w0_1600", "slice0671_w864_1264")
