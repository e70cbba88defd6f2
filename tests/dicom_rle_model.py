"""CPU model of DICOM RLE Lossless (PS3.5 Annex G) for one sample per pixel, 8 or 16 bits allocated: the normative
restatement of what the device codec (csrc/dicom_rle_kernels.hip) writes and reads.

Frame: sixteen little-endian uint32 (segment count, segment offsets from the frame start, zeros), then the segments.  A
16-bit frame has two: the most significant byte plane first.  A segment is its byte plane in raster order, PackBits-coded
row by row, padded with one 0x00 to an even length.

The encoder rule is the one of pydicom's pure-Python encoder (rle_handler._encode_row): maximal groups of equal bytes; a
group of one joins the pending literals; a longer group flushes them and becomes (129, v) per full 128 bytes plus
(257 - r, v) for a remainder r >= 2 or (0, v) for r = 1; literals leave in chunks of 128.  Nothing carries across rows.
The decoder follows the standard and assumes nothing about rows.
"""
import io
import struct

import numpy as np

ITEM_TAG = b"\xfe\xff\x00\xe0"
SEQ_DELIM = b"\xfe\xff\xdd\xe0\x00\x00\x00\x00"


def encode_row(src):
    """PackBits of one row of one byte plane."""
    src = bytes(src)
    out = bytearray()
    lit = bytearray()

    def flush():
        for k in range(0, len(lit), 128):
            chunk = lit[k:k + 128]
            out.append(len(chunk) - 1)
            out.extend(chunk)
        lit.clear()

    i, n = 0, len(src)
    while i < n:
        j = i
        while j < n and src[j] == src[i]:
            j += 1
        L, v = j - i, src[i]
        if L == 1:
            lit.append(v)
        else:
            flush()
            for _ in range(L // 128):
                out += bytes((129, v))
            r = L % 128
            if r >= 2:
                out += bytes((257 - r, v))
            elif r == 1:
                out += bytes((0, v))
        i = j
    flush()
    return bytes(out)


def planes_of(img):
    """Byte planes of a (rows, cols) uint8 / uint16 raster in segment order (most significant first)."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return [img]
    if img.dtype == np.uint16:
        return [(img >> 8).astype(np.uint8), (img & 0xFF).astype(np.uint8)]
    raise TypeError("uint8 or uint16 rasters")


def frame_of_segments(segments):
    """Header + segments, each padded to even length."""
    body = bytearray()
    offs = []
    for s in segments:
        offs.append(64 + len(body))
        body += s
        if len(s) & 1:
            body.append(0)
    head = [len(segments)] + offs + [0] * (15 - len(offs))
    return struct.pack("<16I", *head) + bytes(body)


def encode_frame(img):
    img = np.asarray(img)
    assert img.ndim == 2
    return frame_of_segments([b"".join(encode_row(row.tobytes()) for row in p) for p in planes_of(img)])


def decode_segment(seg, want):
    """`want` bytes of one segment; ValueError when it yields fewer."""
    out = bytearray()
    pos, n = 0, len(seg)
    while pos < n and len(out) < want:
        h = seg[pos]
        pos += 1
        if h < 128:
            out += seg[pos:pos + h + 1]  # a packet cut by the segment end gives what is there
            pos += h + 1
        elif h > 128:
            if pos < n:
                out += bytes((seg[pos],)) * (257 - h)
            pos += 1
    if len(out) < want:
        raise ValueError(f"segment yields {len(out)} of {want} bytes")
    return bytes(out[:want])


def decode_frame(frame, rows, cols, bits=16):
    frame = bytes(frame)
    nseg = bits // 8
    if len(frame) < 64:
        raise ValueError("frame shorter than its header")
    head = struct.unpack("<16I", frame[:64])
    if head[0] != nseg:
        raise ValueError(f"{head[0]} segments, expected {nseg}")
    offs = list(head[1:1 + nseg]) + [len(frame)]
    if offs[0] != 64 or any(b <= a for a, b in zip(offs[:-2], offs[1:-1])) or any(o > len(frame) for o in offs):
        raise ValueError("bad segment offsets")
    N = rows * cols
    planes = [np.frombuffer(decode_segment(frame[offs[k]:offs[k + 1]], N), np.uint8) for k in range(nseg)]
    if nseg == 1:
        return planes[0].reshape(rows, cols).copy()
    return ((planes[0].astype(np.uint16) << 8) | planes[1]).reshape(rows, cols)


def encapsulate(frames):
    """Encapsulated PixelData: Basic Offset Table, one fragment per frame (padded to even length), sequence delimiter."""
    items = bytearray()
    offsets = []
    for f in frames:
        f = bytes(f)
        if len(f) & 1:
            f += b"\x00"
        offsets.append(len(items))
        items += ITEM_TAG + struct.pack("<I", len(f)) + f
    bot = struct.pack(f"<{len(offsets)}I", *offsets)
    return ITEM_TAG + struct.pack("<I", len(bot)) + bot + bytes(items) + SEQ_DELIM


def fragments(pixel_data):
    """The frames of encapsulate(); ValueError on a malformed item structure."""
    d = bytes(pixel_data)
    pos, items = 0, []
    while True:
        if pos + 8 > len(d):
            raise ValueError("item structure ends without a sequence delimiter")
        tag, (ln,) = d[pos:pos + 4], struct.unpack("<I", d[pos + 4:pos + 8])
        pos += 8
        if tag == SEQ_DELIM[:4]:
            if ln != 0 or pos != len(d):
                raise ValueError("bad sequence delimiter")
            break
        if tag != ITEM_TAG:
            raise ValueError(f"unexpected tag {tag.hex()}")
        if pos + ln > len(d):
            raise ValueError("item runs past the data")
        items.append(d[pos:pos + ln])
        pos += ln
    if not items:
        raise ValueError("no Basic Offset Table item")
    bot, frames = items[0], items[1:]
    if len(bot) % 4 or (bot and len(bot) != 4 * len(frames)):
        raise ValueError("Basic Offset Table does not match the fragments")
    return frames


def have_libtiff():
    try:
        from PIL import features
        return bool(features.check("libtiff"))
    except Exception:
        return False


def libtiff_frame(img):
    """A foreign frame: each byte plane PackBits-coded by libtiff (Pillow's TIFF writer), strips concatenated.  libtiff codes
    rows separately too, but merges 2-byte runs into literals: valid packets the model's encoder never writes."""
    from PIL import Image
    segs = []
    for p in planes_of(img):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(p)).save(buf, "TIFF", compression="packbits")
        data = buf.getvalue()
        tags = Image.open(io.BytesIO(data)).tag_v2
        offs, cnts = tags[273], tags[279]
        segs.append(b"".join(data[o:o + c] for o, c in zip(offs, cnts)))
    return frame_of_segments(segs)


# ---- rasters that exercise the encoder rule -------------------------------------------------------------------------

ROWS = (1, 2, 3)
COLS = (1, 2, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 258, 300)


def plane_cases(rows, cols, seed=0):
    """{name: (rows, cols) uint8 plane}: constant, alternating, period-3 aab, runs of exactly 128 / 129 / 256 / 257 at
    column 0, in the middle and ending at the last column, literal stretches of 128 / 129 / 257 between runs, rows that end
    and start on the same byte, small-alphabet noise."""
    rng = np.random.default_rng(1000 * rows + cols + seed)
    alt = (10 + (np.arange(cols) & 1)).astype(np.uint8)  # no two neighbours equal
    c = {"constant": np.full((rows, cols), 7, np.uint8),
         "alternating": (1 + 5 * (np.arange(rows * cols) & 1)).astype(np.uint8).reshape(rows, cols),
         "aab": np.tile(np.resize(np.array([3, 3, 9], np.uint8), cols), (rows, 1))}
    for L in (128, 129, 256, 257):
        if cols >= L:
            for where, s in (("start", 0), ("middle", (cols - L) // 2), ("end", cols - L)):
                row = alt.copy()
                row[s:s + L] = 200
                c[f"run{L}_{where}"] = np.tile(row, (rows, 1))
    for K in (128, 129, 257):
        if cols >= K + 4:
            row = np.full(cols, 70, np.uint8)
            row[0:2] = 50
            row[2:2 + K] = alt[:K]
            row[2 + K:4 + K] = 60
            c[f"literals{K}"] = np.tile(row, (rows, 1))
    seam = np.tile(alt, (rows, 1))
    seam[:, :2] = 5
    seam[:, -2:] = 5
    c["row_seam"] = seam
    for k in range(2):
        c[f"random3_{k}"] = rng.integers(0, 3, (rows, cols)).astype(np.uint8)
    return c


def raster_cases(rows, cols, bits):
    """The planes above as rasters: 8-bit as they are; 16-bit with the plane as the low byte under the next case's plane as
    the high byte, plus a constant high plane under a noisy low plane."""
    planes = plane_cases(rows, cols)
    if bits == 8:
        return planes
    names = list(planes)
    out = {n: (planes[names[(i + 1) % len(names)]].astype(np.uint16) << 8) | planes[n] for i, n in enumerate(names)}
    rng = np.random.default_rng(7 * rows + cols)
    out["const_hi_noisy_lo"] = (0x1200 | rng.integers(0, 256, (rows, cols))).astype(np.uint16)
    return out
