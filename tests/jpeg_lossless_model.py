"""JPEG Lossless (ITU-T T.81 process 14, SOF3, Huffman) for one component of precision 2 .. 16, restated in Python: the
normative model of cct_jpegll_encode_batch / cct_jpegll_decode_batch.  The device encoder writes selection value 1 with no
point transform (DICOM transfer syntax 1.2.840.10008.1.2.4.70) and a Huffman table built per frame by Annex K.2; this
encoder also takes any predictor, a point transform, restart intervals, a caller's table and extra segments, so that the
decoder is exercised with what other writers produce.  Frames of precision 8 are checked against libjpeg-turbo through
Pillow (tests/test_jpeg_lossless_host.py); precisions 9 .. 16 rest on this model alone."""
import functools
import io
import struct

import numpy as np

ROWS = (1, 2, 3, 17)
COLS = (1, 2, 3, 63, 64, 65, 257)
SYMS = tuple(range(17)) + (256,)  # the categories and Annex K.2's reserved symbol


class JpegError(ValueError):
    """kind: 'JPEG' (CCT_E_JPEG), 'STREAM' (CCT_E_STREAM) or 'MIXED' (CCT_E_MIXED)"""

    def __init__(self, kind, why):
        super().__init__(f"{kind}: {why}")
        self.kind = kind


# ---- Huffman table (Annex K.2) -------------------------------------------------------------------------------------

def huffman_table(freq17):
    """category counts -> (BITS, a list of 16; HUFFVAL): Figures K.1 - K.4 with the reserved symbol 256 of frequency 1"""
    freq = {s: 0 for s in SYMS}
    for i in range(17):
        freq[i] = int(freq17[i])
    freq[256] = 1
    codesize = {s: 0 for s in SYMS}
    others = {s: -1 for s in SYMS}
    while True:
        c1, v = -1, 1 << 62
        for i in SYMS:  # ascending with <=: ties go to the larger symbol
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1 << 62
        for i in SYMS:
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for s in SYMS:
        if codesize[s]:
            bits[codesize[s]] += 1
    for i in range(32, 16, -1):  # Figure K.3
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1  # the reserved symbol leaves: no code of all ones
    huffval = [s for ln in range(1, 33) for s in range(17) if codesize[s] == ln]
    return bits[1:17], huffval


def codes_of(bits, huffval):
    """{symbol: (code, length)} of a BITS / HUFFVAL pair (Annex C)"""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[huffval[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def kraft_ok(bits):
    return sum(b << (16 - ln) for ln, b in enumerate(bits, 1)) <= 1 << 16


# ---- encoder ---------------------------------------------------------------------------------------------------------

def predictions(x, precision, predictor, pt, rpi):
    """x: (rows, cols) int64 samples after the point transform -> the prediction of every sample (H.1.2)"""
    rows, cols = x.shape
    ra = np.roll(x, 1, axis=1)
    rb = np.roll(x, 1, axis=0)
    rc = np.roll(rb, 1, axis=1)
    pred = {1: ra, 2: rb, 3: rc, 4: ra + rb - rc, 5: ra + ((rb - rc) >> 1), 6: rb + ((ra - rc) >> 1),
            7: (ra + rb) >> 1}[predictor].copy()
    first = np.arange(0, rows, rpi)
    pred[:, 0] = rb[:, 0]
    pred[first, :] = ra[first, :]
    pred[first, 0] = 1 << (precision - pt - 1)
    return pred


def categories(d):
    """differences modulo 2^16 -> (SSSS, extra bits)"""
    d = np.asarray(d, dtype=np.int64) & 0xFFFF
    sd = np.where(d > 0x8000, d - 0x10000, d)  # -32767 .. 32768
    a = np.abs(sd)
    cat = np.zeros(d.shape, dtype=np.int64)
    for k in range(17):
        cat += (a >> k) > 0
    extra = np.where(sd < 0, sd - 1, sd) & ((1 << cat) - 1)
    extra[cat == 16] = 0
    return cat, extra


def pack_bits(val, nb):
    """values of nb bits each, MSB first, padded with ones to a byte boundary"""
    val, nb = np.asarray(val, dtype=np.int64), np.asarray(nb, dtype=np.int64)
    total = int(nb.sum())
    starts = np.cumsum(nb) - nb
    idx = np.repeat(np.arange(len(nb)), nb)
    pos = np.arange(total) - starts[idx]
    b = ((val[idx] >> (nb[idx] - 1 - pos)) & 1).astype(np.uint8)
    b = np.concatenate([b, np.ones((-total) % 8, dtype=np.uint8)])
    return np.packbits(b).tobytes()


def segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def dht_payload(tables):
    """[(id, BITS, HUFFVAL)] -> the payload of one DHT segment"""
    return b"".join(bytes([tid]) + bytes(bits) + bytes(vals) for tid, bits, vals in tables)


def differences(img, precision, predictor=1, pt=0, restart_rows=0):
    x = np.asarray(img).astype(np.int64) >> pt
    rpi = restart_rows or x.shape[0]
    return ((x - predictions(x, precision, predictor, pt, rpi)) & 0xFFFF), rpi


def encode_frame(img, precision=None, predictor=1, pt=0, restart_rows=0, table=None, table_id=0, pre_segments=(),
                 dht_segments=None):
    """one interchange file.  table: (BITS, HUFFVAL) instead of the frame's own; dht_segments: DHT payloads written instead
    of the single table (the scan still names table_id); pre_segments: whole segments placed between SOI and SOF3."""
    img = np.asarray(img)
    rows, cols = img.shape
    if precision is None:
        precision = 8 * img.dtype.itemsize
    d, rpi = differences(img, precision, predictor, pt, restart_rows)
    cat, extra = categories(d)
    if table is None:
        table = huffman_table(np.bincount(cat.ravel(), minlength=17))
    bits, huffval = table
    co = codes_of(bits, huffval)
    code = np.zeros(17, dtype=np.int64)
    size = np.zeros(17, dtype=np.int64)
    for s, (c, ln) in co.items():
        code[s], size[s] = c, ln
    assert (size[np.unique(cat)] > 0).all(), "the table lacks a category of this image"
    nx = np.where(cat == 16, 0, cat)
    val = ((code[cat] << nx) | extra).reshape(rows, cols)
    nb = (size[cat] + nx).reshape(rows, cols)
    out = bytearray(b"\xff\xd8")
    for s in pre_segments:
        out += s
    out += segment(0xC3, struct.pack(">BHHBBBB", precision, rows, cols, 1, 1, 0x11, 0))
    if dht_segments is None:
        dht_segments = [dht_payload([(table_id, bits, huffval)])]
    for p in dht_segments:
        out += segment(0xC4, p)
    if restart_rows:
        ri = restart_rows * cols
        if ri > 65535:
            raise ValueError("restart interval above 65535 samples")
        out += segment(0xDD, struct.pack(">H", ri))
    out += segment(0xDA, bytes([1, 1, table_id << 4, predictor, 0, pt]))
    for k, r0 in enumerate(range(0, rows, rpi)):
        if k:
            out += bytes([0xFF, 0xD0 + (k - 1) % 8])
        out += pack_bits(val[r0:r0 + rpi].ravel(), nb[r0:r0 + rpi].ravel()).replace(b"\xff", b"\xff\x00")
    out += b"\xff\xd9"
    return bytes(out)


# ---- decoder ---------------------------------------------------------------------------------------------------------

def parse(f):
    """the marker walk of the host: {'P','Y','X','ri','ss','pt','table': (BITS, HUFFVAL),'s0','s1'} or JpegError('JPEG')"""
    f = bytes(f)
    if f[:2] != b"\xff\xd8":
        raise JpegError("JPEG", "no SOI")
    pos, sof, tables, ri = 2, None, {}, 0
    while True:
        if pos + 4 > len(f) or f[pos] != 0xFF:
            raise JpegError("JPEG", "no marker where one is due")
        m = f[pos + 1]
        if m in (0xD8, 0xD9, 0x01, 0xFF, 0x00) or 0xD0 <= m <= 0xD7:
            raise JpegError("JPEG", f"marker {m:02x} before the scan")
        ln = struct.unpack(">H", f[pos + 2:pos + 4])[0]
        if ln < 2 or pos + 2 + ln > len(f):
            raise JpegError("JPEG", "bad segment length")
        seg = f[pos + 4:pos + 2 + ln]
        pos += 2 + ln
        if m == 0xC3:
            if sof or len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise JpegError("JPEG", "SOF3 twice or of a bad length")
            p, y, x, nf = struct.unpack(">BHHB", seg[:6])
            if nf != 1 or y == 0 or x == 0 or not 2 <= p <= 16:
                raise JpegError("JPEG", "Nf, Y, X or P")
            sof = (p, y, x, seg[6])
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise JpegError("JPEG", "another SOF type")
        elif m == 0xC4:
            while seg:
                if len(seg) < 17 or len(seg) < 17 + sum(seg[1:17]):
                    raise JpegError("JPEG", "bad segment length")
                bits, cnt = list(seg[1:17]), sum(seg[1:17])
                vals = list(seg[17:17 + cnt])
                if seg[0] > 3 or cnt > 17 or any(v > 16 for v in vals) or not kraft_ok(bits):
                    raise JpegError("JPEG", "Huffman table")
                tables[seg[0]] = (bits, vals)
                seg = seg[17 + cnt:]
        elif m == 0xDD:
            if len(seg) != 2:
                raise JpegError("JPEG", "bad segment length")
            ri = struct.unpack(">H", seg)[0]
        elif m == 0xDC:
            raise JpegError("JPEG", "DNL")
        elif m == 0xDA:
            if not sof or len(seg) != 6 or seg[0] != 1 or seg[1] != sof[3]:
                raise JpegError("JPEG", "SOS")
            td, ss, se, ah, al = seg[2] >> 4, seg[3], seg[4], seg[5] >> 4, seg[5] & 15
            if not 1 <= ss <= 7 or se or ah or al >= sof[0] or td not in tables:
                raise JpegError("JPEG", "scan parameters")
            break
    if ri % sof[2]:
        raise JpegError("JPEG", "DRI that is not whole rows")
    i = pos
    while True:
        j = f.find(b"\xff", i)
        if j < 0 or j + 1 >= len(f):
            raise JpegError("JPEG", "no EOI")
        nx = f[j + 1]
        if nx == 0 or 0xD0 <= nx <= 0xD7:
            i = j + 2
        elif nx == 0xFF:
            i = j + 1
        elif nx == 0xD9:
            break
        else:
            raise JpegError("JPEG", "a marker other than EOI behind the scan")
    return {"P": sof[0], "Y": sof[1], "X": sof[2], "ri": ri, "ss": ss, "pt": al, "table": tables[td], "s0": pos, "s1": j}


def info(f):
    h = parse(f)
    return h["Y"], h["X"], h["P"]


def intervals_of(data, n_int):
    """entropy-coded bytes -> the unstuffed bytes of each interval; STREAM on a wrong, missing or spare RST"""
    out, cur, i = [], bytearray(), 0
    while i < len(data):
        b = data[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
        elif i + 1 < len(data) and data[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif i + 1 < len(data) and 0xD0 <= data[i + 1] <= 0xD7:
            if data[i + 1] - 0xD0 != len(out) % 8:
                raise JpegError("STREAM", "RST out of sequence")
            out.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            i += 1  # a fill byte
    out.append(bytes(cur))
    if len(out) != n_int:
        raise JpegError("STREAM", f"{len(out)} intervals where {n_int} are due")
    return out


def decode_frame(f, rows, cols, bits=16):
    f = bytes(f)
    h = parse(f)
    if (h["Y"], h["X"]) != (rows, cols) or h["P"] > bits:
        raise JpegError("MIXED", "shape or precision")
    rpi = h["ri"] // cols or rows
    n_int = -(-rows // rpi)
    lookup = {(ln, c): s for s, (c, ln) in codes_of(*h["table"]).items()}
    d = np.zeros(rows * cols, dtype=np.int64)
    for k, data in enumerate(intervals_of(f[h["s0"]:h["s1"]], n_int)):
        need = min(rpi, rows - k * rpi) * cols
        nbits, pos = 8 * len(data), 0

        def take(n):  # from the bytes that hold the n bits, so that a long interval costs no more per bit than a short one
            nonlocal pos
            if pos + n > nbits:
                raise JpegError("STREAM", "entropy data ends early")
            v = (int.from_bytes(data[pos >> 3:(pos + n + 7) >> 3], "big") >> (-(pos + n) & 7)) & ((1 << n) - 1)
            pos += n
            return v

        for q in range(need):
            code, ln = 0, 0
            while True:
                code, ln = code << 1 | take(1), ln + 1
                if (ln, code) in lookup:
                    break
                if ln == 16:
                    raise JpegError("STREAM", "a code that is not in the table")
            s = lookup[(ln, code)]
            if s == 16:
                v = 32768
            elif s == 0:
                v = 0
            else:
                v = take(s)
                if v < 1 << (s - 1):
                    v -= (1 << s) - 1
            d[k * rpi * cols + q] = v
        if (pos + 7) // 8 != len(data):
            raise JpegError("STREAM", "entropy data left over")
    d = d.reshape(rows, cols)
    x = np.zeros((rows, cols), dtype=np.int64)
    init, ss = 1 << (h["P"] - h["pt"] - 1), h["ss"]
    for r in range(rows):
        top = r % rpi == 0
        if ss == 1 or top:  # a row of Ra predictions: a running sum
            start = init if top else int(x[r - 1, 0])
            x[r] = (start + np.cumsum(d[r])) & 0xFFFF
            continue
        x[r, 0] = (x[r - 1, 0] + d[r, 0]) & 0xFFFF
        for c in range(1, cols):
            ra, rb, rc = int(x[r, c - 1]), int(x[r - 1, c]), int(x[r - 1, c - 1])
            p = (0, ra, rb, rc, ra + rb - rc, ra + ((rb - rc) >> 1), rb + ((ra - rc) >> 1), (ra + rb) >> 1)[ss]
            x[r, c] = (p + d[r, c]) & 0xFFFF
    return ((x << h["pt"]) & (0xFFFF if bits == 16 else 0xFF)).astype(np.uint16 if bits == 16 else np.uint8)


# ---- the second implementation ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pillow_opens_sof3():
    """False only if Pillow's libjpeg refuses a SOF3 file of this model (an OSError from open / load): the one reason for
    which a test may skip.  A file that opens to another raster is a failure, and so is an error of the model's encoder."""
    from PIL import Image
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    f = encode_frame(img, 8)
    try:
        im = Image.open(io.BytesIO(f))
        im.load()
    except OSError:
        return False
    assert np.array_equal(np.array(im), img), "Pillow opens the model's SOF3 file to another raster"
    return True


# ---- rasters of the tests ------------------------------------------------------------------------------------------

FIB = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584)


def fibonacci_raster():
    """1 x 6763 uint16 whose differences have category c FIB[c] times: unrestricted code lengths reach 17"""
    d = [32768]  # the first sample is predicted by 32768: category 16 once from sample 0 ...
    d += [0] * FIB[0]
    for c in range(1, 16):
        d += [1 << (c - 1)] * FIB[c]
    d += [32768] * (FIB[16] - 1)
    x = (32768 + np.cumsum(np.array(d, dtype=np.int64))) & 0xFFFF
    return x.astype(np.uint16).reshape(1, -1)


def raster_cases(rows, cols, precision, dtype):
    """name -> (rows, cols) raster of samples below 2^precision"""
    rng = np.random.default_rng(rows * 1000 + cols + precision)
    top = (1 << precision) - 1
    rr, cc = np.mgrid[0:rows, 0:cols]
    smooth = (top // 2 + (top // 8) * np.sin(rr / 3.0) * np.cos(cc / 5.0)).astype(np.int64)
    spikes = smooth.copy()
    spikes[rng.random((rows, cols)) < 0.05] = top
    spikes[rng.random((rows, cols)) < 0.05] = 0
    out = {
        "zeros": np.zeros((rows, cols), dtype=np.int64),
        "top": np.full((rows, cols), top, dtype=np.int64),
        "noise": rng.integers(0, top + 1, (rows, cols)),
        "ramp": (rr * cols + cc) % (top + 1),
        "alternating": np.where((rr * cols + cc) % 2 == 0, 0, top),
        "spikes": spikes,
    }
    return {k: v.astype(dtype) for k, v in out.items()}


# ---- damaged files ---------------------------------------------------------------------------------------------------

FLAT5 = ([0, 0, 0, 0, 17] + [0] * 11, list(range(17)))  # a flat 5-bit code: the words 10001 .. 11111 are not in the table


def stuff(data):
    return bytes(data).replace(b"\xff", b"\xff\x00")


def damaged_files(img, precision):
    """name -> (file, kind) for a raster of at least 4 rows and 2 columns: every refusal of the reader, by the kind of
    JpegError that decode_frame(file, rows, cols, 16) raises"""
    img = np.asarray(img)
    rows, cols = img.shape
    assert rows >= 4 and cols >= 2
    good = encode_frame(img, precision)
    h = parse(good)
    s0, s1 = h["s0"], h["s1"]
    sof_at = good.index(b"\xff\xc3")
    sos_at = good.index(b"\xff\xda", sof_at)
    dht_at = good.index(b"\xff\xc4")
    out = {}

    out["no_soi"] = (b"\x00\x00" + good[2:], "JPEG")
    out["no_sof"] = (good[:sof_at] + good[sof_at + 13:], "JPEG")
    out["no_eoi"] = (good[:-2], "JPEG")
    out["empty"] = (b"", "JPEG")
    for m in (0xC0, 0xC1, 0xC2, 0xC5, 0xC7, 0xCB, 0xCF):
        out[f"sof_{m:02x}"] = (good[:sof_at + 1] + bytes([m]) + good[sof_at + 2:], "JPEG")
    out["nf_3"] = (good[:sof_at + 2] + struct.pack(">HBHHB", 17, precision, rows, cols, 3) + bytes([1, 0x11, 0, 2, 0x11, 0, 3, 0x11, 0])
                   + good[sof_at + 13:], "JPEG")
    out["y_0"] = (good[:sof_at + 5] + b"\x00\x00" + good[sof_at + 7:], "JPEG")
    out["dnl_before_scan"] = (good[:sos_at] + segment(0xDC, struct.pack(">H", rows)) + good[sos_at:], "JPEG")
    out["dnl_after_scan"] = (good[:s1] + segment(0xDC, struct.pack(">H", rows)) + good[s1:], "JPEG")
    out["second_scan"] = (good[:s1] + good[sos_at:s1] + good[s1:], "JPEG")
    out["second_sof"] = (good[:sos_at] + good[sof_at:sof_at + 13] + good[sos_at:], "JPEG")
    b = bytearray(good)
    b[sos_at + 6] = 0x10  # the scan names table 1
    out["table_undefined"] = (bytes(b), "JPEG")
    b = bytearray(good)
    b[dht_at + 2:dht_at + 4] = struct.pack(">H", 60000)
    out["segment_past_the_file"] = (bytes(b), "JPEG")
    b = bytearray(good)
    b[dht_at + 2:dht_at + 4] = struct.pack(">H", 1)
    out["segment_length_1"] = (bytes(b), "JPEG")
    b = bytearray(good)
    b[dht_at + 3] -= 1  # the table's last symbol falls off the segment
    out["dht_cut"] = (bytes(b[:dht_at + 4 + (good[dht_at + 3] - 3)]) + good[dht_at + 4 + (good[dht_at + 3] - 2):], "JPEG")
    out["dri_not_rows"] = (good[:sos_at] + segment(0xDD, struct.pack(">H", cols + 1)) + good[sos_at:], "JPEG")
    for name, at, v in (("ss_0", 7, 0), ("ss_8", 7, 8), ("se_1", 8, 1), ("ah_1", 9, 0x10), ("pt_p", 9, precision), ("ns_2", 4, 2)):
        b = bytearray(good)
        b[sos_at + at] = v
        out[name] = (bytes(b), "JPEG")
    b = bytearray(good)
    b[dht_at + 4] = 0x10  # a table of class 1
    out["table_class_1"] = (bytes(b), "JPEG")
    over = ([2, 1] + [0] * 14, [0, 1, 2])  # 2 codes of 1 bit and one of 2: over-subscribed
    out["table_oversubscribed"] = (good[:dht_at] + segment(0xC4, dht_payload([(0, *over)])) + good[sos_at:], "JPEG")
    out["symbol_17"] = (good[:dht_at] + segment(0xC4, dht_payload([(0, [0, 1] + [0] * 14, [17])])) + good[sos_at:], "JPEG")
    out["wrong_shape"] = (encode_frame(img.reshape(cols, rows) if rows != cols else img[:-1], precision), "MIXED")
    # the entropy-coded data
    flat = encode_frame(img, precision, table=FLAT5)
    hf = parse(flat)
    assert flat[hf["s0"]] != 0xFF
    out["code_not_in_table"] = (flat[:hf["s0"]] + b"\xf8" + flat[hf["s0"] + 1:], "STREAM")
    data = intervals_of(good[s0:s1], 1)[0]
    if len(data) > 3:
        out["ends_early"] = (good[:s0] + stuff(data[:-3]) + good[s1:], "STREAM")
    out["left_over"] = (good[:s0] + stuff(data + b"\x00\x00") + good[s1:], "STREAM")
    out["no_data"] = (good[:s0] + good[s1:], "STREAM")
    out["spare_rst"] = (good[:s0] + stuff(data) + b"\xff\xd0" + good[s1:], "STREAM")
    rst = encode_frame(img, precision, restart_rows=1)
    hr = parse(rst)
    first = rst.index(b"\xff\xd0", hr["s0"])
    second = rst.index(b"\xff\xd1", first)
    out["rst_out_of_sequence"] = (rst[:first + 1] + b"\xd1" + rst[first + 2:], "STREAM")
    out["rst_missing"] = (rst[:second] + rst[second + 2:], "STREAM")
    return out
