"""JPEG-LS lossless (ITU-T T.87, DICOM transfer syntax 1.2.840.10008.1.2.4.80) for one component of precision 2 .. 16,
restated in Python: the normative model of cct_jpegls_encode_batch / cct_jpegls_decode_batch.  The device writer emits
NEAR = 0, ILV = 0, the default preset parameters and no LSE segment; this encoder also takes preset parameters of the
caller's (and then writes the LSE segment that states them), so that the reader is exercised with what other writers produce.
The one outside anchor is the worked example of T.87 Annex H.3 (H3_RASTER / H3_FILE); everything else rests on this model
alone, written from the standard's rules and independently of the kernels."""
import bisect
import functools
import struct

import numpy as np

ROWS = (1, 2, 5, 17)
COLS = (1, 2, 63, 64, 65, 130)
PRECISIONS = (2, 8, 12, 16)
RESTARTS = (0, 1, 2)
J = (0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 9, 10, 11, 12, 13, 14, 15)
MIN_C, MAX_C = -128, 127
CENSUS = ("escape_regular", "escape_interruption", "reset_regular", "reset_interruption", "k0_map", "run_eol", "run_len0",
          "runindex_ge16", "stuffed_bit", "interval_ends_ff", "code64")

H3_RASTER = np.array([[0, 0, 90, 74], [68, 50, 43, 205], [64, 145, 145, 145], [100, 145, 145, 145]], dtype=np.uint8)
H3_FILE = bytes.fromhex("ffd8" "fff7000b080004000401011100" "ffda0008010100000000"
                        "c000006c80208e01c00000574000006ee6000001bc18000005d800009160" "ffd9")


class JlsError(ValueError):
    """kind: 'JPEGLS' (CCT_E_JPEGLS), 'STREAM' (CCT_E_STREAM) or 'MIXED' (CCT_E_MIXED)"""

    def __init__(self, kind, why):
        super().__init__(f"{kind}: {why}")
        self.kind = kind


# ---- parameters --------------------------------------------------------------------------------------------------------

def _clamp(i, lo, hi):
    return lo if (i > hi or i < lo) else i  # T.87 C.2.4.1.1: not a saturation


def default_thresholds(maxval):
    if maxval >= 128:
        f = (min(maxval, 4095) + 128) >> 8
        t1 = _clamp(f + 2, 1, maxval)
        t2 = _clamp(4 * f + 3, t1, maxval)
        t3 = _clamp(17 * f + 4, t2, maxval)
    else:
        f = 256 // (maxval + 1)
        t1 = _clamp(max(2, 3 // f), 1, maxval)
        t2 = _clamp(max(3, 7 // f), t1, maxval)
        t3 = _clamp(max(4, 21 // f), t2, maxval)
    return t1, t2, t3


class Params:
    """the coding parameters of a scan: the defaults of a precision, or what an LSE segment of id 1 states (0: the default)"""

    def __init__(self, precision, maxval=0, t1=0, t2=0, t3=0, reset=0):
        self.maxval = maxval or (1 << precision) - 1
        d = default_thresholds(self.maxval)
        self.t1, self.t2, self.t3 = t1 or d[0], t2 or d[1], t3 or d[2]
        self.reset = reset or 64
        self.range = self.maxval + 1
        self.qbpp = (self.range - 1).bit_length()
        self.bpp = max(2, self.maxval.bit_length())
        self.limit = 2 * (self.bpp + max(8, self.bpp))
        self.a0 = max(2, (self.range + 32) >> 6)

    def legal(self, precision):
        return (1 <= self.maxval <= (1 << precision) - 1 and 1 <= self.t1 <= self.t2 <= self.t3 <= self.maxval
                and 3 <= self.reset <= max(255, self.maxval))


def _quantise(d, p):
    if d <= -p.t3:
        return -4
    if d <= -p.t2:
        return -3
    if d <= -p.t1:
        return -2
    if d < 0:
        return -1
    if d == 0:
        return 0
    if d < p.t1:
        return 1
    if d < p.t2:
        return 2
    if d < p.t3:
        return 3
    return 4


def _context(ra, rb, rc, rd, p):
    """-> (q in 1 .. 364, sign), or (0, 1) for run mode"""
    q1, q2, q3 = _quantise(rd - rb, p), _quantise(rb - rc, p), _quantise(rc - ra, p)
    q = 81 * q1 + 9 * q2 + q3
    return (-q, -1) if q < 0 else (q, 1)


def _median(ra, rb, rc):
    if rc >= max(ra, rb):
        return min(ra, rb)
    if rc <= min(ra, rb):
        return max(ra, rb)
    return ra + rb - rc


def _reduce(e, p):
    e %= p.range
    return e - p.range if e >= (p.range + 1) // 2 else e


def _golomb_k(n, a):
    k = 0
    while (n << k) < a:
        k += 1
    return k


class _State:
    def __init__(self, p):
        self.A = [p.a0] * 367
        self.N = [1] * 367
        self.B = [0] * 365
        self.C = [0] * 365
        self.Nn = [0, 0]
        self.runindex = 0

    def update_regular(self, q, e, p, cnt):
        self.B[q] += e
        self.A[q] += abs(e)
        if self.N[q] == p.reset:
            self.A[q] >>= 1
            self.N[q] >>= 1
            b = self.B[q]
            self.B[q] = b >> 1 if b >= 0 else -((1 - b) >> 1)
            cnt["reset_regular"] += 1
        self.N[q] += 1
        n = self.N[q]
        if self.B[q] <= -n:
            self.B[q] += n
            if self.C[q] > MIN_C:
                self.C[q] -= 1
            if self.B[q] <= -n:
                self.B[q] = -n + 1
        elif self.B[q] > 0:
            self.B[q] -= n
            if self.C[q] < MAX_C:
                self.C[q] += 1
            if self.B[q] > 0:
                self.B[q] = 0

    def update_interruption(self, ritype, e, em, p, cnt):
        q = 365 + ritype
        if e < 0:
            self.Nn[ritype] += 1
        self.A[q] += (em + 1 - ritype) >> 1
        if self.N[q] == p.reset:
            self.A[q] >>= 1
            self.N[q] >>= 1
            self.Nn[ritype] >>= 1
            cnt["reset_interruption"] += 1
        self.N[q] += 1
        if self.runindex > 0:
            self.runindex -= 1


# ---- encoder ---------------------------------------------------------------------------------------------------------

def _golomb(out, m, k, limit, qbpp):
    """-> True for the escape code"""
    hi = m >> k
    if hi < limit - qbpp - 1:
        out.append("0" * hi + "1" + (format(m & ((1 << k) - 1), f"0{k}b") if k else ""))
        return False
    out.append("0" * (limit - qbpp - 1) + "1" + format(m - 1, f"0{qbpp}b"))
    return True


def _stuffed(bits, cnt):
    """a string of bits -> the interval's bytes: 7 bits behind a 0xFF, zero padding, 0x00 behind a last 0xFF"""
    out, at = bytearray(), 0
    while at < len(bits):
        w = 7 if out and out[-1] == 0xFF else 8
        cnt["stuffed_bit"] += w == 7
        out.append(int(bits[at:at + w].ljust(w, "0"), 2))
        at += w
    if out and out[-1] == 0xFF:
        out.append(0)
        cnt["interval_ends_ff"] += 1
    return bytes(out)


def _encode_interval(lines, p, cnt):
    cols = len(lines[0])
    st = _State(p)
    out = []
    above = [0] * (cols + 2)  # [0]: Rc of column 0; [1 .. cols]: the line above; [cols + 1]: Rd of the last column
    for line in lines:
        cur = [above[1]] + [int(v) for v in line]  # [0]: Ra of column 0
        above[cols + 1] = above[cols]
        i = 1
        while i <= cols:
            ra, rb, rc, rd = cur[i - 1], above[i], above[i - 1], above[i + 1]
            q, sign = _context(ra, rb, rc, rd, p)
            if q:
                px = min(max(_median(ra, rb, rc) + sign * st.C[q], 0), p.maxval)
                e = _reduce((cur[i] - px) * sign, p)
                k = _golomb_k(st.N[q], st.A[q])
                if k == 0 and 2 * st.B[q] <= -st.N[q]:
                    m = 2 * e + 1 if e >= 0 else -2 * (e + 1)
                    cnt["k0_map"] += 1
                else:
                    m = 2 * e if e >= 0 else -2 * e - 1
                n0 = len(out)
                cnt["escape_regular"] += _golomb(out, m, k, p.limit, p.qbpp)
                cnt["code64"] += len(out[n0]) == 64
                st.update_regular(q, e, p, cnt)
                i += 1
                continue
            count = 0
            while i + count <= cols and cur[i + count] == ra:
                count += 1
            i += count
            cnt["run_len0"] += count == 0
            while count >= 1 << J[st.runindex]:
                out.append("1")
                count -= 1 << J[st.runindex]
                if st.runindex < 31:
                    st.runindex += 1
            cnt["runindex_ge16"] += st.runindex >= 16
            if i > cols:
                cnt["run_eol"] += 1
                if count:
                    out.append("1")
                break
            jr = J[st.runindex]
            out.append("0" + (format(count, f"0{jr}b") if jr else ""))
            rb = above[i]
            ritype = int(ra == rb)
            e = cur[i] - (ra if ritype else rb)
            if not ritype and ra > rb:
                e = -e
            e = _reduce(e, p)
            temp = st.A[366] + (st.N[366] >> 1) if ritype else st.A[365]
            n, nn = st.N[365 + ritype], st.Nn[ritype]
            k = _golomb_k(n, temp)
            mp = int((k == 0 and e > 0 and 2 * nn < n) or (e < 0 and 2 * nn >= n) or (e < 0 and k != 0))
            em = 2 * abs(e) - ritype - mp
            n0 = len(out)
            cnt["escape_interruption"] += _golomb(out, em, k, p.limit - jr - 1, p.qbpp)
            cnt["code64"] += len(out[n0]) == 64
            st.update_interruption(ritype, e, em, p, cnt)
            i += 1
        above = [above[1]] + cur[1:] + [0]
    return _stuffed("".join(out), cnt)


def new_census():
    return {k: 0 for k in CENSUS}


def encode_frame(img, precision, restart_rows=0, lse=None, census=None):
    """one raster (rows, cols) of samples below 2^precision (below MAXVAL + 1 with lse) -> the file.  lse: a dict of
    maxval / t1 / t2 / t3 / reset (0 or absent: the default), written as an LSE segment of id 1.  census: a dict of
    new_census() that counts what the coder went through."""
    img = np.asarray(img)
    rows, cols = img.shape
    p = Params(precision, **(lse or {}))
    assert p.legal(precision) and int(img.max()) <= p.maxval
    cnt = census if census is not None else new_census()
    f = b"\xff\xd8\xff\xf7" + struct.pack(">HBHHBBBB", 11, precision, rows, cols, 1, 1, 0x11, 0)
    if lse is not None:
        f += b"\xff\xf8" + struct.pack(">HBHHHHH", 13, 1, *(lse.get(k, 0) for k in ("maxval", "t1", "t2", "t3", "reset")))
    if restart_rows > 0:
        f += b"\xff\xdd" + struct.pack(">HH", 4, restart_rows)
    f += b"\xff\xda" + struct.pack(">HBBBBBB", 8, 1, 1, 0, 0, 0, 0)
    rpi = restart_rows if restart_rows > 0 else rows
    lines = img.tolist()
    for k, r0 in enumerate(range(0, rows, rpi)):
        if k:
            f += bytes([0xFF, 0xD0 + (k - 1) % 8])
        f += _encode_interval(lines[r0:r0 + rpi], p, cnt)
    return f + b"\xff\xd9"


# ---- parser ------------------------------------------------------------------------------------------------------------

def parse(f):
    """the marker walk -> dict(P, Y, X, ri (lines, 0: none), params, intervals [(start, end)], rst [m ...]); JlsError 'JPEGLS'"""
    f = bytes(f)

    def bad(why):
        return JlsError("JPEGLS", why)

    if len(f) < 4 or f[:2] != b"\xff\xd8":
        raise bad("no SOI")
    pos, sof, lse, ri, comp = 2, None, None, 0, 0
    while True:
        if pos + 4 > len(f) or f[pos] != 0xFF:
            raise bad("no marker where one is due")
        m = f[pos + 1]
        if m in (0xD8, 0xD9, 0x01, 0xFF, 0x00) or 0xD0 <= m <= 0xD7:
            raise bad(f"marker {m:02x} among the headers")
        ln = int.from_bytes(f[pos + 2:pos + 4], "big")
        if ln < 2 or pos + 2 + ln > len(f):
            raise bad("segment length")
        seg = f[pos + 4:pos + 2 + ln]
        pos += 2 + ln
        if m == 0xF7:
            if sof or len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise bad("SOF55")
            P, Y, X = seg[0], int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
            if seg[5] != 1 or Y == 0 or X == 0 or not 2 <= P <= 16:
                raise bad("SOF55: one component, precision 2 .. 16")
            sof, comp = (P, Y, X), seg[6]
        elif (0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC)) or m == 0xF9:
            raise bad("another SOF")
        elif m == 0xF8:
            if len(seg) != 11 or seg[0] != 1:
                raise bad("LSE: only id 1")
            lse = struct.unpack(">HHHHH", seg[1:])
        elif m == 0xDD:
            if len(seg) not in (2, 3, 4):
                raise bad("DRI length")
            ri = int.from_bytes(seg, "big")
        elif m == 0xDC:
            raise bad("DNL")
        elif m == 0xDA:
            if not sof or len(seg) != 6 or seg[0] != 1 or seg[1] != comp or seg[2] != 0 or seg[3] != 0 or seg[4] != 0 or seg[5] != 0:
                raise bad("SOS: one component, no mapping table, NEAR 0, ILV 0, no point transform")
            break
    P, Y, X = sof
    p = Params(P, *(lse or ()))
    if not p.legal(P):
        raise bad("LSE parameters")
    intervals, rst, start, i = [], [], pos, pos
    while True:
        j = f.find(b"\xff", i)
        if j < 0 or j + 1 >= len(f):
            raise bad("no EOI")
        nx = f[j + 1]
        if nx < 0x80:
            i = j + 2
        elif 0xD0 <= nx <= 0xD7:
            intervals.append((start, j))
            rst.append(nx - 0xD0)
            start = i = j + 2
        elif nx == 0xD9:
            intervals.append((start, j))
            break
        else:
            raise bad(f"marker {nx:02x} in the scan")
    return dict(P=P, Y=Y, X=X, ri=ri, params=p, intervals=intervals, rst=rst)


# ---- decoder -----------------------------------------------------------------------------------------------------------

class _Reader:
    def __init__(self, data):
        self.data = data
        parts, ends, n = [], [], 0
        for i, b in enumerate(data):
            w = 7 if i and data[i - 1] == 0xFF else 8
            parts.append(format(b & ((1 << w) - 1), f"0{w}b"))
            n += w
            ends.append(n)
        self.bits, self.ends, self.at = "".join(parts), ends, 0

    def early(self):
        return JlsError("STREAM", "the interval's data ends early")

    def bit(self):
        if self.at >= len(self.bits):
            raise self.early()
        self.at += 1
        return self.bits[self.at - 1] == "1"

    def value(self, n):
        if n == 0:
            return 0
        if self.at + n > len(self.bits):
            raise self.early()
        self.at += n
        return int(self.bits[self.at - n:self.at], 2)

    def zeros(self, most):
        """zeros up to the next one, which is consumed; stops at `most` zeros, the one behind them not consumed"""
        j = self.bits.find("1", self.at, self.at + most)
        if j < 0:
            if self.at + most > len(self.bits):
                raise self.early()
            self.at += most
            return most
        n = j - self.at
        self.at = j + 1
        return n

    def finish(self):
        touched = bisect.bisect_left(self.ends, self.at) + 1 if self.at else 0  # bytes of which a bit was read
        if touched and self.data[touched - 1] == 0xFF:
            touched += 1
        if touched != len(self.data):
            raise JlsError("STREAM", "whole bytes left over" if touched < len(self.data) else "no byte behind a last 0xFF")


def _read_golomb(rd, k, limit, qbpp):
    hi = rd.zeros(limit - qbpp - 1)
    if hi < limit - qbpp - 1:
        m = (hi << k) | rd.value(k)
        if m > 1 << qbpp:  # no coder writes one (the escape code carries M - 1 in qbpp bits), and the state stays in 32 bits
            raise JlsError("STREAM", "a value above 2^qbpp")
        return m
    if not rd.bit():
        raise JlsError("STREAM", "a code longer than LIMIT")
    return rd.value(qbpp) + 1


def _fix(rx, p):
    if rx < 0:
        rx += p.range
    elif rx > p.maxval:
        rx -= p.range
    return min(max(rx, 0), p.maxval)


def _decode_interval(data, nlines, cols, p):
    rd = _Reader(data)
    st = _State(p)
    cnt = new_census()
    lines = []
    above = [0] * (cols + 2)
    for _ in range(nlines):
        cur = [above[1]] + [0] * cols
        above[cols + 1] = above[cols]
        i = 1
        while i <= cols:
            ra, rb, rc, rd_ = cur[i - 1], above[i], above[i - 1], above[i + 1]
            q, sign = _context(ra, rb, rc, rd_, p)
            if q:
                px = min(max(_median(ra, rb, rc) + sign * st.C[q], 0), p.maxval)
                k = _golomb_k(st.N[q], st.A[q])
                m = _read_golomb(rd, k, p.limit, p.qbpp)
                if k == 0 and 2 * st.B[q] <= -st.N[q]:
                    e = (m - 1) >> 1 if m & 1 else -(m >> 1) - 1
                else:
                    e = m >> 1 if not m & 1 else -((m + 1) >> 1)
                st.update_regular(q, e, p, cnt)
                cur[i] = _fix(px + sign * e, p)
                i += 1
                continue
            while True:
                if not rd.bit():
                    break
                n = min(1 << J[st.runindex], cols + 1 - i)
                cur[i:i + n] = [ra] * n
                i += n
                if n == 1 << J[st.runindex] and st.runindex < 31:
                    st.runindex += 1
                if i > cols:
                    break
            if i > cols:
                break
            jr = J[st.runindex]
            n = rd.value(jr)
            if i + n > cols:
                raise JlsError("STREAM", "a run passes the end of the line")
            cur[i:i + n] = [ra] * n
            i += n
            rb = above[i]
            ritype = int(ra == rb)
            temp = st.A[366] + (st.N[366] >> 1) if ritype else st.A[365]
            nq, nn = st.N[365 + ritype], st.Nn[ritype]
            k = _golomb_k(nq, temp)
            em = _read_golomb(rd, k, p.limit - jr - 1, p.qbpp)
            t = em + ritype
            e = (t + 1) >> 1
            if e and (t & 1) == int(k != 0 or 2 * nn >= nq):
                e = -e
            st.update_interruption(ritype, e, em, p, cnt)
            if not ritype and ra > rb:
                e = -e
            cur[i] = _fix((ra if ritype else rb) + e, p)
            i += 1
        lines.append(cur[1:])
        above = [above[1]] + cur[1:] + [0]
    rd.finish()
    return lines


def decode_frame(f, rows, cols, bits=16):
    """file -> (rows, cols) raster of uint8 (bits 8) or uint16; JlsError of kind JPEGLS, MIXED or STREAM"""
    h = parse(f)
    if (h["Y"], h["X"]) != (rows, cols) or h["P"] > bits:
        raise JlsError("MIXED", "the frame's shape or precision is not the call's")
    rpi = h["ri"] if 0 < h["ri"] < rows else rows
    n_int = -(-rows // rpi)
    if len(h["intervals"]) != n_int or h["rst"] != [k % 8 for k in range(n_int - 1)]:
        raise JlsError("STREAM", "RST markers: wrong count or sequence")
    out = []
    for k, (a, b) in enumerate(h["intervals"]):
        out += _decode_interval(f[a:b], min(rpi, rows - k * rpi), cols, h["params"])
    return np.array(out, dtype=np.uint8 if bits == 8 else np.uint16).reshape(rows, cols)


def info(f):
    h = parse(f)
    return h["Y"], h["X"], h["P"]


# ---- rasters -----------------------------------------------------------------------------------------------------------

def dtype_of(precision):
    return np.uint8 if precision <= 8 else np.uint16


def raster_cases(rows, cols, precision, dtype=None):
    """name -> (rows, cols) raster of samples below 2^precision"""
    rng = np.random.default_rng(rows * 1000 + cols + precision)
    top = (1 << precision) - 1
    rr, cc = np.mgrid[0:rows, 0:cols]
    smooth = (top // 2 + (top // 8) * np.sin(rr / 3.0) * np.cos(cc / 5.0)).astype(np.int64)
    spikes = smooth.copy()
    spikes[rng.random((rows, cols)) < 0.05] = top
    spikes[rng.random((rows, cols)) < 0.05] = 0
    flats = np.where(rng.random((rows, cols)) < 0.1, rng.integers(0, top + 1, (rows, cols)), top // 3)
    out = {
        "zeros": np.zeros((rows, cols), dtype=np.int64),
        "top": np.full((rows, cols), top, dtype=np.int64),
        "noise": rng.integers(0, top + 1, (rows, cols)),
        "ramp": (rr * cols + cc) % (top + 1),
        "alternating": np.where((rr * cols + cc) % 2 == 0, 0, top),
        "spikes": spikes,
        "flats": flats,
    }
    return {k: v.astype(dtype or dtype_of(precision)) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def census_cases():
    """name -> (raster, precision): rasters that take the coder where raster_cases does not go"""
    rng = np.random.default_rng(87)
    rr, cc = np.mgrid[0:8, 0:64]
    stripes = np.zeros((12, 70), dtype=np.uint16)
    stripes[:, ::7] = 4095
    return {
        "noise16": (rng.integers(0, 65536, (8, 64)).astype(np.uint16), 16),
        "noise12": (rng.integers(0, 4096, (16, 64)).astype(np.uint16), 12),
        "zeros_wide": (np.zeros((4, 600), dtype=np.uint16), 12),
        "stripes": (stripes, 12),
        "ramp8": ((40 * cc + 3 * rr).astype(np.uint8), 8),
        "noise1_p2": (rng.integers(0, 2, (1, 65)).astype(np.uint8), 2),
        "noise1_p2_tall": (rng.integers(0, 2, (20, 65)).astype(np.uint8), 2),
    }
