"""Plain-Python model of the device JPEG 2000 Part-1 lossless encoder (csrc/jpeg2000_kernels.hip), written from T.800.

The file is fixed so that the output is deterministic: SOC, SIZ, COD, QCD, one SOT, SOD, the packets, EOC; one component,
one tile, one layer, LRCP, maximal precincts, the reversible 5/3 transform, square code-blocks of 32 or 64, code-block
style 0 (one codeword segment per code-block, every coding pass included), no quantization, 2 guard bits.  The device is
held to encode() byte for byte; tests/test_jpeg2000_model.py holds encode() to OpenJPEG through Pillow.

    encode(image, precision, shift, levels, codeblock, jp2) -> bytes
    info(file) -> (rows, cols, precision), ValueError for anything else
    raster_cases(rows, cols, precision, dtype) -> {name: raster}
    matrix(precision), phantoms() -> the rasters of the tests with their files, computed once

Pure-Python MQ coding is slow: keep inputs at or below 130 x 70 and 128 x 128.
"""
import functools
import struct

import numpy as np

# T.800 Table C.2: Qe, NMPS, NLPS, SWITCH
MQ_TABLE = (
    (0x5601, 1, 1, 1), (0x3401, 2, 6, 0), (0x1801, 3, 9, 0), (0x0AC1, 4, 12, 0), (0x0521, 5, 29, 0), (0x0221, 38, 33, 0),
    (0x5601, 7, 6, 1), (0x5401, 8, 14, 0), (0x4801, 9, 14, 0), (0x3801, 10, 14, 0), (0x3001, 11, 17, 0), (0x2401, 12, 18, 0),
    (0x1C01, 13, 20, 0), (0x1601, 29, 21, 0), (0x5601, 15, 14, 1), (0x5401, 16, 14, 0), (0x5101, 17, 15, 0), (0x4801, 18, 16, 0),
    (0x3801, 19, 17, 0), (0x3401, 20, 18, 0), (0x3001, 21, 19, 0), (0x2801, 22, 19, 0), (0x2401, 23, 20, 0), (0x2201, 24, 21, 0),
    (0x1C01, 25, 22, 0), (0x1801, 26, 23, 0), (0x1601, 27, 24, 0), (0x1401, 28, 25, 0), (0x1201, 29, 26, 0), (0x1101, 30, 27, 0),
    (0x0AC1, 31, 28, 0), (0x09C1, 32, 29, 0), (0x08A1, 33, 30, 0), (0x0521, 34, 31, 0), (0x0441, 35, 32, 0), (0x02A1, 36, 33, 0),
    (0x0221, 37, 34, 0), (0x0141, 38, 35, 0), (0x0111, 39, 36, 0), (0x0085, 40, 37, 0), (0x0049, 41, 38, 0), (0x0025, 42, 39, 0),
    (0x0015, 43, 40, 0), (0x0009, 44, 41, 0), (0x0005, 45, 42, 0), (0x0001, 45, 43, 0), (0x5601, 46, 46, 0),
)
CTX_SIGN, CTX_MAG, CTX_RL, CTX_UNI, N_CTX = 9, 14, 17, 18, 19
LL, HL, LH, HH = 0, 1, 2, 3
GAIN = (0, 1, 1, 2)
GUARD_BITS = 2
F_SIG, F_NEG, F_VISIT, F_REFINED = 1, 2, 4, 8
# The eight neighbours in the bit order of a traced neighbour pattern: bit k is the neighbour at NEIGHBOURS[k] = (dy, dx).
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def count(trace, key, item, n=1):
    """trace[key][item] += n: every traced event is a counter, so traces of several blocks or files add up (merge())."""
    d = trace.setdefault(key, {})
    d[item] = d.get(item, 0) + n


def merge(traces):
    out = {}
    for t in traces:
        for key, d in t.items():
            for item, n in d.items():
                count(out, key, item, n)
    return out


class MQEncoder:
    """T.800 Annex C.2.  The byte "before the first" (BP = BPST - 1) is imaginary and never written."""

    def __init__(self, trace=None):
        """trace: "mq_state" {state}, "mq_ctx" {(context, "mps" / "lps")}, "byteout" {"stuff" a byte behind 0xFF, "carry_ff" a carry
        that makes 0xFF, "carry", "plain"}, "flush" {(C lowered by 0x8000, a final 0xFF dropped)}, "seg_tail" {"ff7f": the coded bytes
        end in 0xFF 0x7F when the flush begins}.  The bytes do not depend on it."""
        self.trace = trace
        if trace is not None:
            self.n_state, self.n_ctx = trace.setdefault("mq_state", {}), trace.setdefault("mq_ctx", {})
        self.a, self.c, self.ct, self.b, self.pos = 0x8000, 0, 12, 0, -1
        self.out = bytearray()
        self.state = [0] * N_CTX
        self.mps = [0] * N_CTX
        self.state[0], self.state[CTX_RL], self.state[CTX_UNI] = 4, 3, 46

    def _next(self, byte):  # BP = BP + 1; B = byte
        if self.pos >= 0:
            self.out.append(self.b)
        self.pos += 1
        self.b = byte

    def _byteout(self):
        tr = self.trace
        if self.b == 0xFF:
            if tr is not None:
                count(tr, "byteout", "stuff")
            self._next(self.c >> 20); self.c &= 0xFFFFF; self.ct = 7
            return
        if self.c >= 0x8000000:
            self.b += 1
            if self.b == 0xFF:
                if tr is not None:
                    count(tr, "byteout", "carry_ff")
                self.c &= 0x7FFFFFF
                self._next(self.c >> 20); self.c &= 0xFFFFF; self.ct = 7
                return
            if tr is not None:
                count(tr, "byteout", "carry")
        elif tr is not None:
            count(tr, "byteout", "plain")
        self._next((self.c >> 19) & 0xFF); self.c &= 0x7FFFF; self.ct = 8

    def _renorm(self):
        while True:
            self.a <<= 1; self.c <<= 1; self.ct -= 1
            if self.ct == 0:
                self._byteout()
            if self.a & 0x8000:
                return

    def encode(self, cx, d):
        qe, nmps, nlps, sw = MQ_TABLE[self.state[cx]]
        if self.trace is not None:
            st, key = self.state[cx], (cx, "mps" if d == self.mps[cx] else "lps")
            self.n_state[st] = self.n_state.get(st, 0) + 1
            self.n_ctx[key] = self.n_ctx.get(key, 0) + 1
        self.a -= qe
        if d == self.mps[cx]:
            if self.a & 0x8000:
                self.c += qe
                return
            if self.a < qe:
                self.a = qe
            else:
                self.c += qe
            self.state[cx] = nmps
        else:
            if self.a < qe:
                self.c += qe
            else:
                self.a = qe
            if sw:
                self.mps[cx] ^= 1
            self.state[cx] = nlps
        self._renorm()

    def flush(self):
        """C.2.9; a final 0xFF is not part of the segment."""
        tr, self.trace = self.trace, None  # the two BYTEOUTs of the flush are not counted with those of the coding
        if tr is not None and self.out and self.out[-1] == 0xFF and self.b == 0x7F:
            count(tr, "seg_tail", "ff7f")
        t = self.c + self.a
        self.c |= 0xFFFF
        lowered = self.c >= t
        if lowered:
            self.c -= 0x8000
        self.c <<= self.ct; self._byteout()
        self.c <<= self.ct; self._byteout()
        if self.b != 0xFF and self.pos >= 0:
            self.out.append(self.b)
        if tr is not None:
            count(tr, "flush", (lowered, self.b == 0xFF))
        self.trace = tr
        return bytes(self.out)


def zc_context(orient, h, v, d):
    """Table D.1: h, v, d = significant horizontal (0..2), vertical (0..2), diagonal (0..4) neighbours."""
    if orient == HL:
        h, v = v, h
    if orient == HH:
        hv = h + v
        if d >= 3:
            return 8
        if d == 2:
            return 7 if hv >= 1 else 6
        if d == 1:
            return 5 if hv >= 2 else 3 + hv
        return 2 if hv >= 2 else hv
    if h == 2:
        return 8
    if h == 1:
        return 7 if v >= 1 else (6 if d >= 1 else 5)
    if v == 2:
        return 4
    if v == 1:
        return 3
    return 2 if d >= 2 else d


def t1_encode(mag, neg, w, h, orient, nplanes, trace=None):
    """One code-block (Annex D): mag / neg are row-major lists, nplanes the bit length of the largest magnitude (>= 1).
    -> (bytes of the single codeword segment, coding passes = 3 nplanes - 2).

    trace (and the MQ coder's, see MQEncoder): "zc" {(orient, neighbour pattern, "sp" / "cu")} with the pattern's bits as NEIGHBOURS,
    "zc_ctx" {(orient, context, decision)}, "sign" {((W, E, N, S contributions), centre negative)}, "rows" {(orient, pass "sp" / "mr" / "cu",
    rows of the stripe, mask of the rows the pass codes in one column)}, "rl" {0 .. 3 the row that ends the run, 4 no row},
    "rl_off" {(orient, mask of significant rows, of visited rows, of rows with a significant neighbour)} of a full column without run-length
    mode, "edge_sig" {"col" / "row": a sample of the last column / row becomes significant}, "mag_ctx" {context}, "nplanes", "block"
    {(w, h, orient)}."""
    mq = MQEncoder(trace)
    enc = mq.encode
    tr = trace
    W = w + 2
    F = [0] * ((h + 2) * W)  # flags with a border of never-significant samples
    for y in range(h):
        for x in range(w):
            if neg[y * w + x]:
                F[(y + 1) * W + x + 1] = F_NEG
    if tr is not None:
        count(tr, "nplanes", nplanes)
        count(tr, "block", (w, h, orient))
        all_rows = (orient, "cu", 4, 15)  # run-length mode: every row is a candidate
        n_zc, n_ctx, n_rows, n_mag = (tr.setdefault(key, {}) for key in ("zc", "zc_ctx", "rows", "mag_ctx"))  # the hot counters, inline

    def neighbours(i):
        hh = (F[i - 1] & 1) + (F[i + 1] & 1)
        vv = (F[i - W] & 1) + (F[i + W] & 1)
        dd = (F[i - W - 1] & 1) + (F[i - W + 1] & 1) + (F[i + W - 1] & 1) + (F[i + W + 1] & 1)
        return hh, vv, dd

    def contribution(i):  # of a neighbour to the sign context: +1 positive, -1 negative, 0 insignificant
        f = F[i]
        return 0 if not f & 1 else (-1 if f & 2 else 1)

    def code_sign(i):
        hc = max(-1, min(1, contribution(i - 1) + contribution(i + 1)))
        vc = max(-1, min(1, contribution(i - W) + contribution(i + W)))
        if hc < 0 or (hc == 0 and vc < 0):
            hc, vc, flip = -hc, -vc, 1
        else:
            flip = 0
        cx = CTX_SIGN + (3 + vc if hc else vc)  # (0,0) 9, (0,1) 10, (1,-1) 11, (1,0) 12, (1,1) 13
        if tr is not None:
            count(tr, "sign", ((contribution(i - 1), contribution(i + 1), contribution(i - W), contribution(i + W)), (F[i] >> 1) & 1))
            x, y = i % W - 1, i // W - 1
            if x == w - 1:
                count(tr, "edge_sig", "col")
            if y == h - 1:
                count(tr, "edge_sig", "row")
        enc(cx, ((F[i] >> 1) & 1) ^ flip)

    def cleanup_rows(x, y0):  # traced: the rows of a column that the cleanup pass codes
        rows, i = 0, (y0 + 1) * W + x + 1
        for k in range(min(4, h - y0)):
            if not F[i + k * W] & (F_SIG | F_VISIT):
                rows |= 1 << k
        key = (orient, "cu", min(4, h - y0), rows)
        n_rows[key] = n_rows.get(key, 0) + 1

    def code_zc(i, bit, kind):
        cx = zc_context(orient, *neighbours(i))
        if tr is not None:
            pattern = ((F[i - W - 1] & 1) | (F[i - W] & 1) << 1 | (F[i - W + 1] & 1) << 2 | (F[i - 1] & 1) << 3 | (F[i + 1] & 1) << 4
                       | (F[i + W - 1] & 1) << 5 | (F[i + W] & 1) << 6 | (F[i + W + 1] & 1) << 7)
            key = (orient, pattern, kind)
            n_zc[key] = n_zc.get(key, 0) + 1
            key = (orient, cx, bit)
            n_ctx[key] = n_ctx.get(key, 0) + 1
        enc(cx, bit)

    for p in range(nplanes - 1, -1, -1):
        if p != nplanes - 1:
            # significance propagation
            for y0 in range(0, h, 4):
                for x in range(w):
                    rows = 0
                    for y in range(y0, min(y0 + 4, h)):
                        i = (y + 1) * W + x + 1
                        if F[i] & F_SIG:
                            continue
                        hh, vv, dd = neighbours(i)
                        if hh + vv + dd == 0:
                            continue
                        rows |= 1 << (y - y0)
                        bit = (mag[y * w + x] >> p) & 1
                        code_zc(i, bit, "sp")
                        if bit:
                            code_sign(i)
                            F[i] |= F_SIG
                        F[i] |= F_VISIT
                    if tr is not None:
                        key = (orient, "sp", min(4, h - y0), rows)
                        n_rows[key] = n_rows.get(key, 0) + 1
            # magnitude refinement
            for y0 in range(0, h, 4):
                for x in range(w):
                    rows = 0
                    for y in range(y0, min(y0 + 4, h)):
                        i = (y + 1) * W + x + 1
                        f = F[i]
                        if (f & (F_SIG | F_VISIT)) != F_SIG:
                            continue
                        rows |= 1 << (y - y0)
                        if f & F_REFINED:
                            cx = CTX_MAG + 2
                        else:
                            cx = CTX_MAG + (1 if sum(neighbours(i)) else 0)
                        if tr is not None:
                            n_mag[cx] = n_mag.get(cx, 0) + 1
                        enc(cx, (mag[y * w + x] >> p) & 1)
                        F[i] = f | F_REFINED
                    if tr is not None:
                        key = (orient, "mr", min(4, h - y0), rows)
                        n_rows[key] = n_rows.get(key, 0) + 1
        # cleanup
        for y0 in range(0, h, 4):
            for x in range(w):
                first = 0
                if y0 + 4 <= h:
                    idx = [(y0 + k + 1) * W + x + 1 for k in range(4)]
                    if all(not F[i] & (F_SIG | F_VISIT) and sum(neighbours(i)) == 0 for i in idx):
                        r = next((k for k in range(4) if (mag[(y0 + k) * w + x] >> p) & 1), 4)
                        if tr is not None:
                            count(tr, "rl", r)
                            n_rows[all_rows] = n_rows.get(all_rows, 0) + 1
                        if r == 4:
                            enc(CTX_RL, 0)
                            continue
                        enc(CTX_RL, 1)
                        enc(CTX_UNI, r >> 1)
                        enc(CTX_UNI, r & 1)
                        code_sign(idx[r])
                        F[idx[r]] |= F_SIG
                        first = r + 1
                    elif tr is not None:
                        cleanup_rows(x, y0)
                        count(tr, "rl_off", (orient,) + tuple(sum(1 << k for k, i in enumerate(idx) if t(i)) for t in (
                            lambda i: F[i] & F_SIG, lambda i: F[i] & F_VISIT, lambda i: sum(neighbours(i)))))
                elif tr is not None:
                    cleanup_rows(x, y0)
                for y in range(y0 + first, min(y0 + 4, h)):
                    i = (y + 1) * W + x + 1
                    if F[i] & (F_SIG | F_VISIT):
                        continue
                    bit = (mag[y * w + x] >> p) & 1
                    code_zc(i, bit, "cu")
                    if bit:
                        code_sign(i)
                        F[i] |= F_SIG
        for i in range(len(F)):
            F[i] &= ~F_VISIT
    return mq.flush(), 3 * nplanes - 2


# ---- the 5/3 transform ------------------------------------------------------------------------------------------------

def _lift_53(x):
    """Forward reversible 5/3 along axis 0 of an int64 array whose first sample has an even coordinate (F.4.8.1), with
    whole-sample symmetric extension: -> (low, high).  A length-1 signal passes through."""
    n = x.shape[0]
    if n == 1:
        return x.copy(), x[:0].copy()

    def at(i):
        i = np.abs(i)
        i = np.where(i >= n, 2 * (n - 1) - i, i)
        return x[np.abs(i)]
    nh, nl = n // 2, (n + 1) // 2
    k = np.arange(-1, nl)  # high-pass samples -1 .. nl - 1, the extension included
    d = at(2 * k + 1) - ((at(2 * k) + at(2 * k + 2)) >> 1)
    s = x[0::2] + ((d[:-1] + d[1:] + 2) >> 2)
    return s, d[1:1 + nh]


def dwt_53(a, levels):
    """`levels` stages, columns first and then rows (F.4.2), in place in the Mallat layout: after a stage the LL band is
    the top left ceil(h/2) x ceil(w/2) corner."""
    a = a.astype(np.int64).copy()
    h, w = a.shape
    for _ in range(levels):
        lo, hi = _lift_53(a[:h, :w])
        a[:h, :w] = np.concatenate([lo, hi], axis=0)
        lo, hi = _lift_53(a[:h, :w].T)
        a[:h, :w] = np.concatenate([lo, hi], axis=0).T
        h, w = (h + 1) // 2, (w + 1) // 2
    return a


def resolutions(rows, cols, levels):
    """Per resolution 0 .. levels the subbands in packet order as (orient, x0, y0, w, h) in the Mallat plane."""
    dims = [(rows, cols)]
    for _ in range(levels):
        dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
    res = [[(LL, 0, 0, dims[levels][1], dims[levels][0])]]
    for r in range(1, levels + 1):
        d = levels - r + 1
        ph, pw = dims[d - 1]
        hl, wl = dims[d]
        res.append([(HL, wl, 0, pw - wl, hl), (LH, 0, hl, wl, ph - hl), (HH, wl, hl, pw - wl, ph - hl)])
    return res


# ---- Tier-2 ------------------------------------------------------------------------------------------------------------

class BitWriter:
    """Packet header bits (B.10.1): after a byte 0xFF the next byte carries 7 bits; a header does not end in 0xFF."""

    def __init__(self, trace=None):
        """trace: "hdr_ff" {"inside": a byte 0xFF with header bits behind it}, "hdr_end" {"partial", "partial_after_ff", "full",
        "full_ff": how the header's last byte stands, the last with the appended zero byte}."""
        self.trace = trace
        self.out = bytearray()
        self.cur, self.free, self.cap = 0, 8, 8  # cap: bits the byte under construction takes, free: those still missing

    def put(self, bit):
        self.cur = (self.cur << 1) | bit
        self.free -= 1
        if self.free == 0:
            self.out.append(self.cur)
            self.free = self.cap = 7 if self.cur == 0xFF else 8
            self.cur = 0

    def bits(self, value, n):
        for k in range(n - 1, -1, -1):
            self.put((value >> k) & 1)

    def finish(self):
        if self.trace is not None:
            partial, ff = self.free != self.cap, bool(self.out) and self.out[-1] == 0xFF
            count(self.trace, "hdr_end", ("partial_after_ff" if ff else "partial") if partial else ("full_ff" if ff else "full"))
            if 0xFF in self.out[:-1] or (ff and partial):
                count(self.trace, "hdr_ff", "inside")
        if self.free != self.cap:
            self.out.append(self.cur << self.free)  # zero padding: never 0xFF
            self.cur, self.free, self.cap = 0, 8, 8
        if self.out and self.out[-1] == 0xFF:
            self.out.append(0)
        return bytes(self.out)


class TagTree:
    """B.10.2.  Level 0 holds the w x h leaves; every further level halves both sizes, rounding up, down to 1 x 1."""

    def __init__(self, w, h, leaves, trace=None, name="tree"):
        """trace: "tt_levels" {(w, h, levels)}, "tt_learnt" {(name, level): a node's value is first told at that level, the leaves 0},
        "tt_low" {(name, level): a node starts from a lower bound above 0 that its parent handed down}."""
        self.trace, self.name = trace, name
        self.dims = [(w, h)]
        while self.dims[-1] != (1, 1):
            pw, ph = self.dims[-1]
            self.dims.append(((pw + 1) // 2, (ph + 1) // 2))
        self.val = [list(leaves)]
        for lv in range(1, len(self.dims)):
            pw, ph = self.dims[lv - 1]
            cw, ch = self.dims[lv]
            prev = self.val[-1]
            self.val.append([min(prev[yy * pw + xx] for yy in range(2 * y, min(2 * y + 2, ph)) for xx in range(2 * x, min(2 * x + 2, pw)))
                             for y in range(ch) for x in range(cw)])
        self.low = [[0] * len(v) for v in self.val]
        self.known = [[False] * len(v) for v in self.val]
        if trace is not None:
            count(trace, "tt_levels", (w, h, len(self.dims)))

    def encode(self, bw, x, y, threshold):
        low = 0
        for lv in range(len(self.dims) - 1, -1, -1):
            k = (y >> lv) * self.dims[lv][0] + (x >> lv)
            if self.trace is not None and low > self.low[lv][k]:
                count(self.trace, "tt_low", (self.name, lv))
            low = max(low, self.low[lv][k])
            while low < threshold:
                if low >= self.val[lv][k]:
                    if not self.known[lv][k]:
                        bw.put(1)
                        self.known[lv][k] = True
                        if self.trace is not None:
                            count(self.trace, "tt_learnt", (self.name, lv))
                    break
                bw.put(0)
                low += 1
            self.low[lv][k] = low


def put_passes(bw, n):
    """Table B.4."""
    if n == 1:
        bw.put(0)
    elif n == 2:
        bw.bits(0b10, 2)
    elif n <= 5:
        bw.bits(0b11, 2); bw.bits(n - 3, 2)
    elif n <= 36:
        bw.bits(0b1111, 4); bw.bits(n - 6, 5)
    else:
        bw.bits(0x1FF, 9); bw.bits(n - 37, 7)


def packet(bands, trace=None):
    """One packet: bands = [(ncw, nch, [(passes, zero_planes, data)], mb)] -> header + bodies.
    trace (and BitWriter's and TagTree's): "included" {(blocks of the band, blocks included)}, "zbp" {zero bit-planes}, "passes" {n},
    "lblock" {growth}, "seglen" {bytes}."""
    bw = BitWriter(trace)
    bw.put(1 if any(ncw * nch for ncw, nch, _, _ in bands) else 0)
    body = bytearray()
    for ncw, nch, blocks, mb in bands:
        if ncw * nch == 0:
            continue
        incl = TagTree(ncw, nch, [0 if p else 1 for p, _, _ in blocks], trace, "incl")
        zbp = TagTree(ncw, nch, [z if p else mb for p, z, _ in blocks], trace, "zbp")
        if trace is not None:
            count(trace, "included", (len(blocks), sum(1 for p, _, _ in blocks if p)))
        for k, (passes, zeros, data) in enumerate(blocks):
            x, y = k % ncw, k // ncw
            incl.encode(bw, x, y, 1)
            if not passes:
                continue
            zbp.encode(bw, x, y, 1 << 30)
            put_passes(bw, passes)
            need = len(data).bit_length() - (passes.bit_length() - 1)  # Lblock starts at 3
            grow = max(0, need - 3)
            if trace is not None:
                for key, item in (("zbp", zeros), ("passes", passes), ("lblock", grow), ("seglen", len(data))):
                    count(trace, key, item)
            for _ in range(grow):
                bw.put(1)
            bw.put(0)
            bw.bits(len(data), 3 + grow + passes.bit_length() - 1)
            body += data
    return bw.finish() + bytes(body)


# ---- the file ----------------------------------------------------------------------------------------------------------

def main_header(rows, cols, precision, levels, codeblock):
    """SOC, SIZ, COD, QCD."""
    siz = struct.pack(">HHIIIIIIIIHBBB", 41, 0, cols, rows, 0, 0, cols, rows, 0, 0, 1, precision - 1, 1, 1)
    cbe = codeblock.bit_length() - 1 - 2
    cod = struct.pack(">HBBHBBBBBB", 12, 0, 0, 1, 0, levels, cbe, cbe, 0, 1)
    exps = [precision] + [precision + g for _ in range(levels) for g in (1, 1, 2)]
    qcd = struct.pack(">HB", 3 + len(exps), GUARD_BITS << 5) + bytes(e << 3 for e in exps)
    return b"\xff\x4f\xff\x51" + siz + b"\xff\x52" + cod + b"\xff\x5c" + qcd


def jp2_header(rows, cols, precision):
    """Signature, ftyp, jp2h (ihdr, colr) and the head of jp2c without its length: 81 bytes, 85 with it."""
    ihdr = struct.pack(">I4sIIHBBBB", 22, b"ihdr", rows, cols, 1, precision - 1, 7, 0, 0)
    colr = struct.pack(">I4sBBBI", 15, b"colr", 1, 0, 0, 17)
    return (b"\x00\x00\x00\x0cjP  \r\n\x87\n" + struct.pack(">I4s4sI4s", 20, b"ftyp", b"jp2 ", 0, b"jp2 ")
            + struct.pack(">I4s", 8 + len(ihdr) + len(colr), b"jp2h") + ihdr + colr)


def encode(image, precision, shift=0, levels=5, codeblock=64, jp2=False, trace=None):
    """trace: what t1_encode and packet collect over the file, and "levels", "precision", "lengths" {a length the transform ran on}."""
    img = np.asarray(image)
    assert img.ndim == 2 and img.dtype in (np.uint8, np.uint16) and codeblock in (32, 64)
    assert 2 <= precision <= 8 * img.dtype.itemsize and 0 <= shift <= 15 and precision - shift >= 1 and 0 <= levels <= 8
    rows, cols = img.shape
    v = img.astype(np.int64) << shift
    if int(v.max()) >= 1 << precision:
        raise OverflowError("a sample does not fit the precision")
    plane = dwt_53(v - (1 << (precision - 1)), levels)
    if trace is not None:
        count(trace, "levels", levels)
        count(trace, "precision", precision)
        h, w = rows, cols
        for _ in range(levels):
            count(trace, "lengths", h)
            count(trace, "lengths", w)
            h, w = (h + 1) // 2, (w + 1) // 2
    packets = bytearray()
    for bands in resolutions(rows, cols, levels):
        pk = []
        for orient, x0, y0, w, h in bands:
            mb = GUARD_BITS + precision + GAIN[orient] - 1
            ncw, nch = -(-w // codeblock), -(-h // codeblock)
            blocks = []
            for by in range(0, h, codeblock):
                for bx in range(0, w, codeblock):
                    blk = plane[y0 + by:y0 + min(by + codeblock, h), x0 + bx:x0 + min(bx + codeblock, w)]
                    nplanes = int(np.abs(blk).max()).bit_length()
                    if nplanes > mb:
                        raise OverflowError("a coefficient needs more than the guard bits allow")
                    if nplanes == 0:
                        blocks.append((0, mb, b""))
                        continue
                    data, passes = t1_encode(np.abs(blk).ravel().tolist(), (blk < 0).ravel().tolist(), blk.shape[1], blk.shape[0], orient,
                                             nplanes, trace)
                    blocks.append((passes, mb - nplanes, data))
            pk.append((ncw if w and h else 0, nch if w and h else 0, blocks, mb))
        packets += packet(pk, trace)
    psot = 12 + 2 + len(packets)
    cs = (main_header(rows, cols, precision, levels, codeblock) + b"\xff\x90" + struct.pack(">HHIBB", 10, 0, psot, 0, 1) + b"\xff\x93"
          + bytes(packets) + b"\xff\xd9")
    if not jp2:
        return cs
    return jp2_header(rows, cols, precision) + struct.pack(">I4s", 8 + len(cs), b"jp2c") + cs


def info(file):
    """(rows, cols, precision) of a raw codestream or a JP2 file from its SIZ; ValueError for anything else."""
    f = bytes(file)
    pos = 0
    if f[:12] == b"\x00\x00\x00\x0cjP  \r\n\x87\n":
        pos = 12
        while True:
            if pos + 8 > len(f):
                raise ValueError("JP2 without a jp2c box")
            ln, typ, hd = int.from_bytes(f[pos:pos + 4], "big"), f[pos + 4:pos + 8], 8
            if ln == 1:
                if pos + 16 > len(f):
                    raise ValueError("truncated box")
                ln, hd = int.from_bytes(f[pos + 8:pos + 16], "big"), 16
            if typ == b"jp2c":
                pos += hd
                break
            if ln == 0 or ln < hd or pos + ln > len(f):
                raise ValueError("JP2 without a jp2c box")
            pos += ln
    if f[pos:pos + 4] != b"\xff\x4f\xff\x51" or pos + 6 > len(f):
        raise ValueError("no SOC + SIZ")
    lsiz = int.from_bytes(f[pos + 4:pos + 6], "big")
    if lsiz < 41 or pos + 4 + lsiz > len(f):
        raise ValueError("truncated SIZ")
    _, xs, ys, xo, yo, _, _, _, _, nc, ssiz = struct.unpack_from(">HIIIIIIIIHB", f, pos + 6)
    if nc != 1 or lsiz != 41 or ssiz & 0x80 or ssiz + 1 > 16 or xs <= xo or ys <= yo:
        raise ValueError("not a one-component unsigned image of at most 16 bits")
    return ys - yo, xs - xo, ssiz + 1


def raster_cases(rows, cols, precision, dtype, seed=0):
    """The contents the tests encode at every shape, each picking out one mechanism."""
    rng = np.random.default_rng(seed * 1000003 + rows * 131 + cols)
    top = (1 << precision) - 1
    yy, xx = np.mgrid[0:rows, 0:cols]
    single = np.zeros((rows, cols), np.int64) + (1 << (precision - 1))  # level-shifted zero everywhere but one sample
    single[rows // 2, (2 * cols) // 3] = top
    return {k: v.astype(dtype) for k, v in {
        "zero": np.full((rows, cols), 1 << (precision - 1)),  # every coefficient 0: no code-block included
        "max": np.full((rows, cols), top),
        "checker": ((yy + xx) & 1) * top,
        "noise": rng.integers(0, top + 1, (rows, cols)),
        "ramp": (yy * 7 + xx * 3) % (top + 1),
        "single": single,
    }.items()}


# ---- the test matrix ---------------------------------------------------------------------------------------------------
# The smallest shapes at which each mechanism can still go wrong: length-1 lifting, empty subbands and empty packets at 5
# levels (1 x 1, 1 x 7, 7 x 1); 5 x 3; a one-sample-wide edge code-block and odd subband sizes (33 x 65 at 32, 65 x 33 at
# 64); two code-blocks across a level-1 subband and partial stripes (130 x 70: 35 rows are no multiple of 4).
# What this matrix does not reach (2 to 4 and 6 to 8 levels, precisions other than 8 / 12 / 16, tag trees of more than 4 levels or with
# mixed inclusion, more than 17 bit-planes, planted neighbour patterns and segment lengths) is in tests/jpeg2000_edges.py, and
# tests/test_jpeg2000_edges_host.py pins what the matrix itself reaches, so SHAPES, LEVELS or raster_cases cannot lose it silently.
SHAPES = ((1, 1, (32, 64)), (1, 7, (64,)), (7, 1, (32,)), (5, 3, (64,)), (33, 65, (32,)), (65, 33, (64,)), (130, 70, (32, 64)))
PRECISIONS = {8: np.uint8, 12: np.uint16, 16: np.uint16}
LEVELS = (0, 1, 5)


@functools.lru_cache(maxsize=None)
def matrix(precision):
    """[(rows, cols, codeblock, levels, names, rasters (n, rows, cols), files)] over SHAPES x LEVELS at one precision."""
    out = []
    for rows, cols, cbs in SHAPES:
        c = raster_cases(rows, cols, precision, PRECISIONS[precision])
        imgs = np.stack(list(c.values()))
        for cb in cbs:
            for levels in LEVELS:
                out.append((rows, cols, cb, levels, list(c), imgs, [encode(x, precision, 0, levels, cb) for x in imgs]))
    return out


@functools.lru_cache(maxsize=None)
def phantoms():
    """128 x 128 phantoms and 16-bit noise, with the parameters they are encoded at: [(raster, kwargs, file)]."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "2023-compact-image-compression_amd", "cct_hip", "synth.py")
    spec = importlib.util.spec_from_file_location("_j2k_synth", path)  # the generator alone: no device library is loaded
    synth = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(synth)
    noise = np.random.default_rng(16).integers(0, 65536, (128, 128)).astype(np.uint16)
    out = []
    for img, kw in ((synth.ct_phantom(0, n=128), dict(precision=16, levels=5, codeblock=64)),
                    (synth.ct_phantom(1, n=128), dict(precision=16, levels=5, codeblock=32)),
                    (synth.ct_phantom(2, n=128), dict(precision=12, levels=1, codeblock=64)),
                    (synth.ct_phantom(3, n=128), dict(precision=16, shift=4, levels=5, codeblock=64, jp2=True)),
                    (noise, dict(precision=16, levels=5, codeblock=64)),
                    (noise, dict(precision=16, levels=0, codeblock=32, jp2=True))):
        out.append((img, kw, encode(img, **kw)))
    return out


def packet_data(file):
    """The bytes between SOD and EOC of a file of this encoder."""
    at = file.index(b"\xff\x93", file.index(b"\xff\x90"))
    return file[at + 2:-2]
