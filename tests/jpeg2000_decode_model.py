"""Plain-Python model of the device JPEG 2000 Part-1 lossless decoder (csrc/jpeg2000_decode_kernels.hip and the marker walk of
csrc/api_jpeg2000.cpp), written from T.800.  The device is held to decode() on every input, damaged or not.

    decode(file, rows=None, cols=None, bits=16, shift=0) -> a status name ("CCT_E_J2K", "CCT_E_MIXED", "CCT_E_STREAM") or the raster
    walk(file) -> the parameters of a file this decoder takes, Refused(status name) otherwise
    build(image, precision, ...) -> files neither this project's encoder nor OpenJPEG writes: one guard bit, a COM in the tile-part header,
    Psot 0, no EOC (put together from the encoder model's t1_encode, packet, BitWriter and TagTree)
    foreign_set(), refused_set(), handbuilt_set(), marker_cases(), damaged_set() -> the file sets of the tests and of
    tools/debug/j2k_dec_host_emu, computed once

What is taken: a raw codestream or a JP2 file (the boxes are walked to jp2c); one unsigned component of 2 .. 16 bits, image
and tile origins 0, one tile, subsampling 1; one tile-part (TPsot 0, TNsot 0 or 1, Psot 0: to the end of the codestream);
COD with maximal precincts, no SOP / EPH, any progression order, 1 .. 32 layers, no MCT, 0 .. 8 levels, code-blocks of
4 .. 64 by 4 .. 64, style 0, the 5/3 transform; QCD style 0 with any guard bits and exponents as long as no subband has
more than MB_MAX magnitude bit-planes; COM, TLM, PLM, PLT and CRG anywhere they may stand.  Everything else is CCT_E_J2K.

Damage inside the MQ-coded bytes cannot be detected; the result is defined instead: the MQ decoder reads 0xFF beyond a
block's last byte, coefficients and lifting are two's complement modulo 2^32, and the sample is clamped to 0 .. 2^precision - 1
after the level shift and then shifted right.

Pure-Python MQ decoding is slow: keep inputs at or below 130 x 70 and 128 x 128.
"""
import functools
import io
import struct

import numpy as np

import jpeg2000_model as m
from jpeg2000_model import CTX_MAG, CTX_RL, CTX_SIGN, CTX_UNI, F_NEG, F_REFINED, F_SIG, F_VISIT, GAIN, MQ_TABLE, N_CTX, resolutions, zc_context

MB_MAX = 19          # magnitude bit-planes the Tier-1 word holds (bits 12 .. 30, the encoder's layout)
M32 = 0xFFFFFFFF
SKIPPED = (0xFF64, 0xFF55, 0xFF57, 0xFF58, 0xFF63)  # COM, TLM, PLM, PLT, CRG


class Refused(Exception):
    pass


# ---- the marker walk (host) -------------------------------------------------------------------------------------------

def _codestream(f):
    """(start, end) of the codestream: the whole file, or the contents of the jp2c box."""
    if f[:12] != b"\x00\x00\x00\x0cjP  \r\n\x87\n":
        return 0, len(f)
    pos = 12
    while True:
        if len(f) - pos < 8:
            raise Refused("CCT_E_J2K")
        ln, typ, hd = int.from_bytes(f[pos:pos + 4], "big"), f[pos + 4:pos + 8], 8
        if ln == 1:
            if len(f) - pos < 16:
                raise Refused("CCT_E_J2K")
            ln, hd = int.from_bytes(f[pos + 8:pos + 16], "big"), 16
        if typ == b"jp2c":
            return pos + hd, (min(pos + ln, len(f)) if ln >= hd else len(f))
        if ln < hd or ln > len(f) - pos:
            raise Refused("CCT_E_J2K")
        pos += ln


def walk(file):
    f = bytes(file)
    pos, end = _codestream(f)
    if end - pos < 6 or f[pos:pos + 4] != b"\xff\x4f\xff\x51":
        raise Refused("CCT_E_J2K")
    lsiz = int.from_bytes(f[pos + 4:pos + 6], "big")
    if lsiz != 41 or end - pos - 4 < lsiz:
        raise Refused("CCT_E_J2K")
    _, xs, ys, xo, yo, xt, yt, xto, yto, nc, ssiz, xr, yr = struct.unpack_from(">HIIIIIIIIHBBB", f, pos + 6)
    if (nc != 1 or ssiz & 0x80 or not 2 <= ssiz + 1 <= 16 or xs == 0 or ys == 0 or xs > 0x7FFFFFFF or ys > 0x7FFFFFFF or xo or yo or xto or yto
            or xt < xs or yt < ys or xr != 1 or yr != 1):
        raise Refused("CCT_E_J2K")
    P = dict(rows=ys, cols=xs, precision=ssiz + 1, cod=None, qcd=None)
    pos += 4 + lsiz
    sot = None
    while True:  # main header up to SOT, then the tile-part header up to SOD
        if end - pos < 2 or f[pos] != 0xFF:
            raise Refused("CCT_E_J2K")
        mk = 0xFF00 | f[pos + 1]
        if mk == 0xFF93:
            if sot is None:
                raise Refused("CCT_E_J2K")
            pos += 2
            break
        if end - pos < 4:
            raise Refused("CCT_E_J2K")
        ln = int.from_bytes(f[pos + 2:pos + 4], "big")
        if ln < 2 or ln > end - pos - 2:
            raise Refused("CCT_E_J2K")
        seg = f[pos + 4:pos + 2 + ln]
        if mk == 0xFF90:
            if sot is not None or len(seg) != 8 or seg[0] or seg[1] or seg[6] != 0 or seg[7] > 1:
                raise Refused("CCT_E_J2K")
            sot = pos
            psot = int.from_bytes(seg[2:6], "big")
        elif mk == 0xFF52:
            if len(seg) != 10 or seg[0] != 0 or seg[1] > 4 or seg[4] != 0 or seg[8] != 0 or seg[9] != 1:
                raise Refused("CCT_E_J2K")
            layers, levels, xcb, ycb = int.from_bytes(seg[2:4], "big"), seg[5], seg[6] + 2, seg[7] + 2
            if not 1 <= layers <= 32 or levels > 8 or seg[6] > 4 or seg[7] > 4:
                raise Refused("CCT_E_J2K")
            P["cod"] = dict(seq=0 if seg[1] == 0 else 1, layers=layers, levels=levels, xcb=xcb, ycb=ycb)
        elif mk == 0xFF5C:
            if len(seg) < 1 or seg[0] & 31:
                raise Refused("CCT_E_J2K")
            P["qcd"] = dict(guard=seg[0] >> 5, exps=[b >> 3 for b in seg[1:]])
        elif mk not in SKIPPED:
            raise Refused("CCT_E_J2K")  # COC, QCC, RGN, POC, PPM, PPT, a second SIZ, anything of Part 2
        pos += 2 + ln
    if P["cod"] is None or P["qcd"] is None:
        raise Refused("CCT_E_J2K")
    P.update(P.pop("cod"))
    q = P.pop("qcd")
    if len(q["exps"]) < 1 + 3 * P["levels"]:
        raise Refused("CCT_E_J2K")
    P["mb"] = [max(0, q["guard"] + e - 1) for e in q["exps"][:1 + 3 * P["levels"]]]
    if max(P["mb"]) > MB_MAX:
        raise Refused("CCT_E_J2K")
    P["data0"] = pos
    P["data1"] = min(sot + psot, end) if psot else end
    if P["data1"] < P["data0"]:
        raise Refused("CCT_E_J2K")
    return P


# ---- packets (device: one lane per file) ----------------------------------------------------------------------------

class BitReader:
    """B.10.1: the byte behind a 0xFF carries 7 bits.  Reading past the end sets err and gives zeros."""

    def __init__(self, d, pos, end):
        self.d, self.pos, self.end = d, pos, end
        self.cur, self.left, self.err = 0, 0, False

    def get(self):
        if self.left == 0:
            if self.pos >= self.end:
                self.err = True
                return 0
            self.left = 7 if self.cur == 0xFF else 8
            self.cur = self.d[self.pos]
            self.pos += 1
        self.left -= 1
        return (self.cur >> self.left) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.get()
        return v

    def align(self):  # the end of a packet header: a header that ends in 0xFF is followed by a stuffed zero byte
        if self.cur == 0xFF:
            if self.pos >= self.end:
                self.err = True
            else:
                self.pos += 1
        self.cur, self.left = 0, 0


class TagTreeDecoder:
    """B.10.2; a node's value is unknown (255) until a 1 bit fixes it at the node's lower bound."""

    def __init__(self, w, h):
        self.dims = [(w, h)]
        while self.dims[-1] != (1, 1):
            pw, ph = self.dims[-1]
            self.dims.append(((pw + 1) // 2, (ph + 1) // 2))
        self.low = [[0] * (pw * ph) for pw, ph in self.dims]
        self.val = [[255] * (pw * ph) for pw, ph in self.dims]

    def decode(self, br, x, y, threshold):
        """True if the leaf's value is known and below the threshold."""
        low = 0
        for lv in range(len(self.dims) - 1, -1, -1):
            k = (y >> lv) * self.dims[lv][0] + (x >> lv)
            low = max(low, self.low[lv][k])
            while low < threshold and low < self.val[lv][k]:
                if br.get():
                    self.val[lv][k] = low
                else:
                    low += 1
            self.low[lv][k] = low
        return self.val[0][k] < threshold


def get_passes(br):
    """Table B.4."""
    if not br.get():
        return 1
    if not br.get():
        return 2
    v = br.bits(2)
    if v != 3:
        return 3 + v
    v = br.bits(5)
    if v != 31:
        return 6 + v
    return 37 + br.bits(7)


def parse_packets(P, f, trace=None):
    """-> per resolution the subbands, each with its grid, rectangle, Mb and code-blocks (passes, zero bit-planes, bytes);
    Refused("CCT_E_STREAM") for what the device finds while it parses.  trace collects (start of the header, end of the header,
    end of the bodies) of every packet."""
    cw, ch = 1 << P["xcb"], 1 << P["ycb"]
    res, b = [], 0
    for bands in resolutions(P["rows"], P["cols"], P["levels"]):
        out = []
        for orient, x0, y0, w, h in bands:
            ncw, nch = (-(-w // cw), -(-h // ch)) if w and h else (0, 0)
            band = dict(ncw=ncw, nch=nch, orient=orient, x0=x0, y0=y0, w=w, h=h, mb=P["mb"][b],
                        blocks=[dict(passes=0, zbp=0, data=bytearray(), lblock=3, included=False) for _ in range(ncw * nch)])
            if ncw:
                band["incl"], band["zbpt"] = TagTreeDecoder(ncw, nch), TagTreeDecoder(ncw, nch)
            out.append(band)
            b += 1
        res.append(out)
    br = BitReader(f, P["data0"], P["data1"])
    nres, layers = P["levels"] + 1, P["layers"]
    order = [(l, r) for l in range(layers) for r in range(nres)] if P["seq"] == 0 else [(l, r) for r in range(nres) for l in range(layers)]
    for layer, r in order:
        pending, start = [], br.pos
        if br.get():
            for band in res[r]:
                for k, blk in enumerate(band["blocks"]):
                    x, y = k % band["ncw"], k // band["ncw"]
                    if blk["included"]:
                        inc = br.get()
                    else:
                        inc = band["incl"].decode(br, x, y, layer + 1)
                    if not inc:
                        continue
                    if not blk["included"]:
                        blk["included"] = True
                        for t in range(1, band["mb"] + 2):
                            if band["zbpt"].decode(br, x, y, t):
                                blk["zbp"] = t - 1
                                break
                        else:
                            raise Refused("CCT_E_STREAM")  # more zero bit-planes than Mb
                    n = get_passes(br)
                    while br.get():
                        blk["lblock"] += 1
                        if blk["lblock"] > 32:
                            raise Refused("CCT_E_STREAM")
                    ln = br.bits(blk["lblock"] + n.bit_length() - 1)
                    blk["passes"] += n
                    if br.err or blk["passes"] > 3 * (band["mb"] - blk["zbp"]) - 2:
                        raise Refused("CCT_E_STREAM")
                    pending.append((blk, ln))
        br.align()
        if br.err:
            raise Refused("CCT_E_STREAM")
        hdr_end = br.pos
        for blk, ln in pending:
            if ln > br.end - br.pos:
                raise Refused("CCT_E_STREAM")
            blk["data"] += f[br.pos:br.pos + ln]
            br.pos += ln
        if trace is not None:
            trace.append((start, hdr_end, br.pos))
    return res


# ---- Tier-1 -----------------------------------------------------------------------------------------------------------

class MQDecoder:
    """T.800 Annex C.3; bytes beyond the segment read as 0xFF, C is a 32-bit register."""

    def __init__(self, data, trace=None):
        """trace: "mq_state" and "mq_ctx" as jpeg2000_model.MQEncoder's."""
        self.trace = trace
        if trace is not None:
            self.n_state, self.n_ctx = trace.setdefault("mq_state", {}), trace.setdefault("mq_ctx", {})
        self.d, self.n, self.bp = data, len(data), 0
        self.state = [0] * N_CTX
        self.mps = [0] * N_CTX
        self.state[0], self.state[CTX_RL], self.state[CTX_UNI] = 4, 3, 46
        self.c = self._byte(0) << 16
        self._bytein()
        self.c = (self.c << 7) & M32
        self.ct -= 7
        self.a = 0x8000

    def _byte(self, i):
        return self.d[i] if i < self.n else 0xFF

    def _bytein(self):
        if self._byte(self.bp) == 0xFF:
            b1 = self._byte(self.bp + 1)
            if b1 > 0x8F:
                self.c = (self.c + 0xFF00) & M32
                self.ct = 8
            else:
                self.bp += 1
                self.c = (self.c + (b1 << 9)) & M32
                self.ct = 7
        else:
            self.bp += 1
            self.c = (self.c + (self._byte(self.bp) << 8)) & M32
            self.ct = 8

    def _renorm(self):
        while True:
            if self.ct == 0:
                self._bytein()
            self.a <<= 1
            self.c = (self.c << 1) & M32
            self.ct -= 1
            if self.a & 0x8000:
                return

    def decode(self, cx):
        st = self.state[cx]
        qe, nmps, nlps, sw = MQ_TABLE[st]
        mps = self.mps[cx]
        self.a -= qe
        if (self.c >> 16) < qe:
            lps = self.a >= qe
            self.a = qe
        else:
            self.c -= qe << 16
            if self.a & 0x8000:
                if self.trace is not None:
                    self._count(st, cx, "mps")
                return mps
            lps = self.a < qe
        if lps:
            d = 1 - mps
            if sw:
                self.mps[cx] = d
            self.state[cx] = nlps
        else:
            d = mps
            self.state[cx] = nmps
        if self.trace is not None:
            self._count(st, cx, "lps" if lps else "mps")
        self._renorm()
        return d

    def _count(self, st, cx, what):
        self.n_state[st] = self.n_state.get(st, 0) + 1
        self.n_ctx[cx, what] = self.n_ctx.get((cx, what), 0) + 1


def t1_decode(data, w, h, orient, nplanes, passes, trace=None):
    """One code-block (Annex D): `passes` coding passes from the top plane nplanes - 1 down -> row-major signed coefficients.
    trace: "zc", "zc_ctx", "sign", "rl", "mag_ctx", "nplanes" and "block" as jpeg2000_model.t1_encode's, and the MQ decoder's."""
    mq = MQDecoder(data, trace)
    dec = mq.decode
    tr = trace
    W = w + 2
    F = [0] * ((h + 2) * W)
    mag = [0] * (w * h)
    if tr is not None:
        m.count(tr, "nplanes", nplanes)
        m.count(tr, "block", (w, h, orient))
        n_zc, n_zcx, n_mag = (tr.setdefault(key, {}) for key in ("zc", "zc_ctx", "mag_ctx"))  # the hot counters, inline

    def zc(i, kind):
        cx = zc_context(orient, *neighbours(i))
        bit = dec(cx)
        if tr is not None:
            pattern = ((F[i - W - 1] & 1) | (F[i - W] & 1) << 1 | (F[i - W + 1] & 1) << 2 | (F[i - 1] & 1) << 3 | (F[i + 1] & 1) << 4
                       | (F[i + W - 1] & 1) << 5 | (F[i + W] & 1) << 6 | (F[i + W + 1] & 1) << 7)
            n_zc[orient, pattern, kind] = n_zc.get((orient, pattern, kind), 0) + 1
            n_zcx[orient, cx, bit] = n_zcx.get((orient, cx, bit), 0) + 1
        return bit

    def neighbours(i):
        hh = (F[i - 1] & 1) + (F[i + 1] & 1)
        vv = (F[i - W] & 1) + (F[i + W] & 1)
        dd = (F[i - W - 1] & 1) + (F[i - W + 1] & 1) + (F[i + W - 1] & 1) + (F[i + W + 1] & 1)
        return hh, vv, dd

    def contribution(i):
        f = F[i]
        return 0 if not f & 1 else (-1 if f & 2 else 1)

    def sign(i):
        hc = max(-1, min(1, contribution(i - 1) + contribution(i + 1)))
        vc = max(-1, min(1, contribution(i - W) + contribution(i + W)))
        flip = 0
        if hc < 0 or (hc == 0 and vc < 0):
            hc, vc, flip = -hc, -vc, 1
        if dec(CTX_SIGN + (3 + vc if hc else vc)) ^ flip:
            F[i] |= F_NEG
        if tr is not None:
            m.count(tr, "sign", ((contribution(i - 1), contribution(i + 1), contribution(i - W), contribution(i + W)), (F[i] >> 1) & 1))
        F[i] |= F_SIG

    for k in range(passes):
        p = nplanes - 1 - (k + 2) // 3
        kind = (k + 2) % 3  # 0 significance propagation, 1 magnitude refinement, 2 cleanup
        bit = 1 << p
        for y0 in range(0, h, 4):
            for x in range(w):
                if kind == 0:
                    for y in range(y0, min(y0 + 4, h)):
                        i = (y + 1) * W + x + 1
                        if F[i] & F_SIG:
                            continue
                        hh, vv, dd = neighbours(i)
                        if hh + vv + dd == 0:
                            continue
                        if zc(i, "sp"):
                            mag[y * w + x] |= bit
                            sign(i)
                        F[i] |= F_VISIT
                elif kind == 1:
                    for y in range(y0, min(y0 + 4, h)):
                        i = (y + 1) * W + x + 1
                        f = F[i]
                        if (f & (F_SIG | F_VISIT)) != F_SIG:
                            continue
                        cx = CTX_MAG + 2 if f & F_REFINED else CTX_MAG + (1 if sum(neighbours(i)) else 0)
                        if tr is not None:
                            n_mag[cx] = n_mag.get(cx, 0) + 1
                        if dec(cx):
                            mag[y * w + x] |= bit
                        F[i] = f | F_REFINED
                else:
                    first = 0
                    if y0 + 4 <= h:
                        idx = [(y0 + j + 1) * W + x + 1 for j in range(4)]
                        if all(not F[i] & (F_SIG | F_VISIT) and sum(neighbours(i)) == 0 for i in idx):
                            if not dec(CTX_RL):
                                if tr is not None:
                                    m.count(tr, "rl", 4)
                                continue
                            r = dec(CTX_UNI) << 1
                            r |= dec(CTX_UNI)
                            if tr is not None:
                                m.count(tr, "rl", r)
                            mag[(y0 + r) * w + x] |= bit
                            sign(idx[r])
                            first = r + 1
                    for y in range(y0 + first, min(y0 + 4, h)):
                        i = (y + 1) * W + x + 1
                        if F[i] & (F_SIG | F_VISIT):
                            F[i] &= ~F_VISIT
                            continue
                        if zc(i, "cu"):
                            mag[y * w + x] |= bit
                            sign(i)
    return [-v if F[(k // w + 1) * W + k % w + 1] & F_NEG else v for k, v in enumerate(mag)]


# ---- the inverse 5/3 transform --------------------------------------------------------------------------------------

def _wrap(a):
    """two's complement modulo 2^32"""
    return ((a + (1 << 31)) & M32) - (1 << 31)


def _unlift_53(lo, hi):
    """Inverse of jpeg2000_model._lift_53 along axis 0, modulo 2^32 at every step."""
    n = lo.shape[0] + hi.shape[0]
    if n == 1:
        return lo.copy()
    nl, nh = lo.shape[0], hi.shape[0]
    k = np.arange(nl)
    even = _wrap(lo - (_wrap(_wrap(hi[np.clip(k - 1, 0, nh - 1)] + hi[np.clip(k, 0, nh - 1)]) + 2) >> 2))
    j = np.arange(nh)
    odd = _wrap(hi + (_wrap(even[j] + even[np.minimum(j + 1, nl - 1)]) >> 1))
    x = np.empty((n,) + lo.shape[1:], np.int64)
    x[0::2], x[1::2] = even, odd
    return x


def idwt_53(a, levels):
    a = a.astype(np.int64).copy()
    dims = [a.shape]
    for _ in range(levels):
        dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
    for d in range(levels, 0, -1):
        h, w = dims[d - 1]
        hl, wl = dims[d]
        t = a[:h, :w].T  # rows first: the forward transform did them last
        a[:h, :w] = _unlift_53(t[:wl], t[wl:]).T
        a[:h, :w] = _unlift_53(a[:hl, :w], a[hl:h, :w])
    return a


# ---- the file ---------------------------------------------------------------------------------------------------------

def decode(file, rows=None, cols=None, bits=16, shift=0, trace=None):
    """trace: what t1_decode collects over the file, and "levels", "precision", "passes", "zbp" and "seglen" as jpeg2000_model.encode's."""
    f = bytes(file)
    try:
        P = walk(f)
        if (rows is not None and (P["rows"], P["cols"]) != (rows, cols)) or P["precision"] > bits:
            return "CCT_E_MIXED"
        res = parse_packets(P, f)
    except Refused as e:
        return e.args[0]
    plane = np.zeros((P["rows"], P["cols"]), np.int64)
    for bands in res:
        for band in bands:
            cw, ch = 1 << P["xcb"], 1 << P["ycb"]
            for k, blk in enumerate(band["blocks"]):
                if not blk["passes"]:
                    continue
                bx, by = (k % band["ncw"]) * cw, (k // band["ncw"]) * ch
                w, h = min(cw, band["w"] - bx), min(ch, band["h"] - by)
                if trace is not None:
                    for key, item in (("passes", blk["passes"]), ("zbp", blk["zbp"]), ("seglen", len(blk["data"]))):
                        m.count(trace, key, item)
                co = t1_decode(bytes(blk["data"]), w, h, band["orient"], band["mb"] - blk["zbp"], blk["passes"], trace)
                plane[band["y0"] + by:band["y0"] + by + h, band["x0"] + bx:band["x0"] + bx + w] = np.array(co, np.int64).reshape(h, w)
    if trace is not None:
        m.count(trace, "levels", P["levels"])
        m.count(trace, "precision", P["precision"])
    x = _wrap(idwt_53(plane, P["levels"]) + (1 << (P["precision"] - 1)))
    x = np.clip(x, 0, (1 << P["precision"]) - 1) >> shift
    return x.astype(np.uint8 if bits == 8 else np.uint16)


# ---- files neither this project's encoder nor OpenJPEG writes --------------------------------------------------------------------------

def build(image, precision, levels=2, cbw=32, cbh=32, guard=2, tile_com=False, psot0=False, eoc=True, progression=0, scod=0):
    """A one-layer codestream like jpeg2000_model.encode's, with the choices that one fixes left open: code-blocks of
    cbw x cbh, `guard` guard bits (the exponents follow, so Mb stays precision + gain + 1), a COM segment in the tile-part
    header, Psot 0, no EOC, the progression byte, Scod."""
    img = np.asarray(image)
    rows, cols = img.shape
    plane = m.dwt_53(img.astype(np.int64) - (1 << (precision - 1)), levels)
    packets, exps = bytearray(), []
    for bands in resolutions(rows, cols, levels):
        pk = []
        for orient, x0, y0, w, h in bands:
            mb = 2 + precision + GAIN[orient] - 1
            exps.append(mb + 1 - guard)
            blocks = []
            for by in range(0, h, cbh):
                for bx in range(0, w, cbw):
                    blk = plane[y0 + by:y0 + min(by + cbh, h), x0 + bx:x0 + min(bx + cbw, w)]
                    nplanes = int(np.abs(blk).max()).bit_length()
                    if nplanes == 0:
                        blocks.append((0, mb, b""))
                        continue
                    data, passes = m.t1_encode(np.abs(blk).ravel().tolist(), (blk < 0).ravel().tolist(), blk.shape[1], blk.shape[0], orient, nplanes)
                    blocks.append((passes, mb - nplanes, data))
            pk.append((-(-w // cbw) if w and h else 0, -(-h // cbh) if w and h else 0, blocks, mb))
        packets += m.packet(pk)
    siz = struct.pack(">HHIIIIIIIIHBBB", 41, 0, cols, rows, 0, 0, cols, rows, 0, 0, 1, precision - 1, 1, 1)
    cod = struct.pack(">HBBHBBBBBB", 12, scod, progression, 1, 0, levels, cbw.bit_length() - 3, cbh.bit_length() - 3, 0, 1)
    qcd = struct.pack(">HB", 3 + len(exps), guard << 5) + bytes(e << 3 for e in exps)
    com = b"\xff\x64" + struct.pack(">HH", 4 + 5, 1) + b"tile!" if tile_com else b""
    psot = 0 if psot0 else 12 + len(com) + 2 + len(packets)
    return (b"\xff\x4f\xff\x51" + siz + b"\xff\x52" + cod + b"\xff\x5c" + qcd + b"\xff\x90" + struct.pack(">HHIBB", 10, 0, psot, 0, 1) + com
            + b"\xff\x93" + bytes(packets) + (b"\xff\xd9" if eoc else b""))


# ---- the file sets of the tests and of tools/debug/j2k_dec_host_emu ------------------------------------------------------

def pillow_has_jpeg2000():
    try:
        from PIL import features
        return bool(features.check_codec("jpg_2000"))
    except Exception:
        return False


def openjpeg(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG2000", **{"irreversible": False, "no_jp2": True, **kw})
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def base_rasters():
    """70 x 130 uint16 with structure plus noise, and an 8-bit raster of the same shape"""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:70, 0:130]
    base = ((yy * 37 + xx * 91) % 4096 * 8 + 20000 * ((yy - 30) ** 2 + (xx - 60) ** 2 < 500) + rng.integers(0, 300, (70, 130))).astype(np.uint16)
    return base, (base >> 8).astype(np.uint8)


FOREIGN = (("defaults", {}), ("3 resolutions, 16 x 64", dict(num_resolutions=3, codeblock_size=(16, 64))),
           ("2 resolutions, 4 x 4", dict(num_resolutions=2, codeblock_size=(4, 4))),
           ("three layers by rate", dict(quality_mode="rates", quality_layers=[40, 10, 0])),
           ("three layers by rate, RLCP", dict(quality_mode="rates", quality_layers=[40, 10, 0], progression="RLCP")),
           ("three layers by dB", dict(quality_mode="dB", quality_layers=[30, 40, 0])),
           ("RPCL", dict(progression="RPCL")), ("PCRL", dict(progression="PCRL")), ("CPRL", dict(progression="CPRL")),
           ("PLT and COM", dict(plt=True, comment="hello")), ("JP2", dict(no_jp2=False)))


@functools.lru_cache(maxsize=None)
def foreign_set():
    """OpenJPEG's own files, written through Pillow: [(name, file, the raster Pillow decodes it to)].  Needs Pillow's codec."""
    from PIL import Image
    base, low = base_rasters()
    files = [(name, openjpeg(base, **kw)) for name, kw in FOREIGN] + [("8 bits", openjpeg(low))]
    return [(name, f, np.array(Image.open(io.BytesIO(f)))) for name, f in files]


@functools.lru_cache(maxsize=None)
def refused_set():
    """[(name, file)], each CCT_E_J2K; all but the last need Pillow's codec"""
    base, low = base_rasters()
    out = []
    if pillow_has_jpeg2000():
        out = [("precincts", openjpeg(base, precinct_size=(32, 32))), ("9/7", openjpeg(base, irreversible=True)),
               ("tiles", openjpeg(base, tile_size=(64, 64))), ("RGB", openjpeg(np.stack([low, low, low], axis=2)))]
    return out + [("SOP", build(base, 16, scod=2))]


@functools.lru_cache(maxsize=None)
def handbuilt_set():
    """[(name, file, raster)] of build()'s files, 33 x 65 at 16 bits (the last one at 12)"""
    img = np.ascontiguousarray(base_rasters()[0][:33, :65])
    out = [(name, build(img, 16, **kw), img) for name, kw in (
        ("one guard bit", dict(guard=1)), ("COM in the tile-part header", dict(tile_com=True)), ("Psot 0", dict(psot0=True)), ("no EOC", dict(eoc=False)),
        ("8 x 64 code-blocks, one level, RPCL", dict(cbw=8, cbh=64, levels=1, progression=2)))]
    low = img >> 4
    return out + [("12 bits, three guard bits, Psot 0 and no EOC", build(low, 12, guard=3, psot0=True, eoc=False), low)]


# The damages: (what, packet or None, offset, operation).  "cut" truncates the file at the position, anything else changes the
# byte there: ("xor", v), ("set", v).  Positions: an absolute offset (packet None), or relative to a packet's header start
# ("hdr"), header end = first body byte ("body") or end ("end") of that packet, as parse_packets traces them.
DAMAGES = (
    ("cut", None, 0, None), ("cut", None, 2, None), ("cut", None, 20, None), ("cut", None, "siz", None), ("cut", None, "cod", None),
    ("cut", None, "qcd", None), ("cut", None, "sot", None), ("cut", None, "sod", None), ("cut", 0, "hdr", 1), ("cut", 0, "body", 0),
    ("cut", 0, "end", 0), ("cut", 1, "hdr", 1), ("cut", 1, "body", 0), ("cut", 1, "body", 5), ("cut", 2, "hdr", 2), ("cut", 2, "end", 0),
    ("cut", -1, "hdr", 0), ("cut", -1, "end", 0), ("cut", -1, "end", 1),
    ("xor", 0, "hdr", (0, 0x80)), ("xor", 0, "hdr", (0, 0x40)), ("xor", 0, "hdr", (0, 0x01)), ("xor", 0, "hdr", (1, 0x10)), ("set", 0, "hdr", (1, 0xFF)),
    ("xor", 1, "hdr", (0, 0x20)), ("xor", 1, "hdr", (1, 0x08)), ("xor", 1, "hdr", (2, 0x80)), ("set", 1, "hdr", (0, 0xFF)), ("set", 1, "hdr", (2, 0x00)),
    ("xor", 2, "hdr", (0, 0x04)), ("xor", 2, "hdr", (1, 0x01)), ("xor", -1, "hdr", (0, 0x80)), ("xor", -1, "hdr", (1, 0x02)), ("set", -1, "hdr", (1, 0xFF)),
    ("xor", 0, "body", (0, 0x80)), ("xor", 0, "body", (3, 0x55)), ("set", 0, "body", (1, 0xFF)), ("xor", 1, "body", (0, 0x01)), ("set", 1, "body", (7, 0xFF)),
    ("set", 1, "body", (8, 0xFF)), ("xor", 2, "body", (40, 0xFF)), ("xor", -1, "body", (2, 0x10)), ("xor", -1, "end", (-1, 0x01)), ("set", -1, "end", (-1, 0xFF)),
)


def damaged(file):
    """[(the damage, the damaged file)] over DAMAGES; a position outside the file is clamped into it"""
    f = bytes(file)
    P = walk(f)
    trace = []
    parse_packets(P, f, trace)
    marks = {"siz": f.index(b"\xff\x52"), "cod": f.index(b"\xff\x5c"), "qcd": f.index(b"\xff\x90"), "sot": f.index(b"\xff\x90") + 12, "sod": P["data0"]}
    out = []
    for what, pk, where, arg in DAMAGES:
        if pk is None:
            pos, off, v = marks.get(where, where), 0, None
        else:
            pos = trace[pk][{"hdr": 0, "body": 1, "end": 2}[where]]
            off, v = (arg, None) if what == "cut" else arg
        pos = max(0, min(pos + off, len(f) - 1))
        if what == "cut":
            out.append(((what, pk, where, arg), f[:pos]))
        else:
            out.append(((what, pk, where, arg), f[:pos] + bytes([f[pos] ^ v if what == "xor" else v]) + f[pos + 1:]))
    return out


@functools.lru_cache(maxsize=None)
def damaged_set():
    """[(base name, damage, file, rows, cols)]: DAMAGES on a 33 x 65 file of the encoder model (32 x 32 code-blocks, 2 levels) and,
    with Pillow's codec, on a three-layer file of OpenJPEG's of the same raster (small, so that the model stays quick)"""
    img = np.ascontiguousarray(base_rasters()[0][:33, :65])
    bases = [("model 33 x 65", m.encode(img, 16, 0, 2, 32))]
    if pillow_has_jpeg2000():
        bases.append(("OpenJPEG three layers", openjpeg(img, num_resolutions=3, codeblock_size=(32, 32), quality_mode="rates", quality_layers=[40, 10, 0])))
    return [(name, dmg, g, 33, 65) for name, f in bases for dmg, g in damaged(f)]


@functools.lru_cache(maxsize=None)
def damaged_expected(base):
    """[(damage, file, status name or raster)] of one base of damaged_set(), the model run once"""
    return [(dmg, g, decode(g, rows, cols)) for name, dmg, g, rows, cols in damaged_set() if name == base]


@functools.lru_cache(maxsize=None)
def marker_cases():
    """(a 9 x 11 raster, [(name, file, "OK" / the status name)]): a file of build() with one marker segment changed at a time, every
    line of the list of refusals that no file above reaches, and what is taken next to them"""
    img = np.ascontiguousarray(base_rasters()[0][:9, :11])
    f = build(img, 16, levels=1)
    cod, qcd, sot = f.index(b"\xff\x52"), f.index(b"\xff\x5c"), f.index(b"\xff\x90")

    def put(at, *vals):
        return f[:at] + bytes(vals) + f[at + len(vals):]
    # SIZ: marker 2, Lsiz 4, Rsiz 6, Xsiz 8, Ysiz 12, XOsiz 16, YOsiz 20, XTsiz 24, YTsiz 28, XTOsiz 32, YTOsiz 36, Csiz 40, Ssiz 42, XRsiz 43
    refused = (
        ("EPH", put(cod + 4, 4)), ("precincts", put(cod + 4, 1)), ("progression 5", put(cod + 5, 5)), ("0 layers", put(cod + 6, 0, 0)),
        ("33 layers", put(cod + 6, 0, 33)), ("MCT", put(cod + 8, 1)), ("9 levels", put(cod + 9, 9)), ("128 wide", put(cod + 10, 5)),
        ("bypass", put(cod + 12, 1)), ("9/7", put(cod + 13, 0)), ("scalar derived", put(qcd + 4, (2 << 5) | 1)), ("scalar expounded", put(qcd + 4, (2 << 5) | 2)),
        ("too few exponents", f[:qcd + 2] + bytes([0, 3 + 3]) + f[qcd + 4:qcd + 4 + 4] + f[sot:]), ("20 bit-planes", put(qcd + 7, 19 << 3)),
        ("no QCD", f[:qcd] + f[sot:]), ("no COD", f[:cod] + f[qcd:]), ("COC", f[:sot] + b"\xff\x53\x00\x09" + bytes(7) + f[sot:]),
        ("QCC", f[:sot] + b"\xff\x5d\x00\x05\x00\x40\x80" + f[sot:]), ("RGN", f[:sot] + b"\xff\x5e\x00\x05\x00\x00\x01" + f[sot:]),
        ("POC", f[:sot] + b"\xff\x5f\x00\x09" + bytes(7) + f[sot:]), ("PPM", f[:sot] + b"\xff\x60\x00\x03\x00" + f[sot:]),
        ("PPT", f[:sot + 12] + b"\xff\x61\x00\x03\x00" + f[sot + 12:]), ("tile 1", put(sot + 5, 1)), ("tile-part 1", put(sot + 10, 1)),
        ("two tile-parts", put(sot + 11, 2)), ("segment leaves the file", put(qcd + 2, 0xFF, 0xFF)), ("no SOT", f[:sot] + f[sot + 12:]),
        ("no SOD", f[:sot + 12] + f[sot + 14:]), ("signed", put(42, 0x8F)), ("1 bit", put(42, 0)), ("image origin", put(17, 1)),
        ("tile origin", put(33, 1)), ("tiles", put(24, 0, 0, 0, 8)), ("subsampling", put(43, 2)), ("Psot ends before SOD", put(sot + 6, 0, 0, 0, 5)))
    taken = (("as built", f), ("TNsot 0", put(sot + 11, 0)), ("TLM", f[:sot] + b"\xff\x55\x00\x06\x00\x00\x00\x00" + f[sot:]),
             ("CRG", f[:sot] + b"\xff\x63\x00\x06\x00\x00\x00\x00" + f[sot:]), ("bytes behind EOC", f + b"trailer"),
             ("a larger tile", put(24, 0, 1, 0, 0, 0, 1, 0, 0)))
    return img, ([(n, g, "CCT_E_J2K") for n, g in refused] + [(n, g, "OK") for n, g in taken]
                 + [("Psot ends right behind SOD", put(sot + 6, 0, 0, 0, 15), "CCT_E_STREAM")])
