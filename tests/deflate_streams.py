"""DEFLATE streams built by hand for the device INFLATE (inflate_kernels.hip): a writer that optimises nothing (every code
length, every code-length symbol, every LEN/NLEN and header field is the caller's), a small reference walk of a stream (bit
offset, code length, kind, output offset, copy length and distance of every symbol), the kernel's geometry as constants, and
the named case list that tests/test_deflate_streams_host.py (CPython's zlib judges every stream, every precondition is
asserted) and tests/test_gpu_deflate_streams.py (the device reads every stream) share.  Streams zlib's deflate never
writes: headers longer than the code-length window, codes longer than the root tables, rounds cut by the copy list, the lane
cap and the output budget, zlib's exact verdicts on code sets.  Test infrastructure only: the product never imports it.
Pure Python + numpy + zlib (Adler-32)."""
import collections
import functools
import zlib

import numpy as np

# ---- the kernel's geometry (tests/test_deflate_streams_host.py reads the same names out of inflate_kernels.hip) ---------
SEG_BITS = 256
LL_BITS = 12
D_BITS = 10
CL_WIN = 2048
MLIST_CAP = 2048
LANE_OUT_CAP = 16384
INF_RING = 65536
ROUND_OUT_BUDGET = {256: 24576, 512: 28672}
LANES = (256, 512)

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
BL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
EOB = 256


# ---- writer -------------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n, self.nbits = bytearray(), 0, 0, 0

    def put(self, value, nbits):
        """nbits of value, least significant bit first (header fields, extra bits)"""
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        self.nbits += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        """a Huffman code: most significant bit first"""
        self.put(int(format(code, f"0{nbits}b")[::-1], 2) if nbits else 0, nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """RFC 1951 3.2.2: {symbol: (code, length)}.  For a set that is no prefix code the values are what the rule gives."""
    count = collections.Counter(ln for ln in lengths if ln)
    code, nxt = 0, {}
    for b in range(1, 16):
        code = (code + count.get(b - 1, 0)) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln] & ((1 << ln) - 1), ln)
            nxt[ln] += 1
    return out


def length_symbol(length):
    if length == 258:
        return 285, 0, 0
    s = max(k for k in range(28) if LBASE[k] <= length)
    return 257 + s, LEXTRA[s], length - LBASE[s]


def distance_symbol(dist):
    s = max(k for k in range(30) if DBASE[k] <= dist)
    return s, DEXTRA[s], dist - DBASE[s]


def balanced(used, n):
    """a complete prefix code on the symbols `used` (two at least) of an alphabet of n: lengths differing by at most one"""
    used = sorted(used)
    k = len(used)
    assert k >= 2
    m = (k - 1).bit_length()
    short = (1 << m) - k
    lens = [0] * n
    for i, s in enumerate(used):
        lens[s] = m - 1 if i < short else m
    return lens


def rle(lens):
    """a plain run-length coding of a code-length list: 18 / 17 for zeros, 16 after a value, nothing clever"""
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        run = j - i
        if lens[i] == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r))
                run -= r
            if run >= 3:
                out.append((17, run))
                run = 0
        else:
            out.append(lens[i])
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r))
                run -= r
        out += [lens[i]] * run
        i = j
    return out


def cl_code_for(seq):
    """a complete code-length code (19 lengths) on the symbols a sequence uses"""
    used = {s if isinstance(s, int) else s[0] for s in seq}
    while len(used) < 2:
        used.add(min(set(range(19)) - used))
    return balanced(used, 19)


def stored(data=b"", final=False, len_field=None, nlen_field=None):
    ln = len(data) if len_field is None else len_field
    return dict(type=0, data=bytes(data), final=final, len=ln, nlen=(ln ^ 0xFFFF) if nlen_field is None else nlen_field)


def fixed(body=(), final=False, eob=True):
    return dict(type=1, body=list(body), final=final, eob=eob)


def dynamic(ll_lens, d_lens, body=(), final=False, eob=True, cl_seq=None, cl_lens=None, hclen=None, hlit=None, hdist=None):
    """ll_lens / d_lens: the code lengths the BODY is written with.  cl_seq: the code-length symbols of the header: an int
    0..15 is that length once, (16, n) repeats the previous one n times, (17, n) and (18, n) are n zeros; the default writes
    rle(ll_lens + d_lens).  cl_lens: the 19 code-length-code lengths (default: a complete code on what cl_seq uses); hclen:
    how many of them are written; hlit / hdist: the 5-bit header fields (default: from the lengths)."""
    ll_lens, d_lens = list(ll_lens), list(d_lens)
    if cl_seq is None:
        cl_seq = rle(ll_lens + d_lens)
    if cl_lens is None:
        cl_lens = cl_code_for(cl_seq)
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if cl_lens[BL_ORDER[i]]])
    return dict(type=2, ll=ll_lens, d=d_lens, body=list(body), final=final, eob=eob, cl_seq=list(cl_seq), cl_lens=list(cl_lens),
                hclen=hclen, hlit=len(ll_lens) - 257 if hlit is None else hlit, hdist=len(d_lens) - 1 if hdist is None else hdist)


def raw_bits(fields, final=False):
    """a block that is only the given (value, nbits) fields after BFINAL (block type 3, a cut header, ...)"""
    return dict(type="raw", fields=list(fields), final=final)


def copy(length, dist):
    return ("m", length, dist)


def _body(w, body, ll, d, eob):
    llc, dc = canonical(ll), canonical(d)
    for it in body:
        if isinstance(it, (int, np.integer)):
            w.code(*llc[int(it)])
        elif it[0] == "m":
            s, xb, xv = length_symbol(it[1])
            w.code(*llc[s])
            w.put(xv, xb)
            s, xb, xv = distance_symbol(it[2])
            w.code(*dc[s])
            w.put(xv, xb)
        elif it[0] == "ld":  # literal/length symbol, extra value, distance symbol, extra value: as they are
            _, ls, lx, ds, dx = it
            w.code(*llc[ls])
            w.put(lx, LEXTRA[ls - 257] if ls - 257 < 29 else 0)
            w.code(*dc[ds])
            w.put(dx, DEXTRA[ds] if ds < 30 else 0)
        elif it[0] == "ll":  # one literal/length symbol alone (286, 287, an early end-of-block)
            w.code(*llc[it[1]])
        else:  # ("raw", code, nbits): a code of no symbol
            assert it[0] == "raw"
            w.code(it[1], it[2])
    if eob:
        w.code(*llc[EOB])


def deflate_raw(blocks, w=None):
    w = w or BitWriter()
    for b in blocks:
        w.put(1 if b["final"] else 0, 1)
        if b["type"] == "raw":
            for v, n in b["fields"]:
                w.put(v, n)
        elif b["type"] == 0:
            w.put(0, 2)
            w.align()
            w.put(b["len"], 16)
            w.put(b["nlen"], 16)
            for x in b["data"]:
                w.put(x, 8)
        elif b["type"] == 1:
            w.put(1, 2)
            _body(w, b["body"], FIXED_LL, FIXED_D, b["eob"])
        else:
            w.put(2, 2)
            w.put(b["hlit"], 5)
            w.put(b["hdist"], 5)
            w.put(b["hclen"] - 4, 4)
            for i in range(b["hclen"]):
                w.put(b["cl_lens"][BL_ORDER[i]], 3)
            clc = canonical(b["cl_lens"])
            for s in b["cl_seq"]:
                if isinstance(s, int):
                    w.code(*clc[s])
                else:
                    sym, n = s
                    w.code(*clc[sym])
                    w.put(n - (11 if sym == 18 else 3), 7 if sym == 18 else 3 if sym == 17 else 2)
            _body(w, b["body"], b["ll"], b["d"], b["eob"])
    return w.bytes()


def expand(blocks):
    """the bytes a list of well-formed blocks means (the writer's own model; zlib is the judge)"""
    out = bytearray()
    for b in blocks:
        if b["type"] == 0:
            out += b["data"]
        else:
            for it in b["body"]:
                if isinstance(it, (int, np.integer)):
                    out.append(int(it))
                else:
                    assert it[0] == "m" and 1 <= it[2] <= len(out)
                    for _ in range(it[1]):
                        out.append(out[-it[2]])
    return bytes(out)


def zlib_stream(blocks, data=None, cmf=0x78, flg=None, adler=None):
    """header + raw DEFLATE + Adler-32 of `data` (default: what the blocks expand to); every field can be overridden"""
    if flg is None:
        flg = 0x80
        flg += 31 - ((cmf << 8) | flg) % 31
    if adler is None:
        adler = zlib.adler32(expand(blocks) if data is None else data)
    return bytes([cmf, flg]) + deflate_raw(blocks) + adler.to_bytes(4, "big")


# ---- reference walk -----------------------------------------------------------------------------------------------------
Sym = collections.namedtuple("Sym", "bit nbits kind out length dist dbits")  # nbits / dbits: CODE lengths without extra bits
ClSym = collections.namedtuple("ClSym", "bit sym nbits entries")            # bit: relative to the first one; nbits with extra bits


class Truncated(Exception):
    pass


class _Bits:
    def __init__(self, data, pos=0):
        self.d, self.pos, self.end = bytes(data) + bytes(8), pos, 8 * len(data)

    def get(self, k):
        i = self.pos >> 3
        x = int.from_bytes(self.d[i:i + 4], "little") >> (self.pos & 7)
        self.pos += k
        if self.pos > self.end:  # a read past the last byte ends the walk
            raise Truncated
        return x & ((1 << k) - 1)


def _decoder(lengths):
    return {(ln, code): s for s, (code, ln) in canonical(lengths).items()}


def _sym(bits, table):
    code = 0
    for ln in range(1, 16):
        code = (code << 1) | bits.get(1)
        if (ln, code) in table:
            return table[(ln, code)], ln
    return None, 0


def code_set(lengths, codes_type=False):
    """zlib's verdict on a set of code lengths (inflate_table): "over", "incomplete" or None.  An incomplete set passes only as
    the single one-bit code, or, outside the code-length alphabet, as no code at all."""
    left, mx = 1, 0
    for ln in range(1, 16):
        n = sum(1 for x in lengths if x == ln)
        left = 2 * left - n
        if left < 0:
            return "over"
        if n:
            mx = ln
    if left > 0 and mx and (codes_type or mx != 1):
        return "incomplete"
    if codes_type and mx == 0:
        return "incomplete"
    return None


class _Stop(Exception):
    pass


def walk(stream):
    """A small INFLATE that reports instead of optimising.  -> {"blocks": [...], "out": bytes, "error": None or the name of what
    stops zlib, "error_bit": where}.  A block: type, start (bit offset of BFINAL in the stream), body (bit offset of the first
    symbol), header_bits = body - start, end (bit after end-of-block), cl (the code-length symbols of a dynamic header), syms."""
    bits = _Bits(stream, 0)
    out, blocks, res = bytearray(), [], {"error": None, "error_bit": None}

    def stop(what):
        res["error"] = what
        raise _Stop

    try:
        cmf, flg = bits.get(8), bits.get(8)
        if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 or flg & 0x20:
            stop("zlib header")
        while True:
            blk = {"start": bits.pos, "cl": [], "syms": []}
            blocks.append(blk)
            final, btype = bits.get(1), bits.get(2)
            blk["type"] = btype
            if btype == 3:
                stop("block type 3")
            if btype == 0:
                bits.pos = (bits.pos + 7) & ~7
                n, nn = bits.get(16), bits.get(16)
                blk["body"], blk["out"] = bits.pos, len(out)
                if n ^ 0xFFFF != nn:
                    stop("stored lengths")
                if bits.pos + 8 * n > bits.end:
                    raise Truncated
                out += bits.d[bits.pos >> 3:(bits.pos >> 3) + n]
                bits.pos += 8 * n
            else:
                if btype == 1:
                    ll, d = FIXED_LL, FIXED_D
                else:
                    hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                    blk["hlit"], blk["hdist"], blk["hclen"] = hlit, hdist, hclen
                    if hlit > 286 or hdist > 30:
                        stop("too many symbols")
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[BL_ORDER[i]] = bits.get(3)
                    if code_set(cl, True):
                        stop("code-length set " + code_set(cl, True))
                    ct, lens, b0 = _decoder(cl), [], bits.pos
                    while len(lens) < hlit + hdist:
                        at = bits.pos
                        s, _ = _sym(bits, ct)
                        if s < 16:
                            new = [s]
                        elif s == 16:
                            if not lens:
                                stop("repeat with nothing before it")
                            new = [lens[-1]] * (3 + bits.get(2))
                        else:
                            new = [0] * (3 + bits.get(3) if s == 17 else 11 + bits.get(7))
                        blk["cl"].append(ClSym(at - b0, s, bits.pos - at, len(new)))
                        lens += new
                        if len(lens) > hlit + hdist:
                            stop("repeat past the last entry")
                    blk["lens"] = lens
                    ll, d = lens[:hlit], lens[hlit:]
                    if ll[256] == 0:
                        stop("no end-of-block code")
                    if code_set(ll):
                        stop("literal/length set " + code_set(ll))
                    if code_set(d):
                        stop("distance set " + code_set(d))
                lt, dt = _decoder(ll), _decoder(d)
                blk["body"] = bits.pos
                while True:
                    at = bits.pos
                    res["error_bit"] = at
                    s, ln = _sym(bits, lt)
                    if s is None or s > 285:
                        stop("literal/length code")
                    if s < 256:
                        blk["syms"].append(Sym(at, ln, "lit", len(out), 1, 0, 0))
                        out.append(s)
                        continue
                    if s == 256:
                        blk["syms"].append(Sym(at, ln, "eob", len(out), 0, 0, 0))
                        break
                    length = LBASE[s - 257] + bits.get(LEXTRA[s - 257])
                    ds, dl = _sym(bits, dt)
                    if ds is None or ds > 29:
                        stop("distance code")
                    dist = DBASE[ds] + bits.get(DEXTRA[ds])
                    blk["syms"].append(Sym(at, ln, "len", len(out), length, dist, dl))
                    if dist > len(out):
                        stop("distance too far back")
                    for _ in range(length):
                        out.append(out[-dist])
                res["error_bit"] = None
            blk["end"] = bits.pos
            blk["header_bits"] = blk["body"] - blk["start"]
            if final:
                break
        bits.pos = (bits.pos + 7) & ~7
        res["trailer"] = bits.pos
        if int.from_bytes(bytes(bits.get(8) for _ in range(4)), "big") != zlib.adler32(bytes(out)):
            stop("adler")
    except _Stop:
        pass
    except Truncated:
        res["error"] = "truncated"
    if res["error"] and res["error_bit"] is None:
        res["error_bit"] = bits.pos
    res["blocks"], res["out"], res["end_bit"] = blocks, bytes(out), bits.pos
    return res


def cl_windows(cl):
    """indices of the code-length symbols that open a window of cl_sequence: the first symbol, then every first symbol at or
    after CL_WIN bits from the window's start"""
    opens, w0 = [0], 0
    for k, c in enumerate(cl):
        if c.bit - w0 >= CL_WIN:
            opens.append(k)
            w0 = c.bit
    return opens


def first_round(blk, nt):
    """The lanes of the first round of a block's body: lane t holds the symbols that start in [body + t * SEG_BITS,
    body + (t + 1) * SEG_BITS).  -> [(output bytes, copies)] per lane, up to the lane with the end-of-block"""
    lanes = [[0, 0] for _ in range(nt)]
    for s in blk["syms"]:
        t = (s.bit - blk["body"]) // SEG_BITS
        if t >= nt:
            break
        lanes[t][0] += s.length
        lanes[t][1] += s.kind == "len"
    return [tuple(x) for x in lanes]


def round_cut(blk, nt):
    """what ends the first round of the block: ("mlist" | "budget" | "lane" | None, lane index).  Models inflate_kernel's round
    loop: the prefix sums cb / cm over the lanes and `over = first_lane_with(tid > 0 && (cb > ROUND_OUT_BUDGET || cm > MLIST_CAP))`
    keep the lanes before the first one that exceeds either (lane 0 always stays), and walk_segment's
    `if (nbytes >= LANE_OUT_CAP) flags = SEG_CUT` makes a lane end the round itself: it tests before every general step, so a
    lane whose symbols give a copy (258) and three literal pairs (6) more than the cap certainly meets it.
    tests/test_deflate_streams_host.py checks that the kernel source still states both rules."""
    cb = cm = 0
    for t, (nb, nm) in enumerate(first_round(blk, nt)):
        if nb >= LANE_OUT_CAP + 258 + 6:  # the lane certainly sees the cap before its segment ends
            return "lane", t
        cb, cm = cb + nb, cm + nm
        if t and cm > MLIST_CAP:
            return "mlist", t
        if t and cb > ROUND_OUT_BUDGET[nt]:
            return "budget", t
    return None, nt


def round_copies(blk, nt):
    """the copies of the first round of the block, as the copy list holds them"""
    _, cut = round_cut(blk, nt)
    return [s for s in blk["syms"] if s.kind == "len" and (s.bit - blk["body"]) // SEG_BITS < cut]


def chained(a, b):
    """copy b continues the periodic chain of copy a (the kernel's `head` walk)"""
    return a.dist == b.dist and a.dist < a.length and b.dist < b.length and a.out + a.length == b.out


# ---- cases ----------------------------------------------------------------------------------------------------------------
E_ZLIB, E_CAP = 2, 6  # CCT_E_ZLIB, CCT_E_CAP (include/compact_hip.h)
Case = collections.namedtuple("Case", "name group accept stream pre")
# group: "accept", "refuse" or "truncate" (the order the device tests run in); accept: zlib's verdict; pre(walk) asserts, from the
# walk alone, that the stream reaches what its name says, and may return a line for the test's output

_CASES = []


def case(name, group="accept"):
    def reg(fn):
        @functools.lru_cache(maxsize=None)
        def build():
            stream, pre = fn()
            return Case(name, group, group == "accept", stream, pre)
        _CASES.append((name, build))
        return build
    return reg


def _stops(what, block=0, where=None):
    """precondition of a refused stream: the walk stops for this reason, in this block, and (where = "body") after the header"""
    def pre(w):
        assert w["error"] == what, w["error"]
        assert len(w["blocks"]) == block + 1
        if where == "body":
            assert "body" in w["blocks"][block]
        return f"stops at bit {w['error_bit']}: {what}"
    return pre


def _accepted(check=None):
    def pre(w):
        assert w["error"] is None
        return check(w) if check else None
    return pre


def _rng(seed):
    return np.random.default_rng(seed)


# -- headers
LONG_LL = [8] * 226 + [9] * 60      # 2 * 226 + 60 = 512: complete
LONG_D = [4] * 2 + [5] * 28         # 2 * 2 + 28 = 32: complete
# sixteen 7-bit codes for the lengths 0..15 (16 / 128) + 16, 17, 18 on 3, 2, 1 bits (1/8 + 1/4 + 1/2): complete
LONG_CL = [7] * 16 + [3, 2, 1]


def long_header_block(payload, final=True, cl_seq=None):
    """a dynamic block with all 286 + 30 code lengths written one by one on 7-bit codes (2212 bits of sequence); every byte has a
    code, so the body is any payload as literals"""
    return dynamic(LONG_LL, LONG_D, list(payload), final=final, cl_seq=cl_seq or LONG_LL + LONG_D, cl_lens=LONG_CL)


def long_header_16_block(payload, final=True):
    seq = LONG_LL + LONG_D
    k = 293  # 293 * 7 = 2051: the first symbol at or after bit 2048; entries 292 .. 295 are all 5
    assert seq[k - 1:k + 3] == [5] * 4
    seq[k:k + 3] = [(16, 3)]
    return long_header_block(payload, final, seq)


def pre_long_header(w, second_opens_with=None):
    assert w["error"] is None
    cl = w["blocks"][0]["cl"]
    assert cl[-1].bit + cl[-1].nbits > CL_WIN
    opens = cl_windows(cl)
    assert len(opens) == 2 and cl[opens[1]].bit >= CL_WIN
    if second_opens_with is not None:
        assert cl[opens[1]].sym == second_opens_with and cl[opens[1] - 1].sym < 16  # its source is the first window's last entry
    return f"sequence of {cl[-1].bit + cl[-1].nbits} bits, windows open at symbols {opens}"


_LONG_PAYLOAD = bytes(_rng(1).integers(0, 256, 700, dtype=np.uint8)) + bytes(range(256))


@case("header_longer_than_cl_win")
def _():
    return zlib_stream([long_header_block(_LONG_PAYLOAD)]), pre_long_header


@case("header_16_opens_second_window")
def _():
    return zlib_stream([long_header_16_block(_LONG_PAYLOAD)]), lambda w: pre_long_header(w, second_opens_with=16)


@case("header_16_run_across_ll_d_boundary")
def _():
    # the boundary cannot lie in a second window: 285 entries of at most 7 bits end before bit 2048
    ll = [0] * 258
    for s in (97, 98, 256, 257):
        ll[s] = 2
    seq = rle(ll[:256]) + [2, (16, 5)]  # entry 256, then 257 and the four distance entries
    blocks = [dynamic(ll, [2, 2, 2, 2], list(b"abba") + [copy(3, 1), copy(3, 2), copy(3, 3), copy(3, 4)], final=True, cl_seq=seq)]

    def pre(w):
        cl, at = w["blocks"][0]["cl"], 0
        for c in cl:
            if c.sym == 16:
                assert at < 258 < at + c.entries
            at += c.entries
        assert w["error"] is None and cl[-1].sym == 16 and at == 262
    return zlib_stream(blocks), pre


@case("header_18_with_138_zeros")
def _():
    ll = [0] * 257
    ll[0], ll[139], ll[256] = 1, 2, 2
    seq = [1, (18, 138), 2, (18, 116), 2, 0]
    blocks = [dynamic(ll, [0], [0, 139, 139, 0], final=True, cl_seq=seq)]

    def pre(w):
        assert w["error"] is None and any(c.sym == 18 and c.entries == 138 for c in w["blocks"][0]["cl"])
    return zlib_stream(blocks), pre


@case("refused_hclen_4_names_only_zero_lengths", "refuse")
def _():
    # HCLEN = 4 gives codes to 16, 17, 18 and 0 only: every length such a header can write is 0, so no stream with HCLEN = 4 is
    # accepted: the whole sequence is read and the block is refused for its missing end-of-block code.  HCLEN = 5 (below) is
    # the smallest that can be accepted.
    cl = [0] * 19
    cl[18], cl[0] = 1, 1
    b = dynamic([0] * 257, [0], [], final=True, eob=False, cl_seq=[(18, 138), (18, 119), 0], cl_lens=cl, hclen=4)

    def pre(w):
        assert w["blocks"][0]["hclen"] == 4
        return _stops("no end-of-block code")(w)
    return zlib_stream([b], data=b""), pre


@case("header_hclen_5")
def _():
    # 16, 17, 18, 0, 8: the literals 0..254 and end-of-block on 8 bits each are a complete set
    cl = [0] * 19
    cl[0], cl[8] = 1, 1
    ll = [8] * 255 + [0, 8]
    b = dynamic(ll, [0], list(bytes(range(255))) + [7, 7, 254], final=True, cl_seq=ll + [0], cl_lens=cl)
    return zlib_stream([b]), _accepted(lambda w: w["blocks"][0]["hclen"] == 5 or 1 / 0)


def _hl_case(nll, nd):
    @case(f"header_hlit_{nll}_hdist_{nd}")
    def _():
        # HLIT 257 names no length symbol, so its distance set is read and never used; 286 / 30 use their last symbols
        ll = balanced([0, 1, 2, 256] + ([285] if nll == 286 else []), nll)
        d = balanced(list(range(nd)), nd) if nd > 1 else [1]
        body = [0, 1, 2, 2, 1, 0] * 12
        if nll == 286:
            body += [copy(258, 1)] * (96 if nd == 30 else 2) + ([copy(258, DBASE[29]), copy(258, 24700)] if nd == 30 else []) + [2]
        b = dynamic(ll, d, body, final=True)

        def pre(w):
            blk = w["blocks"][0]
            assert w["error"] is None and (blk["hlit"], blk["hdist"]) == (nll, nd)
            if nll == 286:
                assert any(s.length == 258 for s in blk["syms"])
                assert nd == 1 or any(s.dist >= DBASE[29] for s in blk["syms"])
        return zlib_stream([b]), pre


for _nll, _nd in ((257, 1), (286, 30), (257, 30), (286, 1)):
    _hl_case(_nll, _nd)

_SMALL_LL = balanced([97, 98, 256, 257], 258)   # a, b, end-of-block, length 3: two bits each
_SMALL_BODY = list(b"abab") + [copy(3, 2), copy(3, 1)]


def _refused_header(name, why, where=None, **kw):
    @case(name, "refuse")
    def _():
        args = dict(ll_lens=_SMALL_LL, d_lens=[1, 1], body=_SMALL_BODY, final=True)
        args.update(kw)
        return zlib_stream([dynamic(**args)], data=b"abab"), _stops(why, where=where)


_refused_header("refused_16_as_first_entry", "repeat with nothing before it", cl_seq=[(16, 3)] + rle(_SMALL_LL[3:] + [1, 1]),
                cl_lens=cl_code_for([16, 17, 18, 2, 1, 0]))
_refused_header("refused_repeat_past_hlit_hdist", "repeat past the last entry", cl_seq=rle(_SMALL_LL) + [1, (16, 3)])
_refused_header("refused_zero_run_past_hlit_hdist", "repeat past the last entry", cl_seq=rle(_SMALL_LL) + [1, (17, 3)])
for _f in (30, 31):
    _refused_header(f"refused_hlit_field_{_f}", "too many symbols", hlit=_f, cl_seq=rle(_SMALL_LL + [0] * (_f - 1) + [1, 1]))
    _refused_header(f"refused_hdist_field_{_f}", "too many symbols", hdist=_f, cl_seq=rle(_SMALL_LL + [1, 1] + [0] * (_f - 1)))
_refused_header("refused_no_eob_code", "no end-of-block code", ll_lens=balanced([97, 98, 99, 257], 258), body=list(b"abc"), eob=False)
_refused_header("refused_ll_oversubscribed", "literal/length set over", ll_lens=[2 if s in (97, 98, 99, 256, 257) else 0 for s in range(258)])
_refused_header("refused_ll_incomplete", "literal/length set incomplete", ll_lens=[2 if s in (97, 256, 257) else 0 for s in range(258)],
                body=[97, 97])
_refused_header("refused_d_oversubscribed", "distance set over", d_lens=[1, 1, 1])
_refused_header("refused_d_incomplete", "distance set incomplete", d_lens=[1, 2])
_refused_header("refused_cl_oversubscribed", "code-length set over", cl_seq=_SMALL_LL + [1, 1], cl_lens=[1, 1, 1] + [0] * 16)
_refused_header("refused_cl_incomplete", "code-length set incomplete", cl_seq=_SMALL_LL + [1, 1], cl_lens=[2, 2, 2] + [0] * 16)
_refused_header("refused_cl_single_one_bit_code", "code-length set incomplete", ll_lens=[0] * 257, d_lens=[0], body=[], eob=False,
                cl_seq=[0] * 258, cl_lens=[1] + [0] * 18)
_refused_header("refused_single_two_bit_distance_code", "distance set incomplete", d_lens=[2], body=list(b"abab") + [copy(3, 1)])
_refused_header("refused_unused_code_of_single_distance_code", "distance code", where="body", d_lens=[1],
                body=list(b"abab") + [copy(3, 1), ("ll", 257), ("raw", 1, 1)])
_refused_header("refused_length_symbol_without_any_distance_code", "distance code", where="body", d_lens=[0],
                body=list(b"abab") + [("ll", 257), ("raw", 0, 1)])


def _d_lens_are(want):
    def check(w):
        blk = w["blocks"][0]
        assert blk["lens"][blk["hlit"]:] == want
    return _accepted(check)


@case("single_one_bit_distance_code")
def _():
    return zlib_stream([dynamic(_SMALL_LL, [1], list(b"abab") + [copy(3, 1), 98, copy(3, 1)], final=True)]), _d_lens_are([1])


@case("single_one_bit_distance_code_on_symbol_5")
def _():
    b = dynamic(_SMALL_LL, [0] * 5 + [1], list(b"abababab") + [copy(3, 7), copy(3, 8)], final=True)
    return zlib_stream([b]), _d_lens_are([0] * 5 + [1])


@case("no_distance_code_and_no_length_symbol")
def _():
    return zlib_stream([dynamic(_SMALL_LL, [0], list(b"abbbaab"), final=True)]), _d_lens_are([0])


@case("ll_set_is_one_bit_eob_alone")
def _():
    ll = [0] * 257
    ll[256] = 1

    def check(w):
        assert w["blocks"][1]["lens"] == ll + [0] and w["out"] == b"xy"
    return zlib_stream([fixed(list(b"xy")), dynamic(ll, [0], [], final=True)]), _accepted(check)


# -- long codes
LADDER = list(range(1, 15)) + [15, 15]  # sixteen codes of 1 .. 14, 15, 15 bits: complete
LONG_LITS = tuple(range(12))
LONG_KINDS = ("lit", "len", "eob")


def long_ll_lens(variant, literals=LONG_LITS, extra=None):
    """LADDER on sixteen literal/length symbols.  The codes of 13, 14 and 15 bits go to (a literal, length 4, end-of-block)
    rotated by `variant`; the second 15-bit code is the literal `extra` (default literals[0] + 100); length 3 and the other literals take 1 .. 12 bits."""
    ll = [0] * 259
    tail = [literals[11], 258, 256]
    for ln, s in zip(range(1, 13), [literals[0], 257] + list(literals[1:11])):
        ll[s] = ln
    for ln, s in zip((13, 14, 15), tail[variant:] + tail[:variant]):
        ll[s] = ln
    ll[literals[0] + 100 if extra is None else extra] = 15
    assert code_set(ll) is None
    return ll


def long_ll_body(rng, literals=LONG_LITS, n=400):
    """every literal of the alphabet, both length symbols at distances 1 .. 4, mostly the short codes"""
    p = np.array([2.0 ** -min(k + 1, 6) for k in range(12)])
    body = [int(literals[k]) for k in rng.choice(12, n, p=p / p.sum())] + list(literals)
    for at, (ln, d) in zip(range(20, 400, 38), [(3, 1), (4, 2), (3, 3), (4, 4), (4, 1), (3, 2), (4, 3), (3, 4), (4, 2), (4, 4)]):
        body.insert(at, copy(ln, d))
    return body + [literals[0] + 100, copy(4, 1), literals[11]]


def pre_long_ll(w, variant):
    want = {(LONG_KINDS[(k + variant) % 3], 13 + k) for k in range(3)} | {("lit", 15)}
    seen = {(s.kind, s.nbits) for b in w["blocks"] for s in b["syms"] if s.nbits > LL_BITS}
    assert w["error"] is None and want <= seen, (want, seen)
    return f"codes above {LL_BITS} bits: {sorted(seen)}"


def _ll_case(variant):
    @case(f"long_ll_codes_variant_{variant}")
    def _():
        b = dynamic(long_ll_lens(variant), [2, 2, 2, 2], long_ll_body(_rng(40 + variant)), final=True)
        return zlib_stream([b]), lambda w: pre_long_ll(w, variant)


for _v in range(3):
    _ll_case(_v)


@case("long_distance_codes")
def _():
    # distance symbols 0 .. 15 on the ladder, the long codes on the far symbols; every symbol at both ends of its range
    ll = balanced(list(range(8)) + [256, 257, 260, 285], 286)
    rng = _rng(44)
    body = [int(x) for x in rng.integers(0, 8, 300)]
    for ds in range(16):
        for dist in sorted({DBASE[ds], DBASE[ds] + (1 << DEXTRA[ds]) - 1}):
            body += [copy(int(rng.choice([3, 6, 258])), dist), int(rng.integers(0, 8))]
    b = dynamic(ll, LADDER, body, final=True)

    def pre(w):
        seen = {s.dbits for s in w["blocks"][0]["syms"] if s.kind == "len"}
        assert w["error"] is None and seen == set(range(1, 16)), seen
        assert {x for x in seen if x > D_BITS} == {11, 12, 13, 14, 15}
    return zlib_stream([b]), pre


@case("literal_pairs_straddle_segment_ends")
def _():
    ll = [0] * 257
    for s, ln in zip((101, 116, 97, 111, 110, 105, 256), (1, 2, 3, 4, 5, 6, 6)):
        ll[s] = ln
    body = [int(x) for x in _rng(45).choice([101, 116, 97, 111, 110, 105], 2600, p=[.35, .25, .15, .1, .08, .07])]
    b = dynamic(ll, [0], body, final=True)

    def pre(w):
        blk = w["blocks"][0]
        syms = blk["syms"]
        n = sum(1 for a, c in zip(syms, syms[1:]) if a.kind == c.kind == "lit" and a.nbits + c.nbits <= LL_BITS
                and (a.bit - blk["body"]) // SEG_BITS != (c.bit - blk["body"]) // SEG_BITS)
        assert w["error"] is None and n >= 16 and max(s.nbits for s in syms) == 6
        return f"{n} pairs of literals across segment ends"
    return zlib_stream([b]), pre


# -- round cuts
RUN_LL = [0] * 258
RUN_LL[257], RUN_LL[97], RUN_LL[256] = 1, 2, 2   # length 3 on one bit
RUN_LL345 = [0] * 260                            # lengths 3, 4, 5 on 2, 2, 3 bits; a, b, c; end-of-block
for _s, _l in ((257, 2), (258, 2), (259, 3), (97, 3), (98, 4), (99, 4), (256, 3)):
    RUN_LL345[_s] = _l
N_RUN = 2133  # 1 + 3 * 2133 = 6400 = 80 * 80


def run_block(lead, copies, final=True, ll=None):
    """literals, then copies; the distance code has one bit (one distance) or is balanced on the distance symbols in use"""
    ds = sorted({distance_symbol(c[2])[0] for c in copies})
    d = [0] * (max(ds) + 1)
    if len(ds) == 1:
        d[ds[0]] = 1
    else:
        d = balanced(ds, max(ds) + 1)
    return dynamic(ll or RUN_LL, d, list(lead) + list(copies), final=final)


def pre_mlist(w, blk_index=0):
    blk = w["blocks"][blk_index]
    assert w["error"] is None
    msg = []
    for nt in LANES:
        what, lane = round_cut(blk, nt)
        assert what == "mlist" and lane > 0, (nt, what, lane)
        cps = round_copies(blk, nt)
        assert nt < len(cps) <= MLIST_CAP
        assert chained(cps[nt - 1], cps[nt]) and chained(cps[nt - 2], cps[nt - 1])  # the chain crosses copy index NT
        msg.append(f"NT {nt}: list cut at lane {lane} with {len(cps)} copies")
    return "; ".join(msg)


def _mlist_case(name, lead, copies, ll=None):
    @case(name)
    def _():
        return zlib_stream([run_block(lead, copies, ll=ll)]), pre_mlist


_mlist_case("mlist_cap_runs_3_1", b"a", [copy(3, 1)] * N_RUN)
_mlist_case("mlist_cap_period_2_length_3", b"ab", [copy(3, 2)] * N_RUN, RUN_LL345)
_mlist_case("mlist_cap_period_3_lengths_4_5", b"abc", [copy(4, 3), copy(5, 3)] * (N_RUN // 2 + 1), RUN_LL345)
_mlist_case("mlist_cap_period_2_lengths_3_5_4", b"ab", [copy(3, 2), copy(5, 2), copy(4, 2)] * (N_RUN // 3 + 1), RUN_LL345)


@case("lane_out_cap")
def _():
    ll = [0] * 286
    ll[285], ll[97], ll[256], ll[98] = 1, 2, 3, 3
    b = dynamic(ll, [1], [97] + [copy(258, 1)] * 200 + [98] + [copy(258, 1)] * 30, final=True)

    def pre(w):
        assert w["error"] is None
        for nt in LANES:
            assert round_cut(w["blocks"][0], nt) == ("lane", 0)
    return zlib_stream([b]), pre


@case("round_out_budget")
def _():
    ll = [0] * 286
    ll[97], ll[98], ll[285], ll[256] = 2, 2, 2, 2
    rng = _rng(46)
    body = [97, 98, 98]
    for k in range(160):
        body += [copy(258, int(rng.integers(1, 4)))] + [int(x) for x in rng.choice([97, 98], 13)]
    b = dynamic(ll, [2, 2, 2, 2], body, final=True)

    def pre(w):
        assert w["error"] is None
        msg = []
        for nt in LANES:
            what, lane = round_cut(w["blocks"][0], nt)
            assert what == "budget" and lane > 0, (nt, what, lane)
            msg.append(f"NT {nt}: budget cut at lane {lane}")
        return "; ".join(msg)
    return zlib_stream([b]), pre


def _pre_one_round(w, n_copies):
    blk = w["blocks"][0]
    assert w["error"] is None
    for nt in LANES:
        assert round_cut(blk, nt)[0] is None and blk["end"] - blk["body"] < nt * SEG_BITS
    cps = [s for s in blk["syms"] if s.kind == "len"]
    assert len(cps) == n_copies
    return cps


@case("dependency_chain_640_copies_3_3")
def _():
    def pre(w):
        cps = _pre_one_round(w, 640)
        assert all(not chained(a, c) and c.out - c.dist == a.out for a, c in zip(cps, cps[1:]))  # each reads the one before
    return zlib_stream([run_block(b"abc", [copy(3, 3)] * 640, ll=RUN_LL345)]), pre


@case("doubling_chain")
def _():
    cps = [copy(n, n) for n in (3, 6, 12, 24, 48, 96, 192)] + [copy(258, 258), copy(258, 384)]

    def pre(w):
        assert all(s.dist == s.out for s in _pre_one_round(w, 9)[:7])
    return zlib_stream([fixed(list(b"xyz") + cps, final=True)]), pre


@case("periodic_chain_interrupted")
def _():
    b = run_block(b"ab", [copy(3, 1)] * 300 + [copy(3, 2)] + [copy(3, 1)] * 300 + [copy(5, 2), copy(4, 3)] + [copy(3, 1)] * 40, ll=RUN_LL345)

    def pre(w):
        cps = _pre_one_round(w, 643)
        assert chained(cps[298], cps[299]) and not chained(cps[299], cps[300]) and not chained(cps[300], cps[301])
    return zlib_stream([b]), pre


# -- positions
def _first_copy(w):
    blk = w["blocks"][0]
    s = [x for x in blk["syms"] if x.kind == "len"][0]
    return s, (s.bit - blk["body"]) // SEG_BITS


@case("distance_equals_position_lane_0")
def _():
    def pre(w):
        s, lane = _first_copy(w)
        assert w["error"] is None and s.dist == s.out == 7 and lane == 0
    return zlib_stream([fixed(list(b"abcdefg") + [copy(7, 7), copy(20, 14)], final=True)]), pre


@case("distance_equals_position_later_lane")
def _():
    lits = bytes(_rng(47).integers(0, 256, 100, dtype=np.uint8))

    def pre(w):
        s, lane = _first_copy(w)
        assert w["error"] is None and s.dist == s.out == 100 and 1 <= lane < LANES[0]
        return f"lane {lane}"
    return zlib_stream([fixed(list(lits) + [copy(100, 100), copy(258, 200)], final=True)]), pre


@case("refused_distance_position_plus_one_lane_0", "refuse")
def _():
    def pre(w):
        s, lane = _first_copy(w)
        assert s.dist == s.out + 1 and lane == 0
        return _stops("distance too far back")(w)
    return zlib_stream([fixed(list(b"abc") + [("ld", 257, 0, 3, 0)], final=True)], data=b"abc"), pre


@case("refused_distance_position_plus_one_later_lane", "refuse")
def _():
    lits = bytes(_rng(48).integers(0, 256, 100, dtype=np.uint8))
    s_, _, xv = distance_symbol(101)

    def pre(w):
        s, lane = _first_copy(w)
        assert s.dist == s.out + 1 == 101 and 1 <= lane < LANES[0]
        return _stops("distance too far back")(w) + f", lane {lane}"
    return zlib_stream([fixed(list(lits) + [("ld", 257, 0, s_, xv)] + list(lits[:50]), final=True)], data=lits), pre


RING_LITS = (3, 7, 11, 19, 23, 42, 77, 100, 128, 150, 199, 200, 240, 255)


def _ring_block(copies, seed):
    """32 KiB of literals on 4-bit codes, then copies of length 258 with distances of 24577 .. 32768"""
    ll = [0] * 286
    for s in RING_LITS + (256, 285):
        ll[s] = 4
    lits = [RING_LITS[k] for k in _rng(seed).integers(0, 14, 32768)]
    return dynamic(ll, [0] * 29 + [1], lits + copies, final=True)


def _straddles(lo, n):
    return lo // INF_RING != (lo + n - 1) // INF_RING


def _pre_ring(w):
    cps = [s for s in w["blocks"][0]["syms"] if s.kind == "len"]
    src = [s for s in cps if _straddles(s.out - s.dist, s.length)]
    dst = [s for s in cps if _straddles(s.out, s.length)]
    assert w["error"] is None and src and dst and len(w["out"]) <= 300 * 1024
    return f"{len(src)} sources and {len(dst)} destinations straddle a multiple of the ring"


@case("ring_258_32768_to_200k")
def _():
    def pre(w):
        cps = [s for s in w["blocks"][0]["syms"] if s.kind == "len"]
        assert all(s.dist == 32768 and s.length == 258 for s in cps) and len(w["out"]) >= 200000
        return _pre_ring(w)
    return zlib_stream([_ring_block([copy(258, 32768)] * 651, 49)]), pre


@case("distance_32768_at_position_32768")
def _():
    def pre(w):
        s, _ = _first_copy(w)
        assert w["error"] is None and s.out == s.dist == 32768
    return zlib_stream([_ring_block([copy(258, 32768), copy(258, 32768 - 300), copy(258, 32768)], 53)]), pre


@case("ring_mixed_far_copies")
def _():
    rng = _rng(50)
    cps = [copy(258, int(rng.choice([32768, 32767, 24577, 32768 - 257]))) for _ in range(420)]
    return zlib_stream([_ring_block(cps, 51)]), _pre_ring


# -- blocks
def _n_blocks(n, out=None):
    def check(w):
        assert len(w["blocks"]) == n and (out is None or w["out"] == out)
    return _accepted(check)


@case("blocks_300_dynamic_of_one_literal")
def _():
    blocks = [dynamic(balanced([k % 256, 256], 257), [0], [k % 256], final=k == 299) for k in range(300)]
    return zlib_stream(blocks), _n_blocks(300)


def _empty_case(last):
    @case(f"blocks_empty_interleaved_final_{last}")
    def _():
        ll = [0] * 257
        ll[256] = 1
        seq = [fixed(), dynamic(ll, [0]), stored(), fixed(list(b"q")), stored(), stored(b"rs"), dynamic(balanced([0, 256], 257), [0]),
               fixed(), fixed(), stored(), dynamic(ll, [0])]
        seq.append({"fixed": fixed(), "dynamic": dynamic(ll, [0]), "stored": stored()}[last])
        seq[-1]["final"] = True

        def check(w):
            assert len(w["blocks"]) == 12 and w["out"] == b"qrs" and w["blocks"][-1]["type"] == ("stored", "fixed", "dynamic").index(last)
        return zlib_stream(seq), _accepted(check)


for _last in ("fixed", "dynamic", "stored"):
    _empty_case(_last)


@case("blocks_stored_0_and_65535")
def _():
    data = bytes(_rng(52).integers(0, 256, 65535, dtype=np.uint8))

    def check(w):
        sizes = [(b["end"] - b["body"]) // 8 for b in w["blocks"] if b["type"] == 0]
        assert sizes == [0, 65535, 0, 1]
    return zlib_stream([stored(), stored(data), stored(), fixed(list(b"end")), stored(b"x", final=True)]), _accepted(check)


@case("blocks_stored_after_fixed_at_each_bit_phase")
def _():
    blocks = []
    for k in range(8):  # k nine-bit literals (144 and above) move the end of the fixed block through all phases
        blocks += [fixed([65 + k] + [200 + k] * k), stored(bytes([k, 255 - k, k]))]
    blocks[-1]["final"] = True

    def check(w):
        ends = [b["end"] % 8 for b in w["blocks"] if b["type"] == 1]
        assert sorted(ends) == list(range(8)), ends
    return zlib_stream(blocks), _accepted(check)


@case("refused_stored_len_nlen_mismatch", "refuse")
def _():
    return (zlib_stream([fixed(list(b"ab")), stored(b"cdef", final=True, nlen_field=0xFFFA)], data=b"abcdef"),
            _stops("stored lengths", block=1))


@case("refused_block_type_3", "refuse")
def _():
    return zlib_stream([fixed(list(b"ab")), raw_bits([(3, 2), (0, 13)], final=True)], data=b"ab"), _stops("block type 3", block=1)


def _fixed_bad(name, item, why):
    @case(name, "refuse")
    def _():
        def pre(w):
            assert w["blocks"][0]["type"] == 1 and len(w["blocks"][0]["syms"]) == 6
            return _stops(why, where="body")(w)
        return zlib_stream([fixed(list(b"abcabc") + [item] + list(b"abc"), final=True)], data=b"abcabc"), pre


_fixed_bad("refused_fixed_symbol_286", ("ll", 286), "literal/length code")
_fixed_bad("refused_fixed_symbol_287", ("ll", 287), "literal/length code")
_fixed_bad("refused_fixed_distance_30", ("ld", 257, 0, 30, 0), "distance code")
_fixed_bad("refused_fixed_distance_31", ("ld", 257, 0, 31, 0), "distance code")


@case("fixed_block_uses_symbol_285_and_distance_29")
def _():
    body = [7] * 3 + [copy(258, 1)] * 96 + [copy(258, 24577), copy(257, 3)]

    def check(w):
        syms = w["blocks"][0]["syms"]
        assert any(s.dist == 24577 for s in syms) and any(s.length == 257 for s in syms)
    return zlib_stream([fixed(body, final=True)]), _accepted(check)


def _truncated(name, cut_of, inside):
    @case(name, "truncate")
    def _():
        good = zlib_stream([long_header_block(_LONG_PAYLOAD[:64], final=False), fixed(list(b"tail") + [copy(30, 4)], final=True)])
        g = walk(good)
        assert g["error"] is None
        n = cut_of(g, good)

        def pre(w):
            lo, hi = inside(g)
            assert w["error"] == "truncated" and lo < 8 * n <= hi, (lo, 8 * n, hi)
            return f"cut at bit {8 * n} of ({lo}, {hi}]"
        return good[:n], pre


_truncated("truncated_inside_header", lambda g, s: (g["blocks"][0]["start"] + 1000) // 8,
           lambda g: (g["blocks"][0]["start"] + 17, g["blocks"][0]["body"] - 8))
_truncated("truncated_inside_body", lambda g, s: (g["blocks"][0]["body"] + 200) // 8,
           lambda g: (g["blocks"][0]["body"], g["blocks"][0]["end"] - 8))
_truncated("truncated_inside_second_block", lambda g, s: (g["blocks"][1]["body"] + 20) // 8,
           lambda g: (g["blocks"][1]["body"], g["blocks"][1]["end"] - 8))
_truncated("truncated_before_adler", lambda g, s: len(s) - 4, lambda g: (g["blocks"][1]["end"] - 1, g["trailer"]))
_truncated("truncated_inside_adler", lambda g, s: len(s) - 2, lambda g: (g["trailer"], g["trailer"] + 24))
_truncated("truncated_last_adler_byte", lambda g, s: len(s) - 1, lambda g: (g["trailer"], g["trailer"] + 24))


@case("refused_adler_mismatch", "refuse")
def _():
    return zlib_stream([fixed(list(b"abc"), final=True)], adler=zlib.adler32(b"abc") ^ 0x10000), _stops("adler")


@case("refused_zlib_header_check", "refuse")
def _():
    return zlib_stream([fixed(list(b"abc"), final=True)], flg=0x9D), _stops("zlib header", block=-1)


@case("zlib_header_window_256")
def _():
    return zlib_stream([fixed(list(b"abc") + [copy(9, 3)], final=True)], cmf=0x08), _accepted(lambda w: w["out"] == b"abc" * 4 or 1 / 0)


def oracle_verdict(stream, limit=1 << 20):
    """what CPython's zlib does with a stream, with the semantics of zlib.decompress: bytes, or None when it refuses or the
    stream is incomplete"""
    try:
        d = zlib.decompressobj()
        out = d.decompress(stream, limit)
        return out if d.eof and not d.unconsumed_tail else None
    except zlib.error:
        return None


# -- the capacity cases, built from the largest accepted output of everything above
def base_cases():
    return [build() for _, build in _CASES]


@functools.lru_cache(maxsize=None)
def max_out():
    """the largest accepted output of the named cases: the max_out of the device batch"""
    return max(len(walk(c.stream)["out"]) for c in base_cases() if c.accept)


def out_stride(m):
    """the slot size zlib_decompress_batch (cct_hip/batch.py) gives max_out = m; the device test checks it against the product"""
    return (m + 15 + 16) & ~15


def _stored_run(n, seed):
    data = bytes(_rng(seed).integers(0, 256, n, dtype=np.uint8))
    blocks = [stored(data[i:i + 65535]) for i in range(0, n, 65535)]
    blocks[-1]["final"] = True
    return zlib_stream(blocks)


@functools.lru_cache(maxsize=None)
def cap_cases():
    """[(name, stream, status)]: an output of exactly max_out bytes (fits), and outputs one byte and one whole 16-byte granule
    longer than the slot (CCT_E_CAP).  zlib accepts all three."""
    m = max_out()
    return [("cap_exactly_max_out", _stored_run(m, 60), 0), ("cap_one_byte_above_out_stride", _stored_run(out_stride(m) + 1, 61), E_CAP),
            ("cap_one_granule_above_out_stride", _stored_run(out_stride(m) + 16, 62), E_CAP)]


def cases():
    """every named case; cap_cases() join them in the device batch and in the fixture"""
    return base_cases()
