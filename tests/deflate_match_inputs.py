"""Inputs that put one string on every off-by-one edge of zlib 1.2.11's longest_match / deflate_slow, and of the device's
own restatement of them (csrc/deflate_kernels.hip: sort records, light and cooperative walks, run kernels, dfl_rec_kernel).
No device is needed here: every expectation of bytes is libz's; the `census` of a case only proves, on libz's own token
stream and on the hash chains, that the input reaches the edge it is named after.

How an input is made
  * filler: bytes of a 64-symbol alphabet in which no 3-byte string occurs twice (`FILLER`), so the filler alone has no match;
  * plants: strings over bytes outside that alphabet.  zlib's hash keeps the low five bits (memLevel 8; six at memLevel 9) of
    the third byte of a trigram untouched, so bytes are split into classes by `b & 31`: the filler uses classes 8 .. 31, plants
    classes 0 .. 7, and the third byte Z of the probe trigram T = (X, Y, Z) is the only byte of class 0 in an input.  Nothing
    but the strings planted on purpose can therefore enter T's hash bucket, at either hash width, filler/plant seams included;
  * the census re-derives the bucket from the bytes (`chain`, `sorted_index`) and asserts its shape, so a slip in this
    reasoning fails the host test instead of silently missing the edge.
"""
import functools
import zlib

import numpy as np

import deflate_blocks as db

MIN_MATCH, MAX_MATCH = 3, 258
MAX_DIST = 32768 - (MAX_MATCH + MIN_MATCH + 1)  # 32506
MIN_LOOKAHEAD = 262
TOO_FAR = 4096
Z_FILTERED = 1
LEVELS = (4, 5, 6, 7, 8, 9)
#         level: (good, lazy, nice, chain)
PARAMS = {4: (4, 4, 16, 16), 5: (8, 16, 32, 32), 6: (8, 16, 128, 128), 7: (8, 32, 128, 256), 8: (32, 128, 258, 1024),
          9: (32, 258, 258, 4096)}
LIGHT_STEPS = 12   # dfl_match_kernel: chain entries a lane examines before the position is queued for the wave
RUNLEN_OUT = 1784  # positions a workgroup of the run kernels publishes
REC_BLOCK = 64     # positions per block of dfl_rec_kernel

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]


# ------------------------------------------------------------------------------------------------------- token reader
def _lut(lengths):
    """canonical Huffman code -> (table indexed by the next `bits` stream bits, LSB first, of (symbol, length); bits)"""
    bits = max(max(lengths), 1)
    table = [None] * (1 << bits)
    for (ln, code), sym in db._decoder(lengths).items():
        rev = int(format(code, f"0{ln}b")[::-1], 2)
        n = 1 << (bits - ln)
        table[rev::1 << ln] = [(sym, ln)] * n
    return table, (1 << bits) - 1


_FIXED = None


def libz(data, level=9, strategy=0, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, mem_level, strategy)
    return c.compress(data) + c.flush()


def tokens(stream, length=None):
    """([(position, length, distance)], [(position, bytes)] of the stored blocks) of a zlib stream: a small inflate that
    records matches instead of copying them.  The positions must add up to the length of the input."""
    global _FIXED
    if length is None:
        length = len(zlib.decompress(stream))
    bits = db._Bits(stream[2:])
    d = bits.d + bytes(4)
    toks, stored, p = [], [], 0
    while True:
        final, btype = bits.get(1), bits.get(2)
        if btype == 0:
            bits.pos = (bits.pos + 7) & ~7
            n = bits.get(16)
            assert bits.get(16) == n ^ 0xFFFF
            stored.append((p, n))
            bits.pos += 8 * n
            p += n
        else:
            assert btype in (1, 2)
            if btype == 1:
                if _FIXED is None:
                    _FIXED = _lut([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _lut([5] * 30)
                (lt, lmask), (dt, dmask) = _FIXED
            else:
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[db.BL_ORDER[i]] = bits.get(3)
                ct, lens = db._decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = db._sym(bits, ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.get(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.get(3))
                    else:
                        lens += [0] * (11 + bits.get(7))
                (lt, lmask), (dt, dmask) = _lut(lens[:hlit]), _lut(lens[hlit:])
            pos = bits.pos
            while True:
                i = pos >> 3
                s, ln = lt[(int.from_bytes(d[i:i + 4], "little") >> (pos & 7)) & lmask]
                pos += ln
                if s < 256:
                    p += 1
                elif s == 256:
                    break
                else:
                    s -= 257
                    i = pos >> 3
                    v = int.from_bytes(d[i:i + 8], "little") >> (pos & 7)
                    e = db.LEXTRA[s]
                    mlen = LBASE[s] + (v & ((1 << e) - 1))
                    v >>= e
                    c, ln = dt[v & dmask]
                    v >>= ln
                    e2 = db.DEXTRA[c]
                    toks.append((p, mlen, DBASE[c] + (v & ((1 << e2) - 1))))
                    pos += e + ln + e2
                    p += mlen
            bits.pos = pos
        if final:
            break
    assert p == length, (p, length)
    return toks, stored


class Tokens:
    """the matches of one stream, for a census: at(p) = (length, distance) of the token that starts at p, or None"""

    def __init__(self, toks, stored, length):
        self.toks, self.stored, self.length = toks, stored, length
        self._at = {p: (ln, dist) for p, ln, dist in toks}
        self._starts = np.array([t[0] for t in toks], dtype=np.int64)
        self._ends = np.array([t[0] + t[1] for t in toks], dtype=np.int64)

    def at(self, p):
        return self._at.get(p)

    def length_at(self, p):
        return self._at.get(p, (0, 0))[0]

    def covering(self, p):
        """the token that codes byte p, or None if p is a literal"""
        k = int(np.searchsorted(self._starts, p, side="right")) - 1
        return self.toks[k] if k >= 0 and self._ends[k] > p else None

    def literal(self, p, n=1):
        return all(self.covering(q) is None for q in range(p, p + n))

    def first_difference(self, other):
        """(token of self, token of other) where the two lists first differ; None past the end of a list"""
        n = min(len(self.toks), len(other.toks))
        k = next((k for k in range(n) if self.toks[k] != other.toks[k]), n)
        return (self.toks[k] if k < len(self.toks) else None, other.toks[k] if k < len(other.toks) else None)


@functools.lru_cache(maxsize=None)
def _libz_tokens(data, level, strategy, mem_level):
    return Tokens(*tokens(libz(data, level, strategy, mem_level), len(data)), len(data))


def libz_tokens(data, level, strategy=0, mem_level=8):
    return _libz_tokens(bytes(data), level, strategy, mem_level)


# ------------------------------------------------------------------------------------------------------- hashes
def hash15(b0, b1, b2):
    """zlib's UPDATE_HASH over three bytes at memLevel 8: hash_bits 15, hash_shift 5"""
    return ((b0 << 10) ^ (b1 << 5) ^ b2) & 0x7FFF


def hash16(b0, b1, b2):
    """memLevel 9: hash_bits 16, hash_shift 6"""
    return ((b0 << 12) ^ (b1 << 6) ^ b2) & 0xFFFF


@functools.lru_cache(maxsize=64)
def _hashes(data, hash_bits):
    a = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
    if len(a) < 3:
        return np.zeros(0, dtype=np.int64)
    sh = {15: 5, 16: 6}[hash_bits]
    return ((a[:-2] << (2 * sh)) ^ (a[1:-1] << sh) ^ a[2:]) & ((1 << hash_bits) - 1)


def hashes(data, hash_bits=15):
    """hash of the string at every position 0 .. L-3"""
    return _hashes(bytes(data), hash_bits)


def sorted_index(data, p, hash_bits=15):
    """index of position p in the stable sort of all positions by (hash, position): the order the kernels walk chains in"""
    h = hashes(data, hash_bits)
    return int(np.count_nonzero(h < h[p]) + np.count_nonzero(h[:p] == h[p]))


def chain(data, p, hash_bits=15):
    """earlier positions in p's hash bucket, nearest first (window and NIL rules not applied)"""
    h = hashes(data, hash_bits)
    return [int(q) for q in np.flatnonzero(h[:p] == h[p])[::-1]]


# ------------------------------------------------------------------------------------------------------- filler
def _no_repeat(alphabet, n, seed):
    """n bytes over `alphabet` in which no 3-byte string occurs twice (a greedy walk; the alphabet is large enough that it
    never runs out at the sizes used here)"""
    k = len(alphabet)
    used = bytearray(k * k * k)
    state = seed
    out = [seed % k, (seed // k) % k]
    a, b = out
    for _ in range(n - 2):
        state = (state * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        c = (state >> 33) % k
        base = (a * k + b) * k
        for _ in range(k):
            if not used[base + c]:
                break
            c = c + 1 if c + 1 < k else 0
        else:
            raise AssertionError("filler alphabet exhausted")
        used[base + c] = 1
        out.append(c)
        a, b = b, c
    return bytes(alphabet[c] for c in out)


FILL_ALPHABET = bytes(list(range(0x28, 0x40)) + list(range(0x48, 0x60)) + list(range(0x68, 0x78)))  # classes 8 .. 31
BODY_ALPHABET = bytes(b for b in range(256) if 1 <= (b & 31) <= 6)                                 # 48 plant bytes
assert len(FILL_ALPHABET) == 64 and all((b & 31) >= 8 for b in FILL_ALPHABET)


@functools.lru_cache(maxsize=None)
def filler():
    return _no_repeat(FILL_ALPHABET, 150000, 12345)


@functools.lru_cache(maxsize=None)
def body():
    """plant material: no 3-byte string twice, classes 1 .. 6"""
    return _no_repeat(BODY_ALPHABET, 4000, 777)


# the probe trigram T; Z is the only class-0 byte of an input.  X is of class 16, so that about a third of the filler's
# strings hash below T and a pad in front of an input moves p through the sorted order
X, Y, Z = 0x90, 0x42, 0x00
T = bytes([X, Y, Z])
HEAD = 0xA7                 # first byte after T in a probe string: class 7, so no digit of an in-between entry equals it
W = 0xE3                    # the byte before p in the quarter-budget cases: guards and SEP are of class 7, so (W, X, Y) is alone in its bucket
G = (0x67, 0x87)            # guards before the two copies of a string
E = (0x27, 0x47, 0x07)      # terminators after copies of a string: pairwise different, so a match ends where the plant ends
SEP = 0xC7
# byte-different trigrams with T's hash: b0 ^ 0x20/0x40/0x80 collide at both widths (bits 5 .. 7 of b0 are shifted out),
# (X, Y^1, Z^0x20) at 15 bits only, (X, Y^1, Z^0x40) at 16 bits only
COLLIDE = {"same": T, "x20": bytes([X ^ 0x20, Y, Z]), "x40": bytes([X ^ 0x40, Y, Z]), "x80": bytes([X ^ 0x80, Y, Z]),
           "yz15": bytes([X, Y ^ 1, Z ^ 0x20]), "yz16": bytes([X, Y ^ 1, Z ^ 0x40])}
for _k, _t in COLLIDE.items():
    assert (hash15(*_t) == hash15(*T)) == (_k != "yz16") and (hash16(*_t) == hash16(*T)) == (_k != "yz15"), _k


def probe(n, start=0):
    """the probe string of n bytes: T, HEAD, then plant material"""
    return T + bytes([HEAD]) + body()[start:start + n - 4] if n > 3 else T[:n]


def entry(i, kind="same"):
    """i-th in-between chain entry: a trigram in T's bucket and three base-48 digits (classes 1 .. 6) that differ from HEAD,
    so that it shares exactly three bytes ("same") or none with the probe string"""
    a = BODY_ALPHABET
    return COLLIDE[kind] + bytes([a[i % 48], a[i // 48 % 48], a[i // 2304 % 48], SEP])


class Build:
    """an input under construction: filler taken in order from FILLER, plants appended where asked"""

    def __init__(self, skip=0):
        self.buf, self.fpos = bytearray(), skip

    def __len__(self):
        return len(self.buf)

    def fill(self, n):
        assert n >= 0
        f = filler()
        assert self.fpos + n <= len(f)
        self.buf += f[self.fpos:self.fpos + n]
        self.fpos += n

    def fill_to(self, pos):
        self.fill(pos - len(self.buf))

    def put(self, s):
        pos = len(self.buf)
        self.buf += bytes(s)
        return pos

    def bytes(self):
        return bytes(self.buf)


class Case:
    """(name, bytes, census) and what the census is valid for.  census(tk, level, strategy, mem_level) -> bool over the
    Tokens of libz's stream.  levels: where the census is checked (all six for level-independent cases)."""

    def __init__(self, family, name, data, census, levels=LEVELS, strategies=(0,), mem9=False, runs=False):
        self.family, self.name, self.data, self.census = family, name, data, census
        self.levels, self.strategies, self.mem9, self.runs = tuple(levels), tuple(strategies), mem9, runs

    def __iter__(self):
        return iter((self.name, self.data, self.census))

    def holds(self, level, strategy=0, mem_level=8):
        return bool(self.census(libz_tokens(self.data, level, strategy, mem_level), level, strategy, mem_level))


def _hash_bits(mem_level):
    return 15 if mem_level == 8 else 16


# ------------------------------------------------------------------------------------------------------- the families
def _window_cases():
    """1. the head of a chain may sit at MAX_DIST, later entries must be strictly closer"""
    out = []
    for where, lead in (("low", 9), ("high", 33100)):
        for dist in (MAX_DIST - 1, MAX_DIST, MAX_DIST + 1):
            for between in (None, "same", "x20"):
                b = Build()
                b.fill(lead)
                b.put([G[0]])
                q = b.put(probe(9))
                b.put([E[0]])
                if between:
                    b.fill(700)
                    mid = b.put(entry(0, between))
                p = q + dist
                b.fill_to(p - 1)
                b.put([G[1]])
                assert b.put(probe(9)) == p
                b.put([E[1]])
                b.fill(400)  # lookahead >= MIN_LOOKAHEAD: the slide quirk stays out of this family
                data = b.bytes()
                assert (p < 32768) if where == "low" else (p > 65536)
                found = dist <= (MAX_DIST - 1 if between else MAX_DIST)
                census = functools.partial(_window_census, data, p, q, mid if between else None, dist, between, found)
                out.append(Case("window", f"window_{where}_d{dist}_{between or 'head'}", data, census))
    return out


def _window_census(data, p, q, mid, dist, between, found, tk, level, strategy=0, mem_level=8):
    if chain(data, p, _hash_bits(mem_level)) != ([mid, q] if between else [q]):
        return False
    if found:
        return tk.at(p) == (9, dist)
    # cut: no 9-byte match at p; a same-trigram entry in between leaves a 3-byte candidate beyond TOO_FAR, which is dropped
    return tk.at(p) is None


def _nil_cases():
    """2. position 0 is NIL; the slide_hash quirk turns the string at the new window origin into NIL"""
    out = []
    for first in (0, 1):
        b = Build()
        b.fill(first)
        q = b.put(probe(9))
        b.put([E[0]])
        b.fill(120)
        b.put([G[1]])
        p = b.put(probe(9))
        b.put([E[1]])
        b.fill(400)
        data = b.bytes()

        def census(tk, level, strategy=0, mem_level=8, data=data, p=p, q=q):
            if chain(data, p, _hash_bits(mem_level)) != [q]:
                return False
            if q == 0:  # NIL at p; p + 1 finds the old string from its second byte on
                return tk.at(p) is None and tk.at(p + 1) == (8, p - q)
            return tk.at(p) == (9, p - q)
        out.append(Case("nil", f"nil_first_at_{first}", data, census))
    for k in (1, 2):
        for after in (1, 10, 261, 262, 263):
            b = Build()
            b.fill(32768 * k - 1)
            b.put([G[0]])
            q = b.put(probe(9))
            b.put([E[0]])
            p = q + MAX_DIST
            b.fill_to(p - 1)
            b.put([G[1]])
            b.put(probe(min(9, after)))
            if after > 9:
                b.put([E[1]])
                b.fill(after - 10)
            data = b.bytes()
            assert len(data) - p == after and q == 32768 * k and p == MAX_DIST + 32768 * k

            def census(tk, level, strategy=0, mem_level=8, data=data, p=p, q=q, after=after):
                if after >= 3 and chain(data, p, _hash_bits(mem_level)) != [q]:
                    return False
                if after >= MIN_LOOKAHEAD:  # no slide yet: the head at MAX_DIST is taken
                    return tk.at(p) == (9, MAX_DIST)
                return tk.at(p) is None    # the window slid: the candidate is NIL (or the lookahead is below MIN_MATCH)
            out.append(Case("nil", f"nil_slide_k{k}_after{after}", data, census))
    return out


def _chain_input(n_mid, kind, pad=0, long_len=9):
    """probe string, n_mid in-between entries of T's bucket, probe string again at p: the old copy is chain entry n_mid + 1"""
    b = Build()
    b.fill(8 + pad)
    b.put([G[0]])
    q = b.put(probe(long_len))
    b.put([E[0]])
    b.fill(5)
    for i in range(n_mid):
        b.put(entry(i, kind))
    b.fill(5)
    b.put([G[1]])
    p = b.put(probe(long_len))
    b.put([E[1]])
    b.fill(400)
    return b.bytes(), p, q


def _chain_census(data, p, q, depth, kind, tk, level, strategy=0, mem_level=8):
    bits = _hash_bits(mem_level)
    ch = chain(data, p, bits)
    collide = kind in ("same", "x20", "x40", "x80") or (kind == "yz15") == (bits == 15)
    if ch[-1] != q or len(ch) != (depth if collide else 1) or p - q >= MAX_DIST:
        return False
    if len(ch) <= PARAMS[level][3]:
        return tk.at(p) == (9, p - q)
    return tk.length_at(p) < 9 and tk.at(p + 1) == (8, p - q)  # p + 1 heads a chain of its own and finds the rest


def _tune_pad(make, want, limit=1200):
    """vary the pad in front of an input until want(data, p) holds: about one filler string in three sorts before T's
    bucket, so a longer pad moves the sorted index of p through every residue"""
    for pad in range(limit):
        r = make(pad)
        if want(r[0], r[1]):
            return r
    raise AssertionError("no pad puts the position where the case needs it")


def _chain_cases():
    """3. max_chain entries are examined; 4. the best candidate on either side of the light walk's 12 entries and of the
    cooperative matcher's 64-candidate steps; 11. the same with p in the first lanes of a wave of the sorted order"""
    out = []
    depths = {}
    for level in LEVELS:
        mc = PARAMS[level][3]
        for d in (mc, mc + 1, mc + 2):  # max_chain - 1, max_chain, max_chain + 1 entries in between
            depths.setdefault(d, ("budget", f"L{level}"))
    for d in (11, 12, 13, 14, 63, 64, 65, 128, 129):
        depths[d] = ("steps", "") if d not in depths else depths[d]
    for depth, (family, tag) in sorted(depths.items()):
        kinds = ("same", "x20") if depth > 2000 else ("same", "x20", "x80") if family == "budget" else ("same", "x40")
        for kind in kinds:
            data, p, q = _chain_input(depth - 1, kind)
            out.append(Case(family, f"{family}_depth{depth}_{kind}", data,
                            functools.partial(_chain_census, data, p, q, depth, kind)))
    # hash collisions of one width only: at memLevel 8 / 9 the in-between entries are in the bucket or not
    for depth in (17, 18, 129, 130):
        for kind in ("yz15", "yz16"):
            data, p, q = _chain_input(depth - 1, kind)
            out.append(Case("budget", f"budget_depth{depth}_{kind}", data,
                            functools.partial(_chain_census, data, p, q, depth, kind), mem9=True))
    # 11. sorted-order seams
    for depth in (13, 16, 17, 33, 65, 129, 257, 1025):
        for kind in ("same", "x20"):
            data, p, q = _tune_pad(lambda pad: _chain_input(depth - 1, kind, pad),  # noqa: B023
                                   lambda d, p: sorted_index(d, p) % 64 <= LIGHT_STEPS)
            out.append(Case("sorted", f"sorted_lane_depth{depth}_{kind}", data,
                            functools.partial(_sorted_census, data, p, q, depth, kind, 64)))
    for depth in (13, 17, 65):
        data, p, q = _tune_pad(lambda pad: _chain_input(depth - 1, "same", pad),  # noqa: B023
                               lambda d, p: sorted_index(d, p) % 256 <= LIGHT_STEPS - 1)
        out.append(Case("sorted", f"sorted_block_depth{depth}_same", data,
                        functools.partial(_sorted_census, data, p, q, depth, "same", 256)))
    return out


def _sorted_census(data, p, q, depth, kind, modulus, tk, level, strategy=0, mem_level=8):
    if mem_level == 8 and sorted_index(data, p) % modulus > (LIGHT_STEPS if modulus == 64 else LIGHT_STEPS - 1):
        return False  # the light walk's 12 candidates start in the previous wave (workgroup) of the sorted order
    return _chain_census(data, p, q, depth, kind, tk, level, strategy, mem_level)


def _nice_in_step_cases():
    """4. a nice-reaching entry and a longer one in the same 64-candidate step, in both orders"""
    out = []
    for level, (da, db_) in ((5, (15, 25)), (7, (20, 40)), (7, (70, 100))):
        nice = PARAMS[level][2]
        for order in ("nice_nearer", "longer_nearer"):
            na, nb = (nice, nice + 9) if order == "nice_nearer" else (nice + 9, nice)
            b = Build()
            b.fill(8)
            b.put([G[0]])
            qb = b.put(probe(nb))           # farther of the two
            b.put([E[0]])
            b.fill(3)
            for i in range(db_ - da - 1):
                b.put(entry(i, "same"))
            b.fill(3)
            b.put([G[1]])
            qa = b.put(probe(na))           # nearer
            b.put([E[1]])
            b.fill(3)
            for i in range(da - 1):
                b.put(entry(1000 + i, "same"))
            b.fill(3)
            b.put([SEP])
            p = b.put(probe(nice + 12))
            b.put([E[2]])
            b.fill(400)
            data = b.bytes()

            def census(tk, level_, strategy=0, mem_level=8, data=data, p=p, qa=qa, qb=qb, na=na, da=da, db_=db_):
                ch = chain(data, p, _hash_bits(mem_level))
                if len(ch) != db_ or ch[da - 1] != qa or ch[db_ - 1] != qb:
                    return False
                return tk.at(p) == (na, p - qa)  # the nearer one either reaches nice and ends the walk, or is the longer
            out.append(Case("steps", f"steps_L{level}_{order}_at{da}_{db_}", data, census, levels=(level,)))
    return out


def _quarter_cases():
    """5. once prev_length >= good_match the budget is max_chain >> 2"""
    out = []
    for level in LEVELS:
        good, lazy, nice, mc = PARAMS[level]
        for c in ((mc >> 2), (mc >> 2) + 1):
            for m in (good - 1, good):
                for kind in ("same", "x40"):
                    if kind == "x40" and c > 300:
                        continue
                    out.append(_quarter_case(level, c, m, kind))
    # 11. the same with p early in a wave of the sorted order
    for level in (5, 7, 8):
        good, lazy, nice, mc = PARAMS[level]
        for c in ((mc >> 2), (mc >> 2) + 1):
            out.append(_quarter_case(level, c, good, "same", tuned=True))
    return out


def _quarter_input(level, c, m, kind, pad=0):
    len2 = m + 3
    own = 1 if m - 1 >= 3 else 0  # the string matched at p - 1 holds T itself: one more entry of p's bucket
    b = Build()
    b.fill(8 + pad)
    b.put([G[0]])
    ql = b.put(probe(len2))
    b.put([E[0]])
    b.fill(5)
    for i in range(c - 1 - own):
        b.put(entry(i, kind))
    b.fill(5)
    b.put([G[1]])
    qm = b.put(bytes([W]) + probe(m - 1))
    b.put([E[1]])
    b.fill(4)
    b.put([W])
    p = b.put(probe(len2))
    b.put([E[2]])
    b.fill(400)
    return b.bytes(), p, ql, qm


def _quarter_case(level, c, m, kind, tuned=False):
    good, lazy, nice, mc = PARAMS[level]
    if tuned:
        data, p, ql, qm = _tune_pad(lambda pad: _quarter_input(level, c, m, kind, pad),
                                    lambda d, p: sorted_index(d, p) % 64 <= LIGHT_STEPS)
    else:
        data, p, ql, qm = _quarter_input(level, c, m, kind)
    len2 = m + 3

    def census(tk, level_, strategy=0, mem_level=8):
        ch = chain(data, p, _hash_bits(mem_level))
        if len(ch) != c or ch[-1] != ql or chain(data, p - 1, _hash_bits(mem_level)) != [qm]:
            return False
        if tuned and mem_level == 8 and sorted_index(data, p) % 64 > LIGHT_STEPS:
            return False
        g, lz, _, ch_max = PARAMS[level_]
        found = m < lz and c <= ((ch_max >> 2) if m >= g else ch_max)
        if found:
            return tk.at(p) == (len2, p - ql) and tk.literal(p - 1)
        return tk.at(p - 1) == (m, p - 1 - qm)
    name = f"quarter_L{level}_depth{c}_prev{m}_{kind}" + ("_lane" if tuned else "")
    return Case("sorted" if tuned else "quarter", name, data, census, levels=(level,))


def _nice_cases():
    """6. the first entry reaching min(nice_match, lookahead) ends the walk"""
    out = []
    for level in LEVELS:
        nice = PARAMS[level][2]
        for n in (nice - 1, nice, nice + 1):
            if n > MAX_MATCH:
                continue
            far = min(n + 5, MAX_MATCH)
            b = Build()
            b.fill(8)
            b.put([G[0]])
            qf = b.put(probe(far))
            b.put([E[0]])
            b.fill(6)
            b.put([G[1]])
            qn = b.put(probe(n))
            b.put([E[1]])
            b.fill(6)
            b.put([SEP])
            p = b.put(probe(far + 2))
            b.fill(400)
            data = b.bytes()

            def census(tk, level_, strategy=0, mem_level=8, data=data, p=p, qf=qf, qn=qn, n=n, far=far):
                if chain(data, p, _hash_bits(mem_level)) != [qn, qf]:
                    return False
                nc = PARAMS[level_][2]
                return tk.at(p) == ((n, p - qn) if n >= nc or far <= n else (far, p - qf))
            out.append(Case("nice", f"nice_L{level}_near{n}_far{far}", data, census, levels=(level,)))
    # lookahead below nice: a candidate as long as the lookahead ends the walk
    for look in (5, 10, 15):
        b = Build()
        b.fill(8)
        b.put([G[0]])
        qf = b.put(probe(look + 4))
        b.put([E[0]])
        b.fill(6)
        b.put([G[1]])
        qn = b.put(probe(look))
        b.put([E[1]])
        b.fill(300)
        b.put([SEP])
        p = b.put(probe(look))
        data = b.bytes()

        def census(tk, level_, strategy=0, mem_level=8, data=data, p=p, qf=qf, qn=qn, look=look):
            return chain(data, p, _hash_bits(mem_level)) == [qn, qf] and tk.at(p) == (look, p - qn) and len(data) == p + look
        out.append(Case("nice", f"nice_lookahead{look}", data, census))
    return out


def _lazy_cases():
    """7. prev_length >= max_lazy suppresses the search; deferral chains"""
    out = []
    mat = body()
    for level in LEVELS:
        lazy = PARAMS[level][1]
        for m in (lazy - 1, lazy):
            if m + 2 > MAX_MATCH and m < lazy:
                longer = MAX_MATCH
            else:
                longer = m + 2
            if m >= MAX_MATCH:
                continue  # level 9: nothing is longer than 258
            c = mat[1000:1000 + m + 8]  # data[p:] = c
            b = Build()
            b.fill(8)
            b.put([G[0]])
            q1 = b.put(c[1:1 + longer])           # what p + 1 finds
            b.put([E[0]])
            b.fill(6)
            b.put([G[1]])
            q0 = b.put(c[:m])                     # what p finds
            b.put([E[1]])
            b.fill(6)
            b.put([SEP])
            p = b.put(c[:1 + longer])
            b.put([E[2]])
            b.fill(400)
            data = b.bytes()

            def census(tk, level_, strategy=0, mem_level=8, p=p, q0=q0, q1=q1, m=m, longer=longer):
                if m < PARAMS[level_][1]:
                    return tk.literal(p) and tk.at(p + 1) == (longer, p + 1 - q1)
                return tk.at(p) == (m, p - q0)
            out.append(Case("lazy", f"lazy_L{level}_len{m}", data, census, levels=(level,)))
    # deferral chains: p finds 5, p + 1 finds 6, ... ; with max_lazy 4 (level 4) the first one is taken
    for steps, at in ((2, None), (3, None), (3, 62), (3, 63), (2, 63), (3, 61)):
        c = mat[2000:2000 + 5 + 3 * steps]
        b = Build()
        b.fill(8)
        olds = []
        for k in range(steps, -1, -1):
            b.put([G[k & 1]])
            olds.append((k, b.put(c[k:k + 5 + k + k])))  # c[k:] over 5 + k bytes ... see census
            b.put([E[k % 3]])
            b.fill(5)
        if at is not None:
            b.fill_to((len(b) // REC_BLOCK + 2) * REC_BLOCK + at - 1)
        b.put([SEP])
        p = b.put(c)
        b.put([E[(steps + 1) % 3]])
        b.fill(400)
        data = b.bytes()
        olds = dict(olds)

        def census(tk, level_, strategy=0, mem_level=8, p=p, olds=olds, steps=steps, at=at):
            if at is not None and p % REC_BLOCK != at:
                return False
            if PARAMS[level_][1] <= 5:
                return tk.at(p) == (5, p - olds[0])
            # the old copy for p + k starts at c[k] and is 5 + 2k bytes long: each step is two bytes longer than the last
            return tk.literal(p, steps) and tk.at(p + steps) == (5 + 2 * steps, p + steps - olds[steps])
        out.append(Case("lazy", f"lazy_chain{steps}" + (f"_at{at}mod64" if at is not None else ""), data, census))
    return out


def _far_cases():
    """8. a 3-byte match further than TOO_FAR is dropped; Z_FILTERED needs six bytes"""
    out = []
    for n, dist in ((3, TOO_FAR - 1), (3, TOO_FAR), (3, TOO_FAR + 1), (4, TOO_FAR + 1), (4, TOO_FAR)):
        b = Build()
        b.fill(8)
        b.put([G[0]])
        q = b.put(probe(n))
        b.put([E[0]])
        b.fill_to(q + dist - 1)
        b.put([G[1]])
        p = b.put(probe(n))
        b.put([E[1]])
        b.fill(400)
        data = b.bytes()

        def census(tk, level, strategy=0, mem_level=8, data=data, p=p, q=q, n=n, dist=dist):
            if chain(data, p, _hash_bits(mem_level)) != [q]:
                return False
            keep = (n > 3 or dist <= TOO_FAR) and (strategy != Z_FILTERED or n > 5)
            return tk.at(p) == (n, dist) if keep else tk.literal(p, n)
        out.append(Case("far", f"far_len{n}_d{dist}", data, census, strategies=(0, Z_FILTERED)))
    for n in (3, 4, 5, 6, 7):
        b = Build()
        b.fill(8)
        b.put([G[0]])
        q = b.put(probe(n))
        b.put([E[0]])
        b.fill(50)
        b.put([G[1]])
        p = b.put(probe(n))
        b.put([E[1]])
        b.fill(400)
        data = b.bytes()

        def census(tk, level, strategy=0, mem_level=8, data=data, p=p, q=q, n=n):
            if chain(data, p, _hash_bits(mem_level)) != [q]:
                return False
            return tk.at(p) == (n, p - q) if (strategy != Z_FILTERED or n > 5) else tk.literal(p, n)
        out.append(Case("far", f"filtered_len{n}", data, census, strategies=(0, Z_FILTERED)))
    return out


def _end_cases():
    """9. lengths are capped by the end of the input; the last positions of a slice"""
    out = []
    for n in (9, 8, 7, 6, 5, 4, 3):  # the plant starts at L - n and ends at L
        b = Build()
        b.fill(8)
        b.put([G[0]])
        q = b.put(probe(9))
        b.put([E[0]])
        b.fill(200)
        b.put([G[1]])
        p = b.put(probe(n))
        data = b.bytes()

        def census(tk, level, strategy=0, mem_level=8, data=data, p=p, q=q, n=n):
            return len(data) == p + n and chain(data, p, _hash_bits(mem_level)) == [q] and tk.at(p) == (n, p - q)
        out.append(Case("end", f"end_plant_at_L-{n}", data, census))
    for n in (4, 9):  # one byte short of the end, and the plant cut by the end
        b = Build()
        b.fill(8)
        b.put([G[0]])
        q = b.put(probe(12))
        b.put([E[0]])
        b.fill(200)
        b.put([G[1]])
        p = b.put(probe(12)[:n])
        b.put([E[1]] if n == 4 else [])
        data = b.bytes()

        def census(tk, level, strategy=0, mem_level=8, data=data, p=p, q=q, n=n):
            return tk.at(p) == (n, p - q) and len(data) - (p + n) == (1 if n == 4 else 0)
        out.append(Case("end", f"end_cut_len{n}", data, census))
    for n in (258, 259):
        b = Build()
        b.fill(8)
        b.put([G[0]])
        q = b.put(probe(n))
        b.put([E[0]])
        b.fill(60)
        b.put([G[1]])
        p = b.put(probe(n))
        b.put([E[1]])
        b.fill(300 if n == 258 else 0)
        data = b.bytes()

        def census(tk, level, strategy=0, mem_level=8, data=data, p=p, q=q, n=n):
            if tk.at(p) != (258, p - q):
                return False
            return tk.literal(p + 258) if n == 258 else tk.literal(p + 258, 2) and len(data) == p + 260
        out.append(Case("end", f"end_repeat{n}", data, census))
    # the same 258-byte repeat ending exactly at L
    b = Build()
    b.fill(8)
    b.put([G[0]])
    q = b.put(probe(258))
    b.put([E[0]])
    b.fill(60)
    b.put([G[1]])
    p = b.put(probe(258))
    data = b.bytes()
    out.append(Case("end", "end_repeat258_at_L", data,
                    lambda tk, level, strategy=0, mem_level=8, p=p, q=q: tk.at(p) == (258, p - q)))
    mid = b"\xa7\x21\x22\x23"
    tiny = [("L3", T, []), ("L4", T + T[:1], []), ("L4_run", b"\x05" * 4, []),
            ("L8", b"\x67" + T + mid[:1] + T, [(5, 3, 4)]), ("L9", b"\x67" + T + mid[:2] + T, [(6, 3, 5)]),
            ("L10", b"\x67" + T + mid[:3] + T, [(7, 3, 6)]),
            ("L8_nil", T + mid[:2] + T, []), ("L9_nil", T + mid[:3] + T, []), ("L10_nil", T + mid + T, [])]
    for name, data, want in tiny:  # the _nil ones: the only candidate is position 0
        out.append(Case("end", f"end_{name}", data,
                        lambda tk, level, strategy=0, mem_level=8, want=want: tk.toks == want))
    return out


RUN = 0xE0  # the run byte: the only class-0 byte of a run input, so the bucket of (RUN, RUN, RUN) holds run strings only
SEPS = (0x27, 0x47, 0x07, 0x67)


def _run(r):
    return bytes([RUN]) * r


def _cont(n=12):
    return body()[3000:3000 + n]


def _run_input(parts, tail=300):
    """parts: int = that many filler bytes, ('to', pos) = filler up to pos, bytes = a plant.  -> (data, plant positions)"""
    b = Build()
    pos = []
    for part in parts:
        if isinstance(part, int):
            b.fill(part)
        elif isinstance(part, tuple):
            b.fill_to(part[1])
        else:
            pos.append(b.put(part))
    b.fill(tail)
    return b.bytes(), pos


def _short_runs(k):
    """k entries of the run bucket from short runs: a run of nine holds seven strings of three equal bytes, a run of three one"""
    out, i = bytearray(), 0
    while k:
        n = 7 if k >= 7 else 1
        out += _run(n + 2) + bytes([SEPS[i % 4]])
        k, i = k - n, i + 1
    return bytes(out)


def _lone_run_census(data, s, r, tk, level, strategy=0, mem_level=8):
    """a run of r with no earlier run: a literal, then distance-1 matches of at most 258; what is left below 3 is literals"""
    if data[s:s + r] != _run(r) or (s and data[s - 1] == RUN) or (s + r < len(data) and data[s + r] == RUN):
        return False
    if chain(data, s, _hash_bits(mem_level)):
        return False
    first = 2 if s == 0 else s + 1  # position 0 is NIL: a run at the start of the input is matched from its third byte
    q, left = first, s + r - first
    if not tk.literal(s, first - s):
        return False
    while left >= 3:
        n = min(left, MAX_MATCH)
        if tk.at(q) != (n, 1):
            return False
        q, left = q + n, left - n
    return tk.literal(q, left)


def _prev_run_census(data, q, p, r0, r, same, tk, level, strategy=0, mem_level=8):
    """an earlier run of r0 at q, the run of r at p; `same`: twelve equal bytes follow both"""
    good, lazy, nice, mc = PARAMS[level]
    ch = chain(data, p, _hash_bits(mem_level))
    if ch != list(range(q + r0 - 3, q - 1, -1)) or tk.at(q + 1) != (min(r0 - 1, MAX_MATCH), 1):
        return False
    t = tk.at(p)
    if r0 >= nice and (r > nice or nice == MAX_MATCH <= r):
        # the walk ends at the first string that reaches nice: nice bytes, no extension (nice - 2 <= max_chain at every level)
        return t == (nice, p - (q + r0 - nice))
    if r0 >= r and r + 12 < MAX_MATCH and r - 2 <= mc:  # the string with r run bytes left is reached: the extension counts
        return t is not None and t[1] == p - (q + r0 - r) and t[0] in ((r + 12, r + 13) if same else (r,))
    if r0 < r <= MAX_MATCH and r0 < lazy and r0 - 2 <= mc:  # the whole earlier run, then the distance-1 match is longer
        return tk.literal(p) and tk.at(p + 1) == (r - 1, 1)
    return tk.covering(p + 1) is not None


def _far_run_census(data, q, p, mid, dist, tk, level, strategy=0, mem_level=8):
    """the earlier run's first string is the only one that matches all 12 + 4 bytes, at `dist` from p; with an entry in
    between or at MAX_DIST as a non-head it is out of reach and p makes do with the 11 run bytes one position closer"""
    ch = chain(data, p, _hash_bits(mem_level))
    if ch[-1] != q or p - q != dist or (mid is not None and ch[0] != mid) or (mid is None and ch[0] != q + 9):
        return False
    reach = dist < MAX_DIST and len(ch) <= PARAMS[level][3]
    if reach and PARAMS[level][2] > 11:
        return tk.at(p) == (16, dist)
    return tk.at(p) is not None and tk.at(p)[1] < dist


def _run_budget_input(level, needed, quarter):
    good = PARAMS[level][0]
    if quarter:  # a match of `good` bytes at p - 1, the run of four and good + 2 more bytes at p
        c = _cont(good + 2)
        parts = [20, bytes([G[0]]) + _run(4) + c + bytes([E[0]]), 3, _short_runs(needed - 4), 3,
                 bytes([W]) + _run(4) + c[:good - 5] + bytes([E[1]]), 4, bytes([W]), _run(4) + c + bytes([E[2]])]
    else:
        c = _cont(6)
        parts = [20, bytes([G[0]]) + _run(12) + c + bytes([E[0]]), 3, _short_runs(needed - 10), 3,
                 bytes([G[1]]), _run(12) + c + bytes([E[2]])]
    data, pos = _run_input(parts)
    return data, pos[0] + 1, pos[-1], (pos[-3] if quarter else None)


def _run_budget_census(data, far, p, qm, level, needed, quarter, tk, level_, strategy=0, mem_level=8):
    """qmin4 / qmin1: the first string of the far run, the only one with the extension, is chain entry `needed`"""
    good, lazy, nice, mc = PARAMS[level]
    ch = chain(data, p, _hash_bits(mem_level))
    if len(ch) != needed or ch[-1] != far or data[p - 1] == RUN:
        return False
    if quarter:
        if needed <= mc >> 2:
            return tk.literal(p - 1) and tk.at(p) == (good + 6, p - far)
        return tk.at(p - 1) == (good, p - 1 - qm)
    if needed <= mc:
        return tk.at(p) == (18, p - far)
    return tk.at(p) == (11, p - far - 1)  # the cut falls one string short: eleven run bytes of the far run


def _run_cases():
    """10. strings of equal bytes: dfl_run_len / dfl_run_lists / dfl_run_info / dfl_match_run"""
    out = []

    def lone(name, data, s, r):
        out.append(Case("runs", name, data, functools.partial(_lone_run_census, data, s, r), runs=True))

    for s in (0, 1, 2):
        data, _ = _run_input([s, _run(10)])
        lone(f"run_start{s}", data, s, 10)
    for r in (3, 4, 5, 257, 258, 259, 260, 261, 262, 510, 511, 512, 513, 600):
        data, (s,) = _run_input([100, _run(r)])
        lone(f"run_len{r}", data, s, r)
    for edge in (RUNLEN_OUT - 1, RUNLEN_OUT, RUNLEN_OUT + 1, 2 * RUNLEN_OUT - 1, 2 * RUNLEN_OUT, 2 * RUNLEN_OUT + 1):
        data, (s,) = _run_input([("to", edge), _run(40)])
        lone(f"run_starts_at{edge}", data, s, 40)
        data, (s,) = _run_input([("to", edge - 40), _run(40)])
        lone(f"run_ends_at{edge}", data, s, 40)
    for edge, r in ((RUNLEN_OUT, 40), (RUNLEN_OUT, 600), (2 * RUNLEN_OUT, 40), (2 * RUNLEN_OUT, 520)):
        data, (s,) = _run_input([("to", edge - r // 2), _run(r)])
        lone(f"run_straddles{edge}_len{r}", data, s, r)
    data, (s,) = _run_input([("to", RUNLEN_OUT - 100), _run(2 * RUNLEN_OUT)])
    lone("run_over_three_chunks", data, s, 2 * RUNLEN_OUT)
    lone("run_whole_input", _run(700), 0, 700)
    data, (s,) = _run_input([50, _run(300)], tail=0)
    lone("run_to_the_end", data, s, 300)

    # an earlier run of the same byte: longer, equal, shorter; the same or another continuation; r below, at and above
    # the 258 of a match and the 511 of the run-info word
    cont = _cont()
    for r in (20, 258, 300, 511, 520):
        for r0 in (r - 7, r, r + 7):
            for same in (True, False):
                c0 = cont if same else bytes([cont[0] ^ 0x80]) + cont[1:]
                data, (q, p) = _run_input([20, _run(r0) + c0, 40, _run(r) + cont])
                out.append(Case("runs", f"run_prev{r0}_then{r}_{'same' if same else 'other'}_cont", data,
                                functools.partial(_prev_run_census, data, q, p, r0, r, same), runs=True))
    # nice < r
    for level in (4, 5, 6, 7):
        nice = PARAMS[level][2]
        for r in (nice + 1, nice + 40):
            for r0 in (nice - 1, nice, r, r + 3):
                data, (q, p) = _run_input([20, _run(r0) + cont, 40, _run(r) + cont])
                out.append(Case("runs", f"run_nice_L{level}_prev{r0}_then{r}", data,
                                functools.partial(_prev_run_census, data, q, p, r0, r, True), levels=(level,), runs=True))

    # the earlier run at MAX_DIST - 1 / MAX_DIST from a run start with no equal byte before it
    for dist in (MAX_DIST - 1, MAX_DIST):
        for between in (False, True):
            parts = [30, _run(12) + cont[:4] + bytes([E[0]])]
            if between:
                parts += [500, _run(3) + bytes([E[1]])]
            data, pos = _run_input(parts + [("to", 30 + dist), _run(12) + cont[:4] + bytes([E[2]])], tail=400)
            q, p = pos[0], pos[-1]
            out.append(Case("runs", f"run_prev_at_d{dist}" + ("_entry_between" if between else ""), data,
                            functools.partial(_far_run_census, data, q, p, pos[1] if between else None, dist), runs=True))

    # the same with runs of three: the earlier run is one string, the head of p's chain, at MAX_DIST - 1, MAX_DIST, MAX_DIST + 1
    for dist in (MAX_DIST - 1, MAX_DIST, MAX_DIST + 1):
        data, (q, p) = _run_input([30, _run(3) + cont[:4] + bytes([E[0]]), ("to", 30 + dist), _run(3) + cont[:4] + bytes([E[2]])],
                                  tail=400)

        def census(tk, level, strategy=0, mem_level=8, data=data, q=q, p=p, dist=dist):
            if chain(data, p, _hash_bits(mem_level)) != [q] or p - q != dist:
                return False
            return tk.at(p) == (7, dist) if dist <= MAX_DIST else tk.at(p) is None
        out.append(Case("runs", f"run3_head_at_d{dist}", data, census, runs=True))

    # more strings of one byte than the chain budget: the cut falls inside an earlier run (qmin4), and after a match of
    # `good` bytes at p - 1 inside the quarter budget (qmin1)
    for level in LEVELS:
        mc = PARAMS[level][3]
        for needed in (mc - 1, mc, mc + 1):
            data, far, p, _ = _run_budget_input(level, needed, False)
            out.append(Case("runs", f"run_budget_L{level}_entry{needed}", data,
                            functools.partial(_run_budget_census, data, far, p, None, level, needed, False),
                            levels=(level,), runs=True))
        if level >= 5:
            for needed in ((mc >> 2) - 1, mc >> 2, (mc >> 2) + 1):
                data, far, p, qm = _run_budget_input(level, needed, True)
                out.append(Case("runs", f"run_quarter_L{level}_entry{needed}", data,
                                functools.partial(_run_budget_census, data, far, p, qm, level, needed, True),
                                levels=(level,), runs=True))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = (_window_cases() + _nil_cases() + _chain_cases() + _nice_in_step_cases() + _quarter_cases() + _nice_cases()
           + _lazy_cases() + _far_cases() + _end_cases() + _run_cases())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def family_counts():
    counts = {}
    for c in cases():
        counts[c.family] = counts.get(c.family, 0) + 1
    return counts
