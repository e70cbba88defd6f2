"""Inputs for the symbol walk of the device INFLATE (walk_segment in inflate_kernels.hip): the longest symbol DEFLATE has, a
length with 5 extra bits and a distance with 13 on 15-bit codes (48 bits), placed where the walk's input reads change: at
every bit offset of a dword, at every fill of the lane's bit buffer, across a segment end, in front of the end of the
batch's input, across the wrap of the staged window, and as a refusal.  Built with tests/deflate_streams.py; CPython's zlib is
the judge of every stream.  `device_walk` models how the kernel's lanes come by the symbols of a stream (the true chain of
every round: which lane decodes a symbol, in a literal-only step or in the general step, and with how many valid bits in its
buffer), so that every case carries a precondition on the path it is meant to reach.  Test infrastructure only.
Pure Python + numpy + zlib."""
import collections
import functools

import numpy as np

import deflate_streams as ds

# ---- the kernel's walk constants (tests/test_inflate_walk_inputs_host.py reads them out of inflate_kernels.hip) -----------
FAST_STEPS = 3
INF_IN = {256: 16384, 512: 32768}
ROUND_IN_SLACK = 32
SYM_BITS = 48
WALK_MIN_BITS = 33 - ds.LL_BITS

# ---- alphabets: the ladder 1 .. 14, 15, 15 (complete) on sixteen symbols ------------------------------------------------------
LITS = tuple(b"etaoinshrdlu")           # literals with codes of 1 .. 12 bits
LIT_X1, LIT_X2 = ord("q"), ord("z")     # the literals on the long codes that are left
LEN_SYM, LEN_BASE = 281, 131            # a length symbol with 5 extra bits
DIST_SYM, DIST_BASE = 28, 16385         # a distance symbol with 13 extra bits


def _ladder(n, order):
    lens = [0] * n
    for ln, s in zip(ds.LADDER, order):
        lens[s] = ln
    assert ds.code_set(lens) is None
    return lens


# case 1: both codes 15 bits long.  case 3: the shortest codes that miss both root tables (LL_BITS + 1, D_BITS + 1)
LL_48 = _ladder(282, list(LITS) + [ds.EOB, LIT_X1, LEN_SYM, LIT_X2])
D_48 = _ladder(30, list(range(14)) + [DIST_SYM, 29])
LL_MISS = _ladder(282, list(LITS) + [LEN_SYM, ds.EOB, LIT_X1, LIT_X2])
D_MISS = _ladder(30, list(range(10)) + [DIST_SYM, 10, 11, 12, 13, 29])
assert LL_48[LEN_SYM] == 15 and D_48[DIST_SYM] == 15 and LL_MISS[LEN_SYM] == ds.LL_BITS + 1 and D_MISS[DIST_SYM] == ds.D_BITS + 1
PAIR_BITS_48 = 15 + 5 + 15 + 13
PAIR_BITS_MISS = (ds.LL_BITS + 1) + 5 + (ds.D_BITS + 1) + 13
D_ONE = [0] * DIST_SYM + [1]            # the single one-bit distance code: its other code names no symbol


def pair(lx, dx):
    return ("ld", LEN_SYM, lx, DIST_SYM, dx)


def lead_in():
    """16 514 bytes in 106 bytes of stream: the history a distance of 16 385 and more needs; two blocks, so that no lane comes near
    LANE_OUT_CAP"""
    return [ds.fixed([7] + [ds.copy(258, 1)] * 32), ds.fixed([9] + [ds.copy(258, 1)] * 32)]


LEAD_OUT = 2 * (1 + 32 * 258)


def pad(nbits, rng, tail=()):
    """literals whose codes take nbits in all and end with codes of the lengths `tail`"""
    n = nbits - sum(tail)
    assert n >= 0
    out = []
    while n > 12:
        ln = int(rng.integers(5, 13))
        out.append(LITS[ln - 1])
        n -= ln
    if n:
        out.append(LITS[n - 1])
    return out + [LITS[ln - 1] for ln in tail]


def _body_start(ll, d, head):
    """bit offset of the first body symbol of the dynamic block behind `head` (the header depends on the lengths alone)"""
    w = ds.walk(ds.zlib_stream(head + [ds.dynamic(ll, d, [], final=True)]))
    assert w["error"] is None
    return w["blocks"][-1]["body"]


def expand(blocks):
    """ds.expand for blocks that hold ("ld", ...) items"""
    out = bytearray()
    for b in blocks:
        if b["type"] == 0:
            out += b["data"]
            continue
        for it in b["body"]:
            if isinstance(it, (int, np.integer)):
                out.append(int(it))
                continue
            if it[0] == "m":
                n, dist = it[1], it[2]
            else:
                n, dist = ds.LBASE[it[1] - 257] + it[2], ds.DBASE[it[3]] + it[4]
            assert 1 <= dist <= len(out)
            for _ in range(n):
                out.append(out[-dist])
    return bytes(out)


# ---- model of the device's walk ---------------------------------------------------------------------------------------------
Step = collections.namedtuple("Step", "bit kind bits cnt next merges lane end round block")
# one general step of the true chain: bit (in the stream), kind ("lit", "len", "eob", "bad"), bits the symbol takes, cnt = valid
# bits in the lane's buffer and next = dword (from the 16-byte aligned base of the stream) it would merge, both on entry;
# merges = dwords merged in the step; end = where the lane's segment ends


def _len_parts(s, total):
    """(literal/length bits, distance bits) of a copy that takes `total` bits"""
    lx = 0 if s.length == 258 and total - s.nbits - s.dbits < 5 else ds.length_symbol(s.length)[1]
    return s.nbits + lx, total - s.nbits - lx


@functools.lru_cache(maxsize=4)
def host_walk(stream):
    return ds.walk(stream)


def device_walk(stream, nt, align=0):
    """[Step] of every round of every Huffman block: the walks the device's emit pass makes (lane t starts where lane t - 1
    landed).  align = offset of the stream in the batch modulo 16.  Models walk_segment: FAST_STEPS literal-only steps, each
    merging a dword at cnt <= 32 and taking one literal or a pair (second literal only if it starts before `end`, both codes
    within LL_BITS), then the exit test, then a general step with its three merges; and the round loop's cut at the first lane
    whose output or copies exceed ROUND_OUT_BUDGET / MLIST_CAP (that lane opens the next round).  Asserts that no lane comes to
    LANE_OUT_CAP, which it does not model."""
    w = host_walk(stream)
    steps = []
    for bi, blk in enumerate(w["blocks"]):
        if blk["type"] == 0 or "body" not in blk:
            continue
        syms = blk["syms"]
        at = {s.bit: k for k, s in enumerate(syms)}

        def total(k):
            return (syms[k + 1].bit if k + 1 < len(syms) else blk.get("end", syms[k].bit + syms[k].nbits)) - syms[k].bit

        def literals(p, end):
            """bits and bytes of the root entry at p when it is a literal entry"""
            k = at.get(p)
            if k is None or syms[k].kind != "lit" or syms[k].nbits > ds.LL_BITS:
                return 0, 0
            l1 = syms[k].nbits
            k2 = at.get(p + l1)
            if k2 is not None and syms[k2].kind == "lit" and l1 + syms[k2].nbits <= ds.LL_BITS and p + l1 < end:
                return l1 + syms[k2].nbits, 2
            return l1, 1

        origin, rnd, flag = blk["body"], 0, None
        while flag is None:
            p, cb, cm = origin, 0, 0
            for t in range(nt):
                end = origin + (t + 1) * ds.SEG_BITS
                p0, n_steps = p, len(steps)
                a = p + 8 * align
                cnt, nxt, nb, nm = 64 - (a & 31), (a >> 5) + 2, 0, 0
                while True:
                    for _ in range(FAST_STEPS):
                        if cnt <= 32:
                            cnt, nxt = cnt + 32, nxt + 1
                        assert cnt >= WALK_MIN_BITS
                        used, n = literals(p, end) if p < end else (0, 0)
                        cnt, p, nb = cnt - used, p + used, nb + n
                    if p >= end:
                        break
                    assert nb < ds.LANE_OUT_CAP and WALK_MIN_BITS <= cnt <= 64
                    c0, n0, merges = cnt, nxt, 0
                    if cnt <= 32:
                        cnt, nxt, merges = cnt + 32, nxt + 1, merges + 1
                    k = at.get(p)
                    if k is None:  # the walk stopped here: no such literal/length code, or a distance code that names nothing
                        assert p == w["error_bit"]
                        steps.append(Step(p, "bad", 0, c0, n0, merges, t, end, rnd, bi))
                        flag = "bad"
                        break
                    s, tb = syms[k], total(k)
                    if s.kind == "lit":
                        used, n = literals(p, end)
                        if not used:
                            used, n = s.nbits, 1  # a literal on a code longer than the root table
                        cnt, p, nb = cnt - used, p + used, nb + n
                    elif s.kind == "eob":
                        steps.append(Step(p, "eob", tb, c0, n0, merges, t, end, rnd, bi))
                        p += s.nbits
                        flag = "eob"
                        break
                    else:
                        lb, db = _len_parts(s, tb)
                        cnt -= lb
                        if cnt <= 32:
                            cnt, nxt, merges = cnt + 32, nxt + 1, merges + 1
                        assert cnt >= db
                        cnt, nb, nm = cnt - db, nb + s.length, nm + 1
                        if s.dist > s.out:
                            steps.append(Step(p, "bad", tb, c0, n0, merges, t, end, rnd, bi))
                            flag = "bad"
                            break
                        p += tb
                    if cnt <= 32:
                        cnt, nxt, merges = cnt + 32, nxt + 1, merges + 1
                    assert merges <= 2 and nxt * 32 - cnt == p + 8 * align
                    steps.append(Step(s.bit, s.kind, tb if s.kind == "len" else used, c0, n0, merges, t, end, rnd, bi))
                cb, cm = cb + nb, cm + nm
                if t and (cb > ds.ROUND_OUT_BUDGET[nt] or cm > ds.MLIST_CAP):  # the round ends in front of this lane
                    del steps[n_steps:]
                    p, flag = p0, None
                    break
                if flag:
                    break
            origin, rnd = p, rnd + 1
        if flag == "bad":
            break
    return steps


def fill_class(cnt):
    """the three fills of the buffer on entry to a general step: the least there can be, a dword boundary just crossed, no merge"""
    return "min" if cnt == WALK_MIN_BITS else "low" if cnt <= 32 else "high"


def pair_steps(stream, nt, align=0, bits=PAIR_BITS_48):
    return [s for s in device_walk(stream, nt, align) if s.kind == "len" and s.bits == bits]


# ---- cases ------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name group accept stream pre")
# group: 1 .. 6 as the cases are numbered above; pre(stream) asserts, from the host walk and the model, that the stream reaches
# its path, and returns a line for the test's output
_CASES = []


def case(name, group, accept=True):
    def reg(fn):
        @functools.lru_cache(maxsize=None)
        def build():
            stream, pre = fn()
            return Case(name, group, accept, stream, pre)
        _CASES.append((name, build))
        return build
    return reg


def cases(group=None):
    return [b() for _, b in _CASES if group is None or b().group == group]


# literals in front of the pair, by the lengths of their codes: what the buffer holds when the general step finds the pair
TAILS = ((12,), (6, 6), (12, 12, 12), (1, 11), (7, 9, 12), (1, 1, 1))
# The fill on entry to a general step is low only if the third literal-only step before it took its literal without a merge.  A
# copy is always taken by a general step, whose last merge leaves cnt = 64 - (a mod 32) valid bits at the bit a where the copy
# ends.  Three literals that cannot pair up (7 + 7 > LL_BITS) are then one literal-only step each: 7, 7 and 12 bits after a copy
# that ends at a = 6 + ph (mod 32) go 58 - ph -> 51 - ph -> 44 - ph -> 32 - ph without a merge for ph = 0 .. 11, and the symbol
# behind them starts at bit ph (mod 32) with 32 - ph valid bits: ph = 11 is the least there can be (WALK_MIN_BITS).
FILL_TAIL = (7, 7, 12)
FILL_REPS = 3  # a segment end between the two copies gives the second one to a fresh lane: more than one try per phase


def _sweep(ll, d, tails, seed, offsets=range(64)):
    """lead-in + one dynamic block.  For every tail and every offset: a pad that ends with the tail, then the pair at that bit
    offset modulo 64 of the stream.  Then, FILL_REPS times for every bit a modulo 32: a pair that ends there, FILL_TAIL, a pair."""
    rng = np.random.default_rng(seed)
    head = lead_in()
    pos = _body_start(ll, d, head)
    pbits = ll[LEN_SYM] + 5 + d[DIST_SYM] + 13
    body, want = [], []

    def put(n, tail):
        nonlocal pos
        body.extend(pad(n, rng, tail) + [pair(int(rng.integers(0, 32)), int(rng.integers(0, 100)))])
        want.append(pos + n)
        pos += n + pbits

    for tail in tails:
        for off in offsets:
            n = sum(tail) + int(rng.integers(0, 40))
            put(n + (off - pos - n) % 64, tail)
    for rep in range(FILL_REPS):
        for a in range(32):
            n = int(rng.integers(0, 30))
            put(n + (a - pbits - pos - n) % 32, ())
            put(sum(FILL_TAIL), FILL_TAIL)
    blocks = head + [ds.dynamic(ll, d, body + list(LITS), final=True)]
    return ds.zlib_stream(blocks, data=expand(blocks)), want, pbits


def _pre_sweep(want, pbits):
    def pre(stream):
        w = host_walk(stream)
        assert w["error"] is None
        got = [s.bit for s in w["blocks"][-1]["syms"] if s.kind == "len"]
        syms = w["blocks"][-1]["syms"]
        assert got == want and all(b.bit - a.bit == pbits for a, b in zip(syms, syms[1:]) if a.kind == "len")
        assert {b % 64 for b in got} == set(range(64))
        fills = set()
        for nt in ds.LANES:
            for align in range(4):
                st = pair_steps(stream, nt, align, pbits)
                assert [s.bit for s in st] == want  # every pair is met by a general step of the true chain
                assert {(s.bit + 8 * align) % 32 for s in st} == set(range(32))
                here = {s.cnt for s in st}
                # the least fill, a dword boundary just crossed, no merge at the top
                assert here >= {WALK_MIN_BITS, 29, 30, 31, 32} and max(here) > 32, (nt, align, sorted(here))
                assert {s.merges for s in st} == {1, 2}
                fills |= here
        return f"{len(got)} symbols of {pbits} bits at every offset modulo 64; valid bits on entry {min(fills)} .. {max(fills)}"
    return pre


@case("pair_48_bits_at_every_phase", 1)
def _():
    stream, want, pbits = _sweep(LL_48, D_48, TAILS, 101)
    assert pbits == SYM_BITS
    return stream, _pre_sweep(want, pbits)


@case("pair_on_codes_that_miss_both_roots_at_every_phase", 3)
def _():
    stream, want, pbits = _sweep(LL_MISS, D_MISS, TAILS, 103)
    assert pbits == PAIR_BITS_MISS
    return stream, _pre_sweep(want, pbits)


@case("pair_48_bits_across_every_segment_end", 2)
def _():
    rng = np.random.default_rng(102)
    head = lead_in()
    b0 = _body_start(LL_48, D_48, head)
    body, pos, want = [], b0, []
    for j in range(1, SYM_BITS):
        tail = TAILS[j % len(TAILS)]
        seg = (pos - b0 + sum(tail) + j) // ds.SEG_BITS + 1  # the next segment end the pair can start j bits before
        n = b0 + seg * ds.SEG_BITS - j - pos
        body += pad(n, rng, tail) + [pair(int(rng.integers(0, 32)), int(rng.integers(0, 100)))]
        want.append((pos + n, b0 + seg * ds.SEG_BITS))
        pos += n + SYM_BITS
    blocks = head + [ds.dynamic(LL_48, D_48, body + list(LITS), final=True)]

    def pre(stream):
        assert ds.walk(stream)["error"] is None
        for nt in ds.LANES:
            for align in range(4):
                st = pair_steps(stream, nt, align)
                assert [(s.bit, s.end) for s in st] == want and all(s.round == 0 for s in st)
                assert sorted(s.end - s.bit for s in st) == list(range(1, SYM_BITS))  # the lane lands end - bit bits short of 48 past `end`
        return f"{len(want)} pairs start 1 .. {SYM_BITS - 1} bits before a multiple of SEG_BITS in the block's first round"
    return ds.zlib_stream(blocks, data=expand(blocks)), pre


def _last_symbol_case(k):
    @case(f"pair_48_bits_is_the_last_symbol_{k}", 4)
    def _():
        rng = np.random.default_rng(140 + k)
        tail = TAILS[k % len(TAILS)]
        blocks = lead_in() + [ds.dynamic(LL_48, D_48, pad(sum(tail) + 5 * k, rng, tail) + [pair(3 + k, 17 * k)], final=True)]

        def pre(stream):
            w = ds.walk(stream)
            syms = w["blocks"][-1]["syms"]
            assert w["error"] is None and len(w["blocks"]) == 3
            assert syms[-1].kind == "eob" and syms[-2].kind == "len" and syms[-1].bit - syms[-2].bit == SYM_BITS
            tr = w["trailer"] // 8 + 4
            assert tr == len(stream)
            for nt in ds.LANES:
                st = pair_steps(stream, nt)
                assert len(st) == 1
                # the two dwords asked for at the pair's general step reach behind the DEFLATE data, into the trailer or past it
                assert (st[0].next + 2) * 4 > w["trailer"] // 8
            return f"pair at bit {syms[-2].bit}, stream of {len(stream)} bytes, fill {st[0].cnt}, dwords asked for end " \
                   f"{(st[0].next + 2) * 4 - len(stream)} bytes past the stream"
        return ds.zlib_stream(blocks, data=expand(blocks)), pre


for _k in range(8):
    _last_symbol_case(_k)

WRAP_VARIANTS = 8


def _wrap_case(v):
    @case(f"pair_48_bits_across_the_window_wrap_{v}", 5)
    def _():
        # literals on the long codes up to a stretch of pairs around every multiple of 16 KiB of the stream; the variants shift
        # the stretch bit by bit so that some pair of the group finds `next` on the last dword before the wrap
        rng = np.random.default_rng(150 + v)
        head = lead_in()
        b0 = _body_start(LL_48, D_48, head)
        body, pos = [], b0
        for wrap in (INF_IN[256], INF_IN[512]):
            lo = 8 * wrap - 8 * 16 - 400 + 9 * v
            n = lo - pos
            while n > 24:
                ln = int(rng.integers(10, 13))
                body.append(LITS[ln - 1])
                n -= ln
            body += pad(n, rng)
            pos = lo
            while pos < 8 * wrap + 64:
                n = int(rng.integers(0, 14)) + v
                body += pad(n, rng) + [pair(int(rng.integers(0, 32)), int(rng.integers(0, 100)))]
                pos += n + SYM_BITS
        body += pad(4000, rng)
        blocks = head + [ds.dynamic(LL_48, D_48, body, final=True)]

        def pre(stream):
            assert host_walk(stream)["error"] is None and len(stream) > INF_IN[512]
            return f"{len(stream)} bytes of stream; alignments at which a pair's two dwords lie on either side of the wrap: " \
                   f"{ {nt: wrap_alignments(stream, nt) for nt in ds.LANES} }"
        return ds.zlib_stream(blocks, data=expand(blocks)), pre


@functools.lru_cache(maxsize=None)
def wrap_alignments(stream, nt):
    """the offsets modulo 16 of the stream in a batch at which a pair's general step asks for the last dword of the staged window
    and the first one (`next` + 1 is a multiple of the window's dwords), and merges both"""
    return [a for a in range(16) if any((s.next + 1) % (INF_IN[nt] // 4) == 0 and s.merges == 2 for s in pair_steps(stream, nt, a))]


for _v in range(WRAP_VARIANTS):
    _wrap_case(_v)


def _refusal_case(kind, off):
    @case(f"refused_{kind}_at_phase_{off}", 6, accept=False)
    def _():
        # a good pair, FILL_TAIL, the bad one at bit `off` modulo 32: valid bits on entry 32 - off for off = 0 .. 11 (see FILL_TAIL)
        rng = np.random.default_rng(160 + off)
        d = D_ONE if kind == "distance_code_without_symbol" else D_48
        head = lead_in()
        pos = _body_start(LL_48, d, head)
        pbits = 15 + 5 + d[DIST_SYM] + 13
        n = int(rng.integers(20, 50))
        n += (off - sum(FILL_TAIL) - pbits - pos - n) % 32
        good = pad(n, rng) + [pair(off & 31, off)] + pad(sum(FILL_TAIL), rng, FILL_TAIL)
        at = pos + n + pbits + sum(FILL_TAIL)
        if kind == "distance_code_without_symbol":  # the length, then the one-bit code that names nothing
            bad = [("ll", LEN_SYM), ("raw", off & 31, 5), ("raw", 1, 1)]
        else:                                         # 16 385 + 8 191 bytes back with 16 514 + a few there
            bad = [pair(off & 31, 8191)]
        blocks = head + [ds.dynamic(LL_48, d, good + bad + list(LITS), final=True)]
        data = expand(head + [ds.dynamic(LL_48, d, good, final=True)])

        def pre(stream):
            w = host_walk(stream)
            assert w["error"] == ("distance code" if kind == "distance_code_without_symbol" else "distance too far back"), w["error"]
            assert w["error_bit"] == at and at % 32 == off and len(w["out"]) == len(data) < DIST_BASE + 8191
            fills = set()
            for nt in ds.LANES:
                st = device_walk(stream, nt)[-1]
                assert st.kind == "bad" and st.bit == at
                fills.add(st.cnt)
            return f"stops at bit {at}: {w['error']}; valid bits on entry {sorted(fills)}"
        return ds.zlib_stream(blocks, data=data), pre


def refusal_fill(c, nt, align=0):
    """valid bits on entry to the general step that meets the bad symbol of a case of group 6"""
    return device_walk(c.stream, nt, align)[-1].cnt


for _off in range(32):
    _refusal_case("distance_too_far_back", _off)
    _refusal_case("distance_code_without_symbol", _off)


# ---- the .cct entrance: a real payload behind 48-bit pairs ---------------------------------------------------------------------
def run_payload_stream(pay):
    """(stream, check) for a payload that is a few bytes, one run of one byte longer than 32 KiB, and a few bytes (the payload of
    a flat image): the run's byte on the one-bit code, DIST_BASE and more of it by copies from one byte back, then 64 times
    seventeen literals and a 48-bit pair, which moves the pair through every bit offset modulo 64, then the rest of the run"""
    pay = bytes(pay)
    run = max(set(pay), key=pay.count)
    lo = pay.index(run)
    hi = lo
    while hi < len(pay) and pay[hi] == run:
        hi += 1
    others = sorted(set(pay) - {run})
    assert hi - lo > 32768 and len(others) <= 11
    fill = [b for b in range(256) if b != run and b not in others]
    lits = [run] + others + fill[:11 - len(others)]
    ll = _ladder(282, lits + [ds.EOB, fill[11], LEN_SYM, fill[12]])
    body, n = list(pay[:lo]), hi - lo
    body.append(run)
    n -= 1
    while hi - lo - n < DIST_BASE + 200:
        body.append(("ld", LEN_SYM, 31, 0, 0))
        n -= LEN_BASE + 31
    for k in range(64):
        lx = (5 * k) % 32
        body += [run] * 17 + [pair(lx, 3 * k)]
        n -= 17 + LEN_BASE + lx
    while n >= LEN_BASE:
        lx = min(31, n - LEN_BASE)
        body.append(("ld", LEN_SYM, lx, 0, 0))
        n -= LEN_BASE + lx
    body += [run] * n + list(pay[hi:])
    blocks = [ds.dynamic(ll, D_48, body, final=True)]
    assert expand(blocks) == pay

    def check(stream):
        w = host_walk(stream)
        syms = w["blocks"][0]["syms"]
        bits = {a.bit % 64 for a, b in zip(syms, syms[1:]) if a.kind == "len" and b.bit - a.bit == SYM_BITS}
        assert w["error"] is None and bits == set(range(64))
    return ds.zlib_stream(blocks, data=pay), check
