"""Hand-built TIFF LZW code streams for tiff_lzw_decode_kernel and planted strips for tiff_lzw_encode_kernel
(csrc/tiff_kernels.hip), with a census of what they reach.  Pillow's libtiff is the judge of every stream; tests/tiff_model.py
gives the expectation.  Test infrastructure only: pure Python + numpy, no device.

A greedy coder decides by its data which lane of a 64-code group holds a KwKwK, how deep a chain inside a group goes and
where a Clear falls.  The streams here are written code by code instead (Stream), so each of those is planted:

    border    a Clear, an EOI and the end of the data at lanes 0, 1, 62, 63 of the first group, a later group and the group
              behind a mid-group Clear; the same EOI / end one code after `want` is reached
    beyond    code 257 + j (refused) and 256 + j (KwKwK) at those lanes, a non-literal behind a Clear at those lanes, a bad code
              one lane before and one lane after the lane that reaches `want`
    ingroup   a KwKwK chain over a whole group (63 hops), two interleaved chains, a star, a chain that goes on in lane 0 of the
              next group, references to late copies
    cross     references to the previous group's last code (ref == jb - 1) from lanes 0, 1, 31, 63 with lane 0 a literal, a
              parallel and a late copy, and to its second-to-last code
    cut       `want` reached at a string's end, one byte before it, inside a parallel copy, a late copy and a KwKwK, at lane 63
              and at lane 0, by a string of more than 64 bytes
    width     codes 254/255, 766/767, 1790/1791 as references, KwKwKs and Clears at every bit phase
    table     3838 .. 3905 and 4862 / 4863 codes without a Clear, references to codes 4094 / 4095 and to low entries from
              beyond the kept entries, each with a twin whose code 4862 is a Clear
    random    120 legal non-greedy streams
    long      a string of 3000 bytes, copied from a later group and as a KwKwK, and `want` reached by it

Lanes are (j - 1) % 64 with j the code's number since the last Clear: the kernel restarts its groups at every Clear.  All
cases but `long` decode to one 24 x 257 strip of 8-bit samples (WANT = 6168 bytes).  A string of L bytes needs its L - 1
prefixes in the output first, L (L + 1) / 2 bytes: in 6168 bytes no string is longer than 110, so the strings of 1000 and
3000 bytes have a shape of their own (LONG_ROWS x LONG_COLS, 4.5 MB in one strip; the files stay at 5 KiB).

group_census replays a code list in groups of 64 as the kernel takes them and reports what it reached; probe_census replays
the encoder's dictionary.  tests/test_tiff_lzw_streams_host.py asserts every planted item by them and every verdict by Pillow;
tests/test_gpu_tiff_lzw_streams.py runs the cases on the device."""
import collections
import functools

import numpy as np

import tiff_model as m
from pass_borders import constant

CLEAR, EOI = m.CLEAR, m.EOI
GROUP = 64                                            # codes a step of the decoder takes: its wave
ROWS, COLS = 24, 257
WANT = ROWS * COLS
LONG_ROWS, LONG_COLS = 1502, 3001
LONG_WANT = LONG_ROWS * LONG_COLS
LONG_CHAIN = 3000
LANES = (0, 1, 62, 63)
SLOTS = constant("cct_internal.h", "TIFF_LZW_SLOTS")
TAB = constant("cct_internal.h", "TIFF_LZW_TAB")
MAX_J = constant("cct_internal.h", "TIFF_LZW_MAX_J")
WIDTH_BORDERS = (254, 766, 1790)
BORDER_NUMBERS = frozenset(B for b in WIDTH_BORDERS for B in (b, b + 1))
TOP_REF = 4095 - 257                                  # the last code a 12-bit code can name: entry 4095
FILL_CLEAR = 3800                                     # the filler clears before a run gets this long

Case = collections.namedtuple("Case", "name group codes data want accept planted")


# ---- a stream, code by code ---------------------------------------------------------------------------------------------

class Stream:
    """A code list and what it decodes to.  j codes have been written since the last Clear; the next one is code j + 1 at lane
    j % 64.  start / length: where the string of code r begins in the output and how long it is."""

    def __init__(self, want=WANT, seed=0, clears=1):
        self.want, self.codes, self.out = want, [], bytearray()
        self.rng = np.random.default_rng([seed, 20231])
        self._reset()
        for _ in range(clears):
            self.clear()

    def _reset(self):
        self.j, self.start, self.length, self.by_len = 0, [None], [None], {}

    @property
    def lane(self):
        return self.j % GROUP

    @property
    def done(self):
        return len(self.out) >= self.want

    @property
    def bits(self):
        return sum(w for _, w in self.codes)

    def _put(self, code):
        assert code < 1 << m.width(self.j + 1), (code, self.j + 1)
        self.codes.append((code, m.width(self.j + 1)))

    def _emit(self, s):
        self.j += 1
        self.start.append(len(self.out))
        self.length.append(len(s))
        if s:
            self.by_len[len(s)] = self.j
        self.out += s

    def clear(self):
        self._put(CLEAR)
        self._reset()

    def raw(self, code):
        """a code that decodes to nothing: an EOI, or one beyond the table"""
        self._put(code)
        self._emit(b"")

    def eoi(self):
        self.raw(EOI)

    def bad(self):
        self.raw(257 + self.j + 1)

    def lit(self, b=None):
        b = int(self.rng.integers(0, 256)) if b is None else b
        self._put(b)
        self._emit(bytes([b]))

    def ref(self, r):
        """table entry 257 + r: the string of code r and the first byte of code r + 1 (r == j: KwKwK)"""
        assert 1 <= r <= self.j and self.length[r], (r, self.j)
        a = self.start[r]
        s = bytes(self.out[a:a + self.length[r]])
        s += s[:1] if r == self.j else bytes(self.out[self.start[r + 1]:self.start[r + 1] + 1])
        assert len(s) == self.length[r] + 1
        self._put(257 + r)
        self._emit(s)

    def kw(self):
        self.ref(self.j)

    def lits_to(self, j):
        """literals until j codes stand behind the last Clear"""
        assert self.j <= j
        while self.j < j:
            self.lit()

    def mixed_to(self, j, maxlen=3, p_lit=0.6):
        """non-greedy codes until j codes stand: literals, references to any earlier string shorter than maxlen, KwKwKs"""
        assert self.j <= j
        while self.j < j:
            u = self.rng.random()
            r = int(self.rng.integers(1, self.j + 1)) if self.j else 0
            if not self.j or u < p_lit or self.length[r] >= maxlen or not self.length[r]:
                self.lit()
            elif u < 0.95 or self.length[self.j] >= maxlen or not self.length[self.j]:
                self.ref(r)
            else:
                self.kw()
        assert not self.done

    def ladder(self, n):
        """a literal and n - 1 KwKwKs: code r of the run is r bytes long (call right behind a Clear)"""
        assert self.j == 0
        self.lit()
        for _ in range(n - 1):
            self.kw()

    def _mark(self):
        return len(self.codes), self.j, len(self.out), dict(self.by_len)

    def _restore(self, mark):
        nc, j, no, by = mark
        del self.codes[nc:], self.start[j + 1:], self.length[j + 1:], self.out[no:]
        self.j, self.by_len = j, by

    def budget(self, ncodes, nbytes):
        """exactly ncodes codes for exactly nbytes bytes, the longest strings first; False and nothing written if they cannot"""
        mark = self._mark()
        for k in range(ncodes, 0, -1):
            room = nbytes - (k - 1)
            if room < 1:
                self._restore(mark)
                return False
            L = min(room, max(self.by_len, default=0) + 1)
            while L > 1 and L - 1 not in self.by_len:
                L -= 1
            if L == 1:
                self.lit()
            else:
                self.ref(self.by_len[L - 1])
            nbytes -= L
        if nbytes:
            self._restore(mark)
            return False
        return True

    def goto(self, lane, nbytes):
        """codes until the next one sits at `lane` with exactly nbytes bytes out"""
        need = nbytes - len(self.out)
        n = (lane - self.j) % GROUP
        while not ((n == 0 and need == 0) or (n and self.budget(n, need))):
            n += GROUP
            assert self.j + n < FILL_CLEAR, "goto: no room"
        assert self.lane == lane and len(self.out) == nbytes

    def spread(self, ncodes, nbytes):
        """exactly ncodes codes for exactly nbytes bytes with short strings only: literals and pairs, sprinkled"""
        slack = nbytes - ncodes
        assert 0 <= slack <= ncodes - 2, (ncodes, nbytes)
        for k in range(ncodes, 0, -1):
            r = int(self.rng.integers(1, min(self.j, TOP_REF) + 1)) if self.j else 0
            want_pair = slack and self.j >= 2 and (slack >= k - 1 or self.rng.random() < 0.3)
            if want_pair:
                while self.length[r] != 1:        # code 1 is a literal
                    r -= 1
                self.ref(r)
                slack -= 1
            else:
                self.lit()
        assert slack == 0

    def fill(self):
        """ordinary non-greedy codes until `want` bytes are out"""
        while not self.done:
            if self.j + 1 > FILL_CLEAR:
                self.clear()
            u = self.rng.random()
            if not self.j or u < 0.5:
                self.lit()
            elif u < 0.9 or not self.length[self.j]:
                r = int(self.rng.integers(1, self.j + 1))
                self.ref(r) if self.length[r] else self.lit()
            else:
                self.kw()
        return self


def pack(codes):
    return m.pack_codes(codes)


def _case(name, group, s, accept, planted, data=None):
    return Case(name, group, tuple(s.codes), pack(s.codes) if data is None else data, s.want, accept, planted)


def _ending(name, group, build, missing, accept, planted, want=WANT, seed=0):
    """build(s) writes the codes; the data ends `missing` bits short of one more code's end (0: right behind the last code).
    Opening Clears move the bit phase until the cut falls on a byte."""
    for clears in range(1, 9):
        s = Stream(want, seed, clears)
        build(s)
        if missing:
            s.lit()
        if s.bits % 8 == missing:
            break
    else:
        raise AssertionError(name)
    data = pack(s.codes)
    return _case(name, group, s, accept, planted, data[:-1] if missing else data)


# ---- the decoder's cases ------------------------------------------------------------------------------------------------

def _to(s, where, lane):
    """the next code sits at `lane` of the first group, a later group, or the group behind a mid-group Clear"""
    if where == "first":
        s.mixed_to(lane)
    elif where == "later":
        s.mixed_to(2 * GROUP + lane)
    else:
        s.mixed_to(20)
        s.clear()
        s.mixed_to(lane)


WHERES = ("first", "later", "after_clear")


def _border_cases(want=WANT):
    out, k = [], 0
    for where in WHERES:
        for lane in LANES:
            tag = f"{where}_lane{lane}"
            s = Stream(want, k)
            _to(s, where, lane)
            s.clear()
            out.append(_case(f"border_clear_{tag}", "border", s.fill(), True, {"stop_clear": {(lane, where)}}))
            s = Stream(want, k)
            _to(s, where, lane)
            s.eoi()
            out.append(_case(f"border_eoi_{tag}", "border", s, False, {"stop_eoi": {(lane, where)}}))
            missing = 1 + k % 7
            for miss in (0, missing):
                out.append(_ending(f"border_end_{tag}_missing{miss}", "border", lambda s, where=where, lane=lane: _to(s, where, lane), miss, False,
                                   {"stop_end": {(lane, where, miss)}}, want, k))
            k += 1
    for lane in LANES:   # one code behind the code that reaches `want`: ignored
        def reach(s, lane=lane):
            s.ladder(12)
            s.goto((lane - 1) % GROUP, s.want - 1)
            s.lit()
        s = Stream(want, 100 + lane)
        reach(s)
        s.eoi()
        out.append(_case(f"border_eoi_after_want_lane{lane}", "border", s, True, {"ignored": {("eoi", lane)}}))
        for miss in (0, 1 + lane % 7):
            out.append(_ending(f"border_end_after_want_lane{lane}_missing{miss}", "border", reach, miss, True, {"ignored": {("end", lane)}}, want, 100 + lane))
    return out


def _beyond_cases(want=WANT):
    out = []
    for where, lanes in (("first", (1, 62, 63)), ("later", LANES)):   # lane 0 of the first group is code 1: see non-literal below
        for lane in lanes:
            s = Stream(want, 200 + lane)
            _to(s, where, lane)
            s.bad()
            out.append(_case(f"beyond_bad_{where}_lane{lane}", "beyond", s, False, {"stop_bad": {lane}}))
            s = Stream(want, 200 + lane)
            _to(s, where, lane)
            s.kw()
            out.append(_case(f"beyond_kwkwk_{where}_lane{lane}", "beyond", s.fill(), True, {"kw_lanes": {lane}}))
    for lane in LANES:
        for code in (258, 300):
            s = Stream(want, 210 + lane)
            _to(s, "later", lane)
            s.clear()
            s.raw(code)
            out.append(_case(f"beyond_non_literal_{code}_behind_clear_at_lane{lane}", "beyond", s, False, {"bad_behind_clear": {lane}}))
    s = Stream(want, 220)
    s.ladder(12)
    s.goto(29, s.want - 5)
    s.bad()
    s.ref(9)
    out.append(_case("beyond_bad_one_lane_before_the_cut", "beyond", s, False, {"stop_bad": {29}, "bad_next_to_cut": {"before"}}))
    s = Stream(want, 220)
    s.ladder(12)
    s.goto(30, s.want - 5)
    s.ref(9)
    s.bad()
    out.append(_case("beyond_bad_one_lane_after_the_cut", "beyond", s, True, {"ignored": {("bad", 31)}, "bad_next_to_cut": {"after"}}))
    return out


def _ingroup_cases(want=WANT):
    out = []

    def chain(s):
        s.mixed_to(2 * GROUP)
        s.lit()
        for _ in range(GROUP - 1):
            s.kw()

    s = Stream(want, 300)
    chain(s)
    out.append(_case("ingroup_kwkwk_chain_over_a_group", "ingroup", s.fill(), True, {"chain": GROUP - 1}))
    s = Stream(want, 301)
    chain(s)
    for _ in range(9):      # lane 0 of the next group goes on: KwKwK across the border, then eight more
        s.kw()
    out.append(_case("ingroup_chain_goes_on_in_the_next_group", "ingroup", s.fill(), True, {"chain": GROUP - 1, "border_refs": {(0, "kw")}}))
    s = Stream(want, 302)
    s.mixed_to(2 * GROUP)
    s.lit(); s.lit()
    for _ in range(GROUP - 2):
        s.ref(s.j - 1)      # lane k names lane k - 2
    out.append(_case("ingroup_two_interleaved_chains", "ingroup", s.fill(), True, {"chain": GROUP // 2 - 1, "late_of_late": 30}))
    s = Stream(want, 303)
    s.mixed_to(2 * GROUP)
    s.lit()
    for _ in range(GROUP - 1):
        s.ref(2 * GROUP + 1)
    out.append(_case("ingroup_star", "ingroup", s.fill(), True, {"fan_in": GROUP - 1}))
    s = Stream(want, 304)
    s.mixed_to(2 * GROUP)
    s.lit(); s.kw()                      # lane 1: a late copy
    s.lits_to(2 * GROUP + 5)
    s.ref(2 * GROUP + 2)                 # lane 5 names lane 1
    s.lits_to(2 * GROUP + 9)
    s.ref(2 * GROUP + 6)                 # lane 9 names lane 5
    s.ref(2 * GROUP + 10)                # and lane 10 lane 9: a KwKwK of a late copy
    out.append(_case("ingroup_references_to_late_copies", "ingroup", s.fill(), True, {"late_of_late": 3}))
    return out


def _cross_cases(want=WANT):
    out = []
    jb = 2 * GROUP + 1

    def front(s, last_literal=False):
        """two groups; the second one's last code is a three-byte string, or a literal"""
        s.lit(); s.kw(); s.kw()
        s.mixed_to(jb - 2)
        if last_literal:
            s.lit()
        else:
            s.ref(2)
        assert s.j == jb - 1

    s = Stream(want, 400)
    front(s)
    s.kw()
    out.append(_case("cross_kwkwk_from_lane0", "cross", s.fill(), True, {"border_refs": {(0, "kw")}}))
    for lane in (1, 31, 63):
        for kind0 in ("lit", "par", "kw"):
            s = Stream(want, 400 + lane)
            front(s)
            {"lit": s.lit, "par": lambda: s.ref(3), "kw": s.kw}[kind0]()
            s.lits_to(jb - 1 + lane)
            s.ref(jb - 1)
            out.append(_case(f"cross_last_code_from_lane{lane}_lane0_{kind0}", "cross", s.fill(), True, {"border_refs": {(lane, kind0)}}))
    for lane in (0, 1, 63):   # the second-to-last code, the last one a literal: the source ends where the group's output starts
        s = Stream(want, 410 + lane)
        front(s, last_literal=True)
        s.lits_to(jb - 1 + lane)
        s.ref(jb - 2)
        out.append(_case(f"cross_second_to_last_code_from_lane{lane}", "cross", s.fill(), True, {"border2_refs": {(lane, True)}}))
    return out


def _cut_cases(want=WANT):
    out = []

    def case(name, lane, short, plant, planted):
        s = Stream(want, 500 + len(out))
        s.ladder(80)                       # code r: r bytes
        s.goto(lane, s.want - short)
        plant(s)
        assert s.done
        out.append(_case("cut_" + name, "cut", s, True, planted))

    case("at_a_strings_end", 10, 6, lambda s: s.ref(5), {"cut": {("par", "exact")}})
    case("one_byte_before_a_strings_end", 10, 5, lambda s: s.ref(5), {"cut": {("par", "inside")}})
    case("inside_a_parallel_copy", 10, 3, lambda s: s.ref(9), {"cut": {("par", "inside")}})

    def late(s):
        s.ref(9); s.lit(); s.ref(s.j - 1)  # lane 12 names lane 10: 11 bytes, a late copy
    case("inside_a_late_copy", 10, 20, late, {"cut": {("late", "inside")}, "cut_lane": {12}})

    def kw(s):
        s.ref(9); s.kw()
    case("inside_a_kwkwk", 10, 15, kw, {"cut": {("kw", "inside")}, "cut_lane": {11}})
    case("at_lane63_by_a_literal", 63, 1, lambda s: s.lit(), {"cut": {("lit", "exact")}, "cut_lane": {63}})
    case("at_lane63_inside_a_string", 63, 3, lambda s: s.ref(9), {"cut": {("par", "inside")}, "cut_lane": {63}})
    case("at_lane0_by_a_literal", 0, 1, lambda s: s.lit(), {"cut": {("lit", "exact")}, "cut_lane": {0}})

    def kw0(s):
        s.ref(4); s.kw()                   # five bytes at lane 63, six at lane 0, three of them wanted
    case("at_lane0_inside_a_kwkwk", 63, 8, kw0, {"cut_lane": {0}, "kw_lanes": {0}})   # cut short of the group's output: no late copy
    case("by_a_string_of_71_bytes", 10, 30, lambda s: s.ref(70), {"cut": {("par", "inside")}, "cut_len": 71})
    return out


def _width_cases(want=WANT):
    out = []
    for B in WIDTH_BORDERS:
        for kind in ("ref", "kw", "clear_at", "clear_behind"):
            for phase in range(8):
                s = Stream(want, 600 + B, clears=phase + 1)
                s.mixed_to(B - 1, p_lit=0.75)
                if kind == "ref":
                    s.ref(int(s.rng.integers(1, s.j)))
                    s.ref(int(s.rng.integers(1, s.j)))
                    planted = {(B, "ref"), (B + 1, "ref")}
                elif kind == "kw":
                    s.kw(); s.kw()
                    planted = {(B, "kw"), (B + 1, "kw")}
                elif kind == "clear_at":
                    s.clear()
                    planted = {(B, "clear")}
                else:
                    s.lit(); s.clear()       # code 255 / 767 / 1791: a Clear in the wider width
                    planted = {(B + 1, "clear")}
                s.fill()
                pos = np.cumsum([0] + [w for _, w in s.codes])
                at = {j: int(pos[phase + j]) % 8 for j in (B, B + 1)}   # phase + 1 opening Clears, then code j
                out.append(_case(f"width_{B}_{kind}_phase{phase}", "width", s, True, {"border_codes": {(j, k, at[j]) for j, k in planted}}))
    return out


def _run_front(s, n):
    """n codes without a Clear for n + 500 bytes at most, the last ones naming the newest entries"""
    s.spread(n - 3, n - 3 + min(500, n // 8))
    s.ref(min(s.j - 1, TOP_REF - 1))
    s.ref(min(s.j, TOP_REF))                            # a KwKwK while 12 bits can still name the last code
    s.ref(1)


def _beyond_tab(s):
    """from code TAB + 1 on: references to entries 4094 and 4095, the last two a 12-bit code can name, and to low ones"""
    assert s.j >= TAB
    for r in (TOP_REF - 1, TOP_REF, 1, 2, TOP_REF, TOP_REF - 1):
        s.ref(r) if s.length[r] else s.lit()


def _table_cases(want=WANT):
    out = []
    for n in (3838, 3839, TAB - 1, TAB, TAB + 1):
        s = Stream(want, 700 + n)
        _run_front(s, n)
        s.clear()
        out.append(_case(f"table_{n}_codes_then_clear", "table", s.fill(), True, {"runs": {n}}))
        s = Stream(want, 700 + n)            # the twin: on to 4861 codes, code 4862 a Clear
        _run_front(s, n)
        s.lits_to(max(s.j, TAB))
        _beyond_tab(s)
        s.spread(MAX_J - 1 - s.j, MAX_J - 1 - s.j + 40)
        s.clear()
        out.append(_case(f"table_{n}_codes_twin_clear_is_code_{MAX_J}", "table", s.fill(), True,
                         {"runs": {MAX_J - 1}, "refs_beyond_tab": {4094, 4095, 258, 259}}))

    def long_run(s, n):
        """n - 1 codes for want - 1 bytes"""
        _run_front(s, TAB)
        _beyond_tab(s)
        s.spread(n - 1 - s.j, s.want - 1 - len(s.out))

    s = Stream(want, 750)
    long_run(s, MAX_J)
    s.lit()
    assert s.done and s.j == MAX_J
    out.append(_case(f"table_{MAX_J}_codes_want_met_by_the_last", "table", s, True, {"runs": {MAX_J}, "refs_beyond_tab": {4094, 4095, 258, 259}}))
    s = Stream(want, 751)
    long_run(s, MAX_J + 1)
    s.lit()
    assert s.done and s.j == MAX_J + 1
    out.append(_case(f"table_{MAX_J + 1}_codes", "table", s, False, {"runs": {MAX_J + 1}}))
    s = Stream(want, 754)                    # libtiff looks at the full table only once a data code comes: a Clear may be code 4863
    _run_front(s, TAB)
    _beyond_tab(s)
    s.spread(MAX_J - s.j, MAX_J - s.j + 40)
    s.clear()
    out.append(_case(f"table_{MAX_J}_codes_then_clear_is_code_{MAX_J + 1}", "table", s.fill(), True, {"runs": {MAX_J}, "clear_numbers": {MAX_J + 1}}))
    for n, seed in ((MAX_J, 752), (MAX_J + 1, 753)):
        s = Stream(want, seed)
        _run_front(s, TAB)
        _beyond_tab(s)
        s.spread(MAX_J - 1 - s.j, MAX_J - 1 - s.j + 40)
        s.clear()
        out.append(_case(f"table_{n}_codes_twin_clear_is_code_{MAX_J}", "table", s.fill(), True, {"runs": {MAX_J - 1}, "clear_numbers": {MAX_J}}))
    return out


RANDOM_MIXES = (   # literal, any earlier code, within 3 codes, within 64 codes, KwKwK, Clear
    (0.50, 0.30, 0.05, 0.05, 0.09, 0.01),
    (0.20, 0.10, 0.30, 0.30, 0.10, 0.00),
    (0.70, 0.05, 0.05, 0.05, 0.05, 0.10),
    (0.10, 0.40, 0.10, 0.10, 0.29, 0.01),
    (0.30, 0.00, 0.00, 0.60, 0.10, 0.00),
    (0.30, 0.00, 0.50, 0.00, 0.19, 0.01),
)


def _random_cases(want=WANT, per_mix=20):
    out = []
    for k, mix in enumerate(RANDOM_MIXES):
        edges = np.cumsum(mix)
        for seed in range(per_mix):
            s = Stream(want, 800 + 100 * k + seed)
            while not s.done:
                if s.j + 1 > FILL_CLEAR:
                    s.clear()
                kind = min(5, int(np.searchsorted(edges, s.rng.random() * edges[-1], side="right"))) if s.j else 0
                if kind == 0:
                    s.lit()
                elif kind == 4:
                    s.kw() if s.length[s.j] else s.lit()
                elif kind == 5:
                    s.clear()
                else:
                    near = {1: s.j, 2: 3, 3: GROUP}[kind]
                    r = int(s.rng.integers(max(1, s.j + 1 - near), s.j + 1))
                    s.ref(r) if s.length[r] else s.lit()
            out.append(_case(f"random_mix{k}_seed{seed}", "random", s, True, {}))
    return out


def _long_cases():
    out = []

    def front(s, pad):
        s.ladder(LONG_CHAIN)                      # code r: r bytes, 4 501 500 in all
        s.lits_to(LONG_CHAIN + pad)               # into a later group
        s.ref(LONG_CHAIN)                         # 3001 bytes from far back: a parallel copy

    s = Stream(LONG_WANT, 900)
    front(s, 40)
    s.kw()                                        # 3002 bytes
    assert s.done
    out.append(_case("long_string_copied_and_cut_inside_its_kwkwk", "long", s, True,
                     {"cut": {("kw", "inside")}, "cut_len": LONG_CHAIN + 2, "longest_parallel": LONG_CHAIN + 1, "longest_late": LONG_CHAIN}))
    s = Stream(LONG_WANT, 901)
    front(s, 70)
    s.ref(LONG_CHAIN - 1)                         # 3000 bytes, cut
    assert s.done
    out.append(_case("long_string_cut_inside_a_parallel_copy", "long", s, True, {"cut": {("par", "inside")}, "cut_len": LONG_CHAIN, "longest_parallel": LONG_CHAIN + 1}))
    s = Stream(LONG_WANT, 902)
    front(s, 10)
    s.bad()
    out.append(_case("long_string_then_a_code_beyond_the_table", "long", s, False, {"longest_parallel": LONG_CHAIN + 1}))
    s = Stream(LONG_WANT, 903)
    front(s, 12)
    s.lit(); s.lit()
    s.fill()
    out.append(_case("long_string_then_filler", "long", s, True, {"longest_parallel": LONG_CHAIN + 1}))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """every decoder case of the common shape, in a fixed order"""
    out = _border_cases() + _beyond_cases() + _ingroup_cases() + _cross_cases() + _cut_cases() + _width_cases() + _table_cases() + _random_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def long_cases():
    return tuple(_long_cases())


def file_of(case):
    """the case as a one-strip 8-bit file, predictor 1"""
    rows, cols = (ROWS, COLS) if case.want == WANT else (LONG_ROWS, LONG_COLS)
    assert rows * cols == case.want
    return m.build_file(np.zeros((rows, cols), np.uint8), 5, 1, rows, code=lambda s, i: case.data)


def expected(case):
    """the model's verdict: the raster, or "CCT_E_STREAM" """
    verdict, raw = m.lzw_decode(case.data, case.want)
    if verdict != "OK":
        return verdict
    rows, cols = (ROWS, COLS) if case.want == WANT else (LONG_ROWS, LONG_COLS)
    return np.frombuffer(raw, np.uint8).reshape(rows, cols)


EMBEDDED = ("cross_last_code_from_lane31_lane0_lit", "ingroup_kwkwk_chain_over_a_group", "beyond_bad_later_lane63", "border_eoi_after_want_lane1")


@functools.lru_cache(maxsize=None)
def embedded_files():
    """[(name, file, the model's raster or "CCT_E_STREAM")]: cases rebuilt for the 560 bytes of a middle strip of
    tiff_model._fixture_raster() in strips of 7 rows, 16 bits, predictor 2, between ordinary strips, in both byte orders"""
    a = m._fixture_raster()
    want = 7 * a.shape[1] * 2
    small = {c.name: c for c in _border_cases(want) + _beyond_cases(want) + _ingroup_cases(want) + _cross_cases(want)}
    out = []
    for name in EMBEDDED:
        c = small[name]
        for order in ("II", "MM"):
            f = m.build_file(a, 5, 2, 7, order, code=lambda s, i: c.data if i == 1 else m.lzw_encode(s))
            out.append((f"{name}_{order}", f, m.read(f, a.shape[0], a.shape[1], 16)))
    return tuple(out)


# ---- census of the decoder's cases ---------------------------------------------------------------------------------------

def group_census(codes, want=WANT, nbits=None):
    """Replay a code list in groups of 64 codes as tiff_lzw_decode_kernel takes them -- a group ends at its first Clear, EOI or
    missing code (F) or its first code beyond the table (X), the next one starts at code 1 behind a Clear or 64 codes on --
    and report what was reached.  nbits: the bits the data holds (default: the codes, padded to a byte)."""
    pos = [0]
    for _, w in codes:
        pos.append(pos[-1] + w)
    if nbits is None:
        nbits = -(-pos[-1] // 8) * 8
    c = dict(verdict=None, stop_clear=set(), stop_eoi=set(), stop_end=set(), stop_bad=set(), ignored=set(), kw_lanes=set(), bad_behind_clear=set(),
             bad_next_to_cut=set(), chain=0, fan_in=0, late_of_late=0, border_refs=set(), border2_refs=set(), cut=set(), cut_lane=set(), cut_len=0,
             longest_parallel=0, longest_late=0, runs=set(), clear_numbers=set(), refs_beyond_tab=set(), border_codes=set(), groups=0)
    i, jb, outpos = 0, 1, 0
    len_of, dst_of = {}, {}
    data_seen, where, clear_lane = False, "first", None

    def kind_of_stop(k):
        if k >= len(codes) or pos[k + 1] > nbits:
            return "end"
        return {CLEAR: "clear", EOI: "eoi"}.get(codes[k][0])

    def is_bad(k, j):
        code = codes[k][0]
        return (code >= 258 and code > 256 + j) or j > MAX_J

    while True:
        c["groups"] += 1
        G = outpos
        F = X = GROUP
        for lane in range(GROUP):
            k, j = i + lane, jb + lane
            if k < len(codes):
                assert codes[k][1] == m.width(j), (k, j, codes[k])
            if kind_of_stop(k):
                F = lane
                break
            if is_bad(k, j):
                X = lane
                break
        nv = min(F, X)
        lens, dsts, kinds, depth, names = [], [], [], [], collections.Counter()
        reached = None
        for lane in range(nv):
            k, j = i + lane, jb + lane
            code = codes[k][0]
            ref = code - 257 if code >= 258 else 0
            if j in BORDER_NUMBERS and ref:
                c["border_codes"].add((j, "kw" if ref == j - 1 else "ref", pos[k] % 8))
            if ref and j > TAB:
                c["refs_beyond_tab"].add(code)
            if not ref:
                ln, src, d = 1, None, 0
            elif ref >= jb:
                t = ref - jb
                ln, src, d = lens[t] + 1, dsts[t], depth[t] + 1
                names[t] += 1
                c["late_of_late"] += kinds[t] in ("late", "kw")
            else:
                ln, src, d = len_of[ref] + 1, dst_of[ref], 0
            dst = min(outpos, want)
            n = min(ln, want - dst)
            late = bool(ref and n and src + n > G)
            kind = "lit" if not ref else ("kw" if ref == j - 1 else "late") if late else "par"
            if ref == j - 1:
                c["kw_lanes"].add(lane)
            if ref and jb > 1 and ref == jb - 1:
                c["border_refs"].add((lane, kinds[0] if lane else kind))
            if ref and jb > 2 and ref == jb - 2:
                assert not late
                c["border2_refs"].add((lane, src + n == G))
            if kind == "par":
                c["longest_parallel"] = max(c["longest_parallel"], n)
            elif ref:
                c["longest_late"] = max(c["longest_late"], n)
            c["chain"] = max(c["chain"], d)
            lens.append(ln); dsts.append(dst); kinds.append(kind); depth.append(d)
            if j < TAB:
                len_of[j], dst_of[j] = ln, dst
            outpos += ln
            if reached is None and outpos >= want:
                reached = lane
                c["cut"].add((kind, "exact" if outpos == want else "inside"))
                c["cut_lane"].add(lane)
                c["cut_len"] = max(c["cut_len"], ln)
        if names:
            c["fan_in"] = max(c["fan_in"], max(names.values()))
        data_seen = data_seen or nv > 0
        if reached is not None:
            c["verdict"] = "OK"
            c["runs"].add(jb + reached)
            k, j = i + reached + 1, jb + reached + 1
            what = kind_of_stop(k) or ("bad" if is_bad(k, j) else None)
            if what:
                c["ignored"].add((what, (reached + 1) % GROUP))
                if what == "bad":
                    c["bad_next_to_cut"].add("after")
            return c
        if X < F:
            c["verdict"] = "CCT_E_STREAM"
            c["stop_bad"].add(X)
            j = jb + X
            if j > MAX_J:
                c["runs"].add(j)
            if j == 1 and clear_lane is not None:
                c["bad_behind_clear"].add(clear_lane)
            k = i + X + 1
            if X + 1 < GROUP and k < len(codes) and not kind_of_stop(k) and codes[k][0] >= 258 and codes[k][0] - 257 < jb:
                if outpos + len_of[codes[k][0] - 257] + 1 >= want:
                    c["bad_next_to_cut"].add("before")
            return c
        if F == GROUP:
            i, jb = i + GROUP, jb + GROUP
            where = "later"
            continue
        k = i + F
        what = kind_of_stop(k)
        if what == "clear":
            if i:   # not the opening one
                c["stop_clear"].add((F, where))
                if jb + F > 1:
                    c["runs"].add(jb + F - 1)
                    c["clear_numbers"].add(jb + F)
                if jb + F in BORDER_NUMBERS:
                    c["border_codes"].add((jb + F, "clear", pos[k] % 8))
            clear_lane = F if i else None
            where = "after_clear" if data_seen and F else ("first" if not data_seen else "later_clear")
            i, jb = k + 1, 1
            len_of, dst_of = {}, {}
            continue
        c["verdict"] = "CCT_E_STREAM"
        if what == "eoi":
            c["stop_eoi"].add((F, where))
        else:
            have = max(0, nbits - pos[k]) if k < len(pos) else 0
            w = m.width(jb + F)
            c["stop_end"].add((F, where, 0 if have == 0 else w - have))
        return c


def merge(censuses):
    """the union of censuses: sets are joined, numbers take their maximum"""
    out = {}
    for c in censuses:
        for key, v in c.items():
            if isinstance(v, set):
                out.setdefault(key, set()).update(v)
            elif isinstance(v, int):
                out[key] = max(out.get(key, 0), v)
    return out


def holds(census, planted):
    """what a case planted is in its census: a set is contained, a number reached"""
    return all(v <= census[k] for k, v in planted.items())


# ---- the encoder's strips ---------------------------------------------------------------------------------------------------

def lzw_hash(key):
    """tiff_lzw_encode_kernel: `uint32_t h = (key * 2654435761u) >> 19;  // 13 bits`"""
    return (key * 2654435761 & 0xFFFFFFFF) >> 19


PROBE_WINDOWS = {"middle": SLOTS // 2, "end": SLOTS - 70}


def probe_strip(H, span=40, again=100):
    """every literal pair whose hash falls in [H, H + span), one after another, then the first `again` pairs once more: their
    entries crowd a few dozen slots, so inserts and finds run several probe windows on"""
    pairs = [(a, b) for a in range(256) for b in range(256) if (lzw_hash(a << 8 | b) - H) % SLOTS < span]
    return bytes(x for p in pairs + pairs[:again] for x in p)


@functools.lru_cache(maxsize=None)
def probe_strips():
    return tuple((name, probe_strip(H)) for name, H in PROBE_WINDOWS.items())


def probe_census(strip):
    """Replay tiff_lzw_encode_kernel's dictionary over a strip: linear probing from the hash, 64 slots a round.  Reports the
    most rounds a probe took, the inserts and finds that ended after the first round, the rounds whose 64 slots wrap the
    table's end (all, and after the first round), and the codes written (tiff_model.lzw_codes must give the same)."""
    c = dict(max_rounds=0, late_inserts=0, late_finds=0, wrapped=0, wrapped_late=0, codes=[(CLEAR, 9)])
    tab = [0] * SLOTS
    w, nxt = 9, 258
    incount, outcount, checkpoint, ratio = 1, 9, m.CHECK_GAP, 0
    omega = strip[0]

    def put(code):
        nonlocal outcount
        c["codes"].append((code, w))
        outcount += w

    for b in strip[1:]:
        incount += 1
        key = omega << 8 | b
        h, off = lzw_hash(key), 0
        while True:
            e = tab[(h + off) & (SLOTS - 1)]
            if e == 0 or e >> 12 == key:
                break
            off += 1
        rounds = off // GROUP + 1
        c["max_rounds"] = max(c["max_rounds"], rounds)
        for r in range(rounds):
            if (h + GROUP * r) & (SLOTS - 1) > SLOTS - GROUP:
                c["wrapped"] += 1
                c["wrapped_late"] += r > 0
        if e:
            omega = e & 0xFFF
            c["late_finds"] += rounds > 1
            continue
        tab[(h + off) & (SLOTS - 1)] = key << 12 | nxt
        c["late_inserts"] += rounds > 1
        put(omega)
        nxt += 1
        clear = nxt == 4094
        if not clear:
            if nxt == 1 << w:
                w += 1
            elif incount >= checkpoint:
                checkpoint = incount + m.CHECK_GAP
                rat = (incount << 8) // outcount      # incount stays below 0x7FFFFF: see DESIGN.md
                if rat <= ratio:
                    clear = True
                else:
                    ratio = rat
        if clear:
            incount, outcount, ratio = 0, 0, 0
            put(CLEAR)
            tab = [0] * SLOTS
            nxt, w = 258, 9
        omega = b
    put(omega)
    nxt += 1
    if nxt == 4094:
        put(CLEAR)
        w = 9
    elif nxt == 1 << w:
        w += 1
    put(EOI)
    return c
