"""Hand-built and damaged token streams for the decode kernel, and the judge of what the decoder owes them.

Plain Python / numpy: no device and no encoder.  The writer lays blocks out as a plan says and writes a random walk as
tokens; the image is what those tokens mean.  The judge is the decoder's contract for streams no encoder writes
 as sequential Python.  The damage generators cut, edit and flip a well-formed file, some of the
edits aimed at the byte offsets the kernel's parse is built around (16-byte segments, steps of threads * 16 bytes).

Token bytes (core.py:484-520): 0xxxxxxx short delta (7 bits, -63 .. 64), 10jjjjjj mesh jump (pair the next free block with
the one j blocks on), 1110xxxx xxxxxxxx full delta (12 bits, -2047 .. 2048), 110xxxxx / 1111xxxx reserved (one byte, the
previous pixel repeats).  The last byte of a payload (EOF, 59) is never read (ByteReader.padding_len).
"""
import numpy as np

from oracle import oracle

SHORT, FULL, RESERVED = 0, 1, 2
RESERVED_BYTES = (0xC0, 0xC5, 0xDF, 0xF0, 0xF3, 0xFF)
DEFECTS = ("jump_inside_block", "two_jumps", "bad_partner", "truncated")
PLANS = ("none", "near", "far", "rand", "p50", "half", "last", "jump63")
SEG = 16  # payload bytes one lane parses per step (DEC_SEG)


# ---------------------------------------------------------------------------------------------------- writer

def layout(NB, plan, rng):
    """Slots of the stream in order: [(leader block, j)], j = 0 for a block emitted alone.
    Plans: none; near / far / rand = every block paired with the nearest / farthest / a random free partner among
    i+1 .. i+63 (far fills the 64-block window completely); p50 = a pair with probability 1/2; half = NB/2 pairs
    (block 2k with 2k+1); last = one pair whose partner is the last block; jump63 = block 0 paired with block 63."""
    claimed = np.zeros(NB, bool)
    slots = []
    for i in range(NB):
        if claimed[i]:
            continue
        claimed[i] = True
        j = 0
        free = None
        if plan in ("near", "far", "rand", "half") or (plan == "p50" and rng.random() < 0.5):
            free = np.flatnonzero(~claimed[i + 1: min(i + 64, NB)]) + 1
        elif plan == "last" and i == max(NB - 40, 0) and NB > 1:
            free = np.array([NB - 1 - i])
        elif plan == "jump63" and i == 0 and NB > 63:
            free = np.array([63])
        if free is not None and len(free):
            j = int(free[-1] if plan == "far" else free[int(rng.integers(0, len(free)))] if plan in ("rand", "p50") else free[0])
            claimed[i + j] = True
        slots.append((i, j))
    return slots


def stream_positions(slots, bs):
    """traversal position of every pixel in stream order (a pair interleaves leader / partner)"""
    lead = np.array([s[0] for s in slots], np.int64)
    jj = np.array([s[1] for s in slots], np.int64)
    npx = np.where(jj > 0, 2 * bs, bs)
    start = np.concatenate(([0], np.cumsum(npx)[:-1]))
    trav = np.empty(int(npx.sum()), np.int64)
    ar = np.arange(bs)
    single = jj == 0
    trav[(start[single, None] + ar).ravel()] = (lead[single, None] * bs + ar).ravel()
    pair = ~single
    trav[(start[pair, None] + 2 * ar).ravel()] = (lead[pair, None] * bs + ar).ravel()
    trav[(start[pair, None] + 2 * ar + 1).ravel()] = ((lead[pair] + jj[pair])[:, None] * bs + ar).ravel()
    return trav, start


def walk(N, rng, full_p=0.2, reserved_p=0.05, bias=0.0):
    """A random walk inside [0, 65535] as (deltas, kinds), one entry per pixel.  bias > 0 shrinks the negative side of every
    draw (the walk climbs to 65535 and stays near it), bias < 0 the positive side.  Within reach of an edge a quarter
    of the draws land on it exactly."""
    r = rng.random(N)
    u = rng.random(N)
    e = rng.random(N)
    deltas = [0] * N
    kinds = [SHORT] * N
    val = 0
    for k in range(N):
        if r[k] < reserved_p:
            kinds[k] = RESERVED
            continue
        full = r[k] < reserved_p + full_p
        lo, hi = (-2047, 2048) if full else (-63, 64)
        if bias > 0:
            lo = int(lo * (1 - bias))
        elif bias < 0:
            hi = int(hi * (1 + bias))
        lo2, hi2 = max(lo, -val), min(hi, 65535 - val)
        d = lo2 + int(u[k] * (hi2 - lo2 + 1))
        if hi2 < hi and e[k] < 0.25:
            d = hi2
        elif lo2 > lo and e[k] < 0.25:
            d = lo2
        deltas[k] = d
        kinds[k] = FULL if full else SHORT
        val += d
    return deltas, kinds


def tokens(slots, bs, deltas, kinds):
    """payload bytes (EOF byte included) of the slots with the given per-pixel deltas and token kinds"""
    out = bytearray()
    k = 0
    for lead, j in slots:
        if j:
            out.append(0x80 | j)
        for _ in range(2 * bs if j else bs):
            kd = kinds[k]
            if kd == RESERVED:
                out.append(RESERVED_BYTES[k % len(RESERVED_BYTES)])
            elif kd == FULL:
                u = deltas[k] & 0xFFF
                out.append(0xE0 | (u >> 8))
                out.append(u & 0xFF)
            else:
                out.append(deltas[k] & 0x7F)
            k += 1
    out.append(59)
    return bytes(out)


def header(W, H, bs, fractal):
    """the 13-byte header of an oracle encode of the same shape and flags (no DEFLATE)"""
    return oracle.encode(np.zeros((W, H), np.uint16), block_size=bs, fractal=fractal, deflate=False)[:13]


def image_of(W, H, bs, fractal, slots, deltas, kinds):
    """what the tokens mean: the running value at the raster position of every stream pixel"""
    N = W * H
    O = oracle.curve(W, H).astype(np.int64) if fractal else np.arange(N, dtype=np.int64)
    trav, _ = stream_positions(slots, bs)
    d = np.array(deltas, np.int64)
    d[np.array(kinds) == RESERVED] = 0
    vals = np.cumsum(d)
    assert vals.min() >= 0 and vals.max() <= 65535
    img = np.zeros(N, np.uint16)
    img[O[trav]] = vals.astype(np.uint16)
    return img.reshape(W, H)


def build(W, H, bs, fractal, plan, rng, full_p=0.2, reserved_p=0.05, bias=0.0, jump_at=(), return_info=False):
    """-> (file bytes, image (W, H) uint16) [, info].  jump_at: payload offsets at which a jump byte shall stand (reached by
    choosing how many full tokens the slots before it hold; the offsets must be far enough apart, see _steer)."""
    N = W * H
    NB = N // bs
    deltas, kinds = walk(N, rng, full_p, reserved_p, bias)
    slots = layout(NB, plan, rng)
    if jump_at:
        slots, deltas, kinds = _steer(NB, bs, plan, rng, deltas, kinds, sorted(jump_at))
    payload = tokens(slots, bs, deltas, kinds)
    for t in jump_at:
        assert (payload[t] & 0xC0) == 0x80 and classify(payload, N, bs) is None, (t, payload[t])
    img = image_of(W, H, bs, fractal, slots, deltas, kinds)
    blob = header(W, H, bs, fractal) + payload
    if return_info:
        return blob, img, {"n_jump": sum(1 for s in slots if s[1]), "NB": NB, "slots": slots}
    return blob, img


def _steer(NB, bs, plan, rng, deltas, kinds, targets):
    """Re-lay the stream so that a jump byte stands at every payload offset of `targets`.  Far from a target the slots
    follow the plan.  Within six blocks of one they are single blocks whose number of full tokens is capped so that the
    target stays in reach, and the slot that can end on the target gets exactly as many full tokens as that takes; the
    slot behind it is made a pair.  The walk is rebuilt around the changed token kinds."""
    deltas, kinds = list(deltas), list(kinds)
    claimed = np.zeros(NB, bool)
    slots, off, k = [], 0, 0
    targets = list(targets)
    force_pair = bool(targets) and targets[0] == 0
    if force_pair:
        targets.pop(0)
    for i in range(NB):
        if claimed[i]:
            continue
        claimed[i] = True
        free = np.flatnonzero(~claimed[i + 1: min(i + 64, NB)]) + 1
        rel = targets[0] - off if targets else None
        near = rel is not None and rel <= 6 * bs + 1
        assert rel is None or rel >= bs or force_pair, f"jump offset {targets[0]} cannot be reached from {off}"
        want = force_pair or (not near and (plan in ("near", "far", "rand", "half") or (plan == "p50" and rng.random() < 0.5)))
        j = 0
        if want and len(free):
            j = int(free[-1] if plan == "far" else free[0])
            claimed[i + j] = True
        npx = 2 * bs if j else bs
        n_full = sum(1 for t in range(npx) if kinds[k + t] == FULL)
        lo = off + (1 if j else 0) + npx  # where the slot ends without a full token
        force_pair = False
        if near and not j and rel <= 2 * bs:
            n_want = targets.pop(0) - lo
            force_pair = True
        elif near:
            n_want = min(n_full, max(targets[0] - bs - lo, 0))
            assert lo + n_want + bs <= targets[0], f"jump offset {targets[0]} cannot be reached from {off}"
        else:
            n_want = n_full
        for t in range(npx):  # exactly n_want full tokens in this slot
            if n_full < n_want and kinds[k + t] != FULL:
                kinds[k + t], deltas[k + t], n_full = FULL, (deltas[k + t] if kinds[k + t] == SHORT else 0), n_full + 1
            elif n_full > n_want and kinds[k + t] == FULL:
                kinds[k + t], deltas[k + t], n_full = RESERVED, 0, n_full - 1
        off = lo + n_want
        k += npx
        slots.append((i, j))
    assert not targets and not force_pair, f"jump offsets {targets} not reached"
    val = 0
    for t in range(len(deltas)):
        if kinds[t] == RESERVED:
            deltas[t] = 0
            continue
        lim = 2048 if kinds[t] == FULL else 64
        d = max(-lim + 1, min(deltas[t], lim))
        d = max(-val, min(d, 65535 - val))
        deltas[t] = d
        val += d
    return slots, deltas, kinds


def edge_stream(W, H, bs, fractal, plan, rng, k, target, kind, at_offset=None):
    """A well-formed stream whose running value is `target` (0, 65535: decodes; -1, 65536: overflow) at pixel ordinal k
    and stays inside [8, 65527] behind the ramp everywhere else: a ramp of full tokens to a plateau 40 (kind SHORT) or
    1000 (kind FULL) away from the edge, a small jitter on the plateau, one token of `kind` to the target and one back.
    k = 0 is the first pixel (the value before it is 0: only the lower edge is in reach).  With at_offset, k is chosen
    so that the token to the target STARTS at that payload offset (None if this layout has no pixel token there).
    -> (file, image or None, k)."""
    N = W * H
    slots = layout(N // bs, plan, rng)
    dist = 40 if kind == SHORT else 1000
    plateau = 65535 - dist if target > 32768 else dist
    vals = list(np.cumsum(_ramp_only(plateau)))
    ramp = len(vals)
    jit = rng.integers(-3, 4, size=N)
    for t in range(ramp, N):
        vals.append(int(max(plateau - 8, min(vals[-1] + int(jit[t]), plateau + 8))))
    vals = [int(v) for v in vals[:N]]

    def kinds_of(v):
        d = np.diff(np.concatenate(([0], v)))
        return d, np.where((d >= -63) & (d <= 64), SHORT, FULL)

    if at_offset is not None:
        _, kd = kinds_of(vals)
        _, start = stream_positions(slots, bs)
        jumps_before = np.zeros(N, np.int64)
        jumps_before[[int(s0) for (lead, j), s0 in zip(slots, start) if j]] = 1
        offs = np.arange(N) + np.cumsum(jumps_before) + np.concatenate(([0], np.cumsum(kd == FULL)[:-1]))
        hit = np.flatnonzero(offs == at_offset)
        if not len(hit) or hit[0] <= ramp:
            return None  # a jump byte of this layout stands there: the caller takes another seed
        k = int(hit[0])
    assert k == 0 and target in (0, -1) or ramp < k < N, (ramp, k)
    vals[k] = target
    deltas, kinds = kinds_of(vals)
    kinds[k] = kind
    deltas, kinds = [int(d) for d in deltas], [int(x) for x in kinds]
    for d, kd in zip(deltas, kinds):
        assert (-63 <= d <= 64) if kd == SHORT else (-2047 <= d <= 2048), (d, kd)
    payload = tokens(slots, bs, deltas, kinds)
    img = image_of(W, H, bs, fractal, slots, deltas, kinds) if 0 <= target <= 65535 else None
    return header(W, H, bs, fractal) + payload, img, k


def _ramp_only(plateau):
    out, val = [], 0
    while val != plateau:
        d = min(2048, plateau - val)
        out.append(d)
        val += d
    return out


def with_deflate(blob, level=9):
    """the same file with its payload behind zlib.compress and header byte 12 set"""
    import zlib
    return blob[:12] + b"\x01" + zlib.compress(blob[13:], level)


# ---------------------------------------------------------------------------------------------------- judge

def classify(payload, N, bs):
    """payload = token bytes including the trailing EOF byte.  None = well formed, else the name of the defect.
    The contract of DESIGN.md section 1: tokens are walked until N pixels are read (tokens behind pixel N-1 do not exist for
    the decoder).  A jump byte must stand where a slot begins; not directly behind another jump byte; with j != 0,
    F + j < NB and F + j unclaimed, F being the first unclaimed block.  Running out of bytes before pixel N-1 is
    complete, the second byte of a full token included, is truncation."""
    NB = N // bs
    Lr = len(payload) - 1  # the last byte is never read
    pos = 0
    ord_ = 0
    claimed = [False] * NB
    F = 0            # first block in traversal order not yet emitted
    slot_end = 0     # pixel ordinal where the current slot (single block or pair) ends
    prev_jump = False
    while ord_ < N:
        if pos >= Lr:
            return "truncated"
        c = payload[pos]
        if (c & 0xC0) == 0x80:
            if prev_jump:
                return "two_jumps"
            if ord_ != slot_end:
                return "jump_inside_block"
            while F < NB and claimed[F]:
                F += 1
            j = c & 0x3F
            if j == 0 or F + j >= NB or claimed[F + j]:
                return "bad_partner"
            claimed[F] = claimed[F + j] = True
            slot_end = ord_ + 2 * bs
            prev_jump = True
            pos += 1
            continue
        if ord_ == slot_end and not prev_jump:
            while F < NB and claimed[F]:
                F += 1
            claimed[F] = True
            slot_end = ord_ + bs
        prev_jump = False
        if (c & 0xF0) == 0xE0:
            if pos + 1 >= Lr:
                return "truncated"
            pos += 2
        else:
            pos += 1
        ord_ += 1
    return None


def token_table(payload):
    """numpy tokeniser of the readable bytes: (offsets of token starts, is_jump, is_full), all tokens, no pixel limit"""
    b = np.frombuffer(payload, np.uint8)[: max(len(payload) - 1, 0)]
    n = len(b)
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z.astype(bool), z.astype(bool)
    isF = (b & 0xF0) == 0xE0
    idx = np.arange(n)
    # inside a run of F bytes the roles alternate: a byte is a second byte iff the byte before it is an F byte at an
    # even place of its run
    run_start = np.where(isF & ~np.concatenate(([False], isF[:-1])), idx, 0)
    run_start = np.maximum.accumulate(run_start)
    opens = isF & (((idx - run_start) & 1) == 0)
    second = np.concatenate(([False], opens[:-1]))
    opens &= ~second
    starts = ~second
    off = idx[starts]
    return off, ((b & 0xC0) == 0x80)[starts], opens[starts]


def _replay(payload, off, ords, jt, NB, bs, state, record=None):
    """the sequential part of classify_fast over the jump tokens jt, from `state` = (F, slot_end, previous jump's token index,
    partners claimed so far); with `record`, (F, slot_end, token index, partner block) after every jump is appended to it"""
    F, slot_end, prev_tok, claimed = state
    for t in jt:
        o = int(ords[t])
        if t == prev_tok + 1:
            return "two_jumps", None
        if o < slot_end or (o - slot_end) % bs:
            return "jump_inside_block", None
        for _ in range((o - slot_end) // bs):  # single blocks up to this jump
            while F in claimed:
                F += 1
            F += 1
        while F in claimed:
            F += 1
        j = int(payload[int(off[t])]) & 0x3F
        if j == 0 or F + j >= NB or (F + j) in claimed:
            return "bad_partner", None
        claimed.add(F + j)
        F += 1
        slot_end = o + 2 * bs
        prev_tok = t
        if record is not None:
            record.append((F, slot_end, prev_tok, F - 1 + j))
    return None, (F, slot_end, prev_tok, claimed)


class Base:
    """A well-formed payload and the judge's state behind each of its jump bytes: a file damaged at one place shares every
    token before that place with it, and classify_fast(..., base=...) takes the walk up from there."""

    def __init__(self, payload, N, bs):
        self.bytes = np.frombuffer(payload, np.uint8)
        off, isj, _ = token_table(payload)
        ords = np.cumsum(~isj) - ~isj
        self.jt = np.flatnonzero(isj)
        self.joff = off[self.jt]
        self.after = []
        verdict, _ = _replay(payload, off, ords, self.jt.tolist(), N // bs, bs, (0, 0, -2, set()), self.after)
        assert verdict is None and int((~isj).sum()) == N, "the base of a damaged set is well formed, with nothing behind pixel N-1"
        self.partners = [a[3] for a in self.after]


def classify_fast(payload, N, bs, base=None):
    """The same judgement as classify(), for long streams: tokens from token_table(), the sequential part runs over
    the jump bytes only, and with `base` only over those at and behind the first byte that differs from the base.
    tests/test_token_streams_host.py holds this and classify() together on every small damaged stream."""
    NB = N // bs
    Lr = len(payload) - 1
    off, isj, isf = token_table(payload)
    pix = ~isj
    npix = int(pix.sum())
    if npix >= N:
        last = int(np.flatnonzero(pix)[N - 1])  # token index of pixel N-1: nothing behind it exists
        off, isj, isf, pix = off[: last + 1], isj[: last + 1], isf[: last + 1], pix[: last + 1]
    cut_full = len(off) > 0 and bool(isf[-1]) and int(off[-1]) + 1 >= Lr
    ords = np.cumsum(pix) - pix  # pixels before each token
    jt = np.flatnonzero(isj)
    state = (0, 0, -2, set())
    if base is not None and len(jt):
        b = np.frombuffer(payload, np.uint8)
        m = min(len(b), len(base.bytes))
        diff = np.flatnonzero(b[:m] != base.bytes[:m])
        first = int(diff[0]) if len(diff) else m
        # tokens that start before the first differing byte are the base's: same offsets, same kinds, same jump distances
        k0 = min(int(np.searchsorted(base.joff, first)), len(jt))
        if k0:
            assert np.array_equal(off[jt[:k0]], base.joff[:k0])
            F, slot_end, prev_tok, _ = base.after[k0 - 1]
            # partners at or ahead of the frontier come from leaders at most 63 blocks back, hence from the last 63 jumps
            state = (F, slot_end, prev_tok, set(base.partners[max(0, k0 - 64):k0]))
            jt = jt[k0:]
    verdict, _ = _replay(payload, off, ords, jt.tolist(), NB, bs, state)
    if verdict:
        return verdict
    if npix < N or cut_full:
        return "truncated"
    return None


def jump_table(payload, N, bs):
    """of a well-formed payload: [(offset of the jump byte, leader block F, j, blocks F+1 .. F+63 claimed at that time)]"""
    NB = N // bs
    off, isj, _ = token_table(payload)
    ords = np.cumsum(~isj) - ~isj
    claimed, F, slot_end, out = set(), 0, 0, []
    for t in np.flatnonzero(isj).tolist():
        o = int(ords[t])
        if o >= N:
            break
        for _ in range((o - slot_end) // bs):
            while F in claimed:
                F += 1
            F += 1
        while F in claimed:
            F += 1
        j = payload[int(off[t])] & 0x3F
        out.append((int(off[t]), F, j, [x - F for x in range(F + 1, min(F + 64, NB)) if x in claimed]))
        claimed.add(F + j)
        F += 1
        slot_end = o + 2 * bs
    return out


# ---------------------------------------------------------------------------------------------------- damage

def _file(head, payload):
    return head + bytes(payload)


def damage(blob, N, bs, rng, n_flips=0, n_bytes=0, n_cuts=0, n_jump_edits=0, n_append=0, boundaries=()):
    """Seeded damage of a well-formed raw file: a list of (name, file bytes).
    n_flips single-bit flips of the payload; n_bytes each of one byte deleted / inserted / duplicated; cuts at every kind
    of place plus n_cuts random ones; n_jump_edits each of the jump edits; n_append files with tokens behind pixel N-1
    (well formed: they must decode); the edits aimed at every payload offset of `boundaries` (b-1 | b)."""
    head, pay = blob[:13], blob[13:]
    L = len(pay)
    out = []
    for _ in range(n_flips):
        bit = int(rng.integers(0, L * 8))
        p = bytearray(pay)
        p[bit >> 3] ^= 1 << (bit & 7)
        out.append(("flip", _file(head, p)))
    for _ in range(n_bytes):
        at = int(rng.integers(0, L - 1))
        out.append(("delete", _file(head, pay[:at] + pay[at + 1:])))
        out.append(("insert", _file(head, pay[:at] + bytes([int(rng.integers(0, 256))]) + pay[at:])))
        out.append(("duplicate", _file(head, pay[:at + 1] + pay[at:])))
    off, isj, isf = token_table(pay)
    fulls = off[isf]
    if n_cuts:
        out.append(("cut_empty", _file(head, b"")))
        out.append(("cut_eof_only", _file(head, b"\x3b")))
        out.append(("cut_one_byte_short", _file(head, pay[:-2] + b"\x3b")))
        out.append(("cut_one_pixel_short", _file(head, pay[:int(off[-1])] + b"\x3b")))
        out.append(("cut_no_eof", _file(head, pay[:-1])))  # the last token byte takes the place of the unread byte
        if len(fulls):
            out.append(("cut_in_last_full", _file(head, pay[:int(fulls[-1]) + 1] + b"\x3b")))
        # the stream ends inside the full token that is pixel N-1: only its second byte is missing
        p = bytearray(pay[:int(off[-1])]) + bytes([0xE0, 0x3B])
        out.append(("cut_second_byte_of_last_pixel", _file(head, p)))
        out.append(("whole_last_pixel_full", _file(head, bytearray(pay[:int(off[-1])]) + bytes([0xE0, 0x00, 0x3B]))))
        for _ in range(n_cuts):
            at = int(rng.integers(1, L - 1))
            out.append(("cut", _file(head, pay[:at] + b"\x3b")))
            if len(fulls):
                f = int(fulls[int(rng.integers(0, len(fulls)))])
                out.append(("cut_in_full", _file(head, pay[:f + 1] + b"\x3b")))
    jt = jump_table(pay, N, bs) if (n_jump_edits or boundaries) else []
    NB = N // bs
    for _ in range(n_jump_edits if jt else 0):
        o, F, j, cl = jt[int(rng.integers(0, len(jt)))]
        out += _jump_edits(head, pay, o, F, j, cl, NB)
        beyond = [x for x in jt if x[1] + 63 >= NB]
        if beyond:
            o, F, j, cl = beyond[int(rng.integers(0, len(beyond)))]
            p = bytearray(pay)
            p[o] = 0x80 | int(rng.integers(NB - F, 64)) if NB - F < 64 else 0x80
            out.append(("jump_beyond_last", _file(head, p)))
    for _ in range(n_append):
        tail = bytes(int(x) for x in rng.integers(0, 256, size=int(rng.integers(1, 40))))
        if rng.random() < 0.5:  # jump bytes behind the last pixel, where no block is left to pair
            tail = bytes([0x80 | int(rng.integers(0, 64))]) + tail
        out.append(("append", _file(head, pay[:-1] + tail + b"\x3b")))
    starts = set(off.tolist())
    jumps_at = {x[0]: x for x in jt}
    for b in boundaries:
        if not 2 <= b < L - 3:
            continue
        # two bytes written over b-1 | b, after making b-1 a token start
        for name, pair in (("aim_two_jumps", (0x81, 0x81)), ("aim_full_straddles", (0xE0, 0x05)), ("aim_full_up", (0xE7, 0xFF)),
                           ("aim_jump_then_pixel", (0x81, 0x01)), ("aim_pixel_then_jump", (0x01, 0x82)),
                           ("aim_F_run", (0xE0, 0xE0))):
            p = bytearray(pay)
            if (b - 1) not in starts:
                p[b - 2] = 0x00
            p[b - 1], p[b] = pair
            out.append((f"{name}@{b}", _file(head, p)))
        for at in (b - 1, b):
            out.append((f"aim_cut@{at}", _file(head, pay[:at] + b"\x3b")))
            out.append((f"aim_delete@{at}", _file(head, pay[:at] + pay[at + 1:])))
            for bit in (7, 6, 5, 0):
                p = bytearray(pay)
                p[at] ^= 1 << bit
                out.append((f"aim_flip{bit}@{at}", _file(head, p)))
            if at in jumps_at:  # the writer put a jump byte here (build(..., jump_at=...)): the jump edits on it
                o, F, j, cl = jumps_at[at]
                out += [(f"aim_{n}@{at}", f) for n, f in _jump_edits(head, pay, o, F, j, cl, NB)]
    return out


def _jump_edits(head, pay, o, F, j, cl, NB):
    out = []
    p = bytearray(pay)
    p[o] = 0x80
    out.append(("jump_zero", _file(head, p)))
    if cl:
        p = bytearray(pay)
        p[o] = 0x80 | cl[len(cl) // 2]
        out.append(("jump_onto_claimed", _file(head, p)))
    if F + 63 >= NB:
        p = bytearray(pay)
        p[o] = 0x80 | 63
        out.append(("jump_beyond_last", _file(head, p)))
    out.append(("jump_doubled", _file(head, pay[:o] + pay[o:o + 1] + pay[o:])))
    n = 2 if (pay[o + 1] & 0xF0) == 0xE0 else 1  # the jump byte moved one token into its block
    out.append(("jump_moved_in", _file(head, pay[:o] + pay[o + 1:o + 1 + n] + pay[o:o + 1] + pay[o + 1 + n:])))
    return out


def oracle_verdict(blob, bs):
    """('pixels', raster bytes) | ('overflow', None) | ('stream', None) from the CPU oracle"""
    try:
        return "pixels", oracle.decode(blob, block_size=bs)
    except oracle.OracleError as e:
        if e.code == oracle.E_OVERFLOW:
            return "overflow", None
        if e.code == oracle.E_STREAM:
            return "stream", None
        raise


def boundaries_for(threads=(256, 512, 1024)):
    """the payload offsets the parse is built around: the first segment boundary and a step of every workgroup size"""
    return (SEG,) + tuple(t * SEG for t in threads)


# ---------------------------------------------------------------------------------------------------- the cases of the tests

def _plans_of(W, H, bs):
    return PLANS if (W, H, bs) in ((64, 64, 16), (512, 512, 16)) else ("far", "rand")


SHAPES = [  # (W, H, block size, fractal)
    (64, 64, 16, True), (512, 512, 16, True), (1024, 1024, 4, True),
    (128, 128, 4, True), (128, 128, 8, True), (128, 128, 32, True), (48, 80, 64, True),
    (96, 65, 5, True), (384, 384, 12, True), (768, 768, 3, True),
    (1, 1024, 16, True), (1024, 1, 16, True), (20, 20, 16, True),
    (128, 128, 16, False),
]
WELL_FORMED = [(W, H, bs, fr, plan) for (W, H, bs, fr) in SHAPES for plan in _plans_of(W, H, bs)]
_cache = {}


def well_formed(case):
    """(file, image, info) of one row of WELL_FORMED; the farthest-partner rows climb to 65535 and stay near it"""
    if case not in _cache:
        W, H, bs, fr, plan = case
        rng = np.random.default_rng([W, H, bs, int(fr), PLANS.index(plan)])
        _cache[case] = build(W, H, bs, fr, plan, rng, bias=0.5 if plan == "far" else 0.0, return_info=True)
    return _cache[case]


DAMAGED_SHAPES = [(64, 64, 16), (128, 128, 4), (96, 65, 5), (512, 512, 16), (1024, 1024, 4)]


def damaged_set(W, H, bs, threads=(256, 512, 1024)):
    """The damaged files of one shape: [(name, seed tag, file bytes, Base of the file it was made from)], deterministic.
    Thousands on 64x64, a few hundred on the larger shapes.  Every set starts from bases whose jump bytes stand on the
    boundaries that the shape's payload reaches."""
    N = W * H
    small = N <= 16384
    out = []
    bounds = boundaries_for(threads)
    bases = (("p50", 0.2, 0.0), ("p50", 1.0, 0.3), ("near", 0.3, 0.6)) if small else (("p50", 0.25, 0.4),)
    for bi, (plan, full_p, bias) in enumerate(bases):
        rng = np.random.default_rng([W, H, bs, 77, bi])
        approx = int(N * (1 + full_p))
        # jump bytes on b-1 of one boundary and on b of the next one the payload reaches (a slot holds >= bs bytes)
        reach = [b for b in bounds if b + 64 < approx and b >= bs]
        jump_at = [b - (1 if (k + bi) % 2 == 0 and b - 1 >= bs else 0) for k, b in enumerate(reach)]
        blob, img = build(W, H, bs, True, plan, rng, full_p=full_p, reserved_p=0.03, bias=bias, jump_at=jump_at)
        base = Base(blob[13:], N, bs)
        if N == 4096:
            kw = dict(n_flips=1500, n_bytes=60, n_cuts=25, n_jump_edits=25, n_append=25)
        elif small:
            kw = dict(n_flips=150, n_bytes=12, n_cuts=8, n_jump_edits=8, n_append=8)
        elif N <= 512 * 512:
            kw = dict(n_flips=100, n_bytes=8, n_cuts=5, n_jump_edits=8, n_append=8)
        else:
            kw = dict(n_flips=60, n_bytes=5, n_cuts=3, n_jump_edits=5, n_append=5)
        items = damage(blob, N, bs, rng, boundaries=[b for b in bounds if b < len(blob) - 16], **kw)
        out += [(name, f"{W}x{H}/{bs} base {bi} #{k}", f, base) for k, (name, f) in enumerate(items)]
    return out
