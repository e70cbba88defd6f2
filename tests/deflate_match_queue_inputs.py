"""Inputs for the two queues of dfl_match_kernel (csrc/deflate_kernels.hip) and a host model of how the kernel fills them.

The kernel visits the positions of a slice in (hash, position) order, 64 per wave and turn, and queues a position for
  kind 2 (run list):   its string starts with three equal bytes, unless the chain head p-1 already reaches nice_match
                       (in[p-1] == in[p] and the run ahead of p is at least min(nice_match, lookahead) long);
  kind 1 (heavy list): otherwise, when more than LIGHT_STEPS earlier positions share its hash inside the window.
A wave collects both kinds in regions of REGION entries and flushes a region after its last turn, and earlier whenever fewer
than 64 entries are free after a turn.  The inputs here aim at that bookkeeping, not at the matching rules: matches stay short
(runs below nice_match at level 9, strings of three or four bytes), so no chain walk ends early and the model below is exact.
tests/test_deflate_match_queue_inputs_host.py checks the claims, tests/test_gpu_deflate_match_queue.py runs the kernels."""
import functools

import numpy as np

import deflate_match_inputs as dmi

REGION = 256          # MATCH_Q of deflate_kernels.hip: entries per wave and list
FLUSH_ABOVE = REGION - 64  # a list is flushed when it holds more than this after a turn
BLOCK = 256           # lanes per workgroup: four waves of 64
GRID_COMPACT, GRID_COMPACT_MIN, GRID_WIDE = 256, 32, 2048  # workgroups per slice at most (launch_deflate)
NICE = {4: 16, 9: 258}


def in_stride(longest):
    """deflate_in_stride of csrc/deflate_workspace.h"""
    return (longest + 16 + 255) & ~255


def nparts(longest, n, compact=True):
    """workgroups per slice of dfl_match_kernel in a batch of n slices whose longest has `longest` bytes (launch_deflate: with
    compact records, as few as still fill an XCD with the slices it works through, from GRID_COMPACT down to GRID_COMPACT_MIN)"""
    cap = max(GRID_COMPACT_MIN, GRID_COMPACT // ((n + 7) // 8)) if compact else GRID_WIDE
    return min(cap, in_stride(longest) // 256)


# ------------------------------------------------------------------------------------------------------- inputs
def _tail(n=16):
    """bytes that end an input: no string of them occurs before, none starts a run"""
    return bytes(range(0xF0, 0xF0 + n))


@functools.lru_cache(maxsize=None)
def queue_heavy(L, seed=1):
    """back-to-back runs of 20 .. 60 equal bytes, each run's byte different from the one before: every position of a run but
    its last two starts three equal bytes"""
    rng = np.random.default_rng(seed)
    nruns = L // 20 + 2
    lens = rng.integers(20, 61, nruns)
    step = rng.integers(1, 0xEF, nruns)          # byte of run k = byte of run k-1 + step (mod 0xEF): never the same, never a tail byte
    vals = (np.cumsum(step) % 0xEF).astype(np.uint8)
    body = np.repeat(vals, lens)[:max(L - 16, 0)].tobytes()
    return (body + _tail())[:L]


@functools.lru_cache(maxsize=None)
def heavy_chain(L, seed=2):
    """units X_j Y_j Z_j f g over 32 trigrams (X, Y, Z from three disjoint sets): a trigram recurs every 160 bytes, about 200
    times inside the window, and the pair (f, g) behind it never twice there, so a match has three or four bytes; f and g
    come from a fourth set, so no three equal bytes occur"""
    k = np.arange(L // 5 + 1, dtype=np.int64)
    k = k + seed * 7
    j = k % 32
    f = 100 + k % 130
    g = 100 + (k // 2080 + 3 * k) % 130          # 2080 = lcm(32, 130): where (j, f) comes again, g has moved on
    u = np.stack([1 + j, 33 + j, 65 + j, f, g], axis=1).astype(np.uint8).reshape(-1)
    body = u[:max(L - 16, 0)].tobytes()
    return (body + _tail())[:L]


@functools.lru_cache(maxsize=None)
def mix(L, run_share=0.5, seed=3):
    """segments of queue_heavy and heavy_chain in turn, about `run_share` of the bytes in runs"""
    rng = np.random.default_rng(seed)
    a, b = queue_heavy(L + 64, seed + 10), heavy_chain(L + 64, seed + 20)
    out, pa, pb = bytearray(), 0, 0
    while len(out) < L:
        n = int(rng.integers(300, 900))
        if rng.random() < run_share:
            out += a[pa:pa + n]; pa += n
        else:
            m = n - n % 5                         # whole units: the trigram order continues across segments
            out += b[pb:pb + m]; pb += m
    return bytes(out[:max(L - 16, 0)] + _tail())[:L]


# ------------------------------------------------------------------------------------------------------- the kernel's rules
@functools.lru_cache(maxsize=None)
def kinds(data, level, hash_bits=15):
    """(order, kind): the positions 0 .. L-3 in (hash, position) order and, for each of them in that order, 0, 1 or 2"""
    L = len(data)
    if L < 3:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    a = np.frombuffer(data, dtype=np.uint8)
    npos = L - 2
    h = dmi.hashes(data, hash_bits)
    order = np.argsort(h, kind="stable")
    # run length ahead of every position (capped by the end of the input and MAX_MATCH)
    last = np.flatnonzero(np.append(a[:-1] != a[1:], True))  # last position of every run
    run = np.minimum(last[np.searchsorted(last, np.arange(L))] - np.arange(L) + 1, dmi.MAX_MATCH)
    pos = np.arange(npos)
    three = run[:npos] >= 3
    has_prev = np.zeros(npos, bool)
    has_prev[2:] = a[1:npos - 1] == a[2:npos]     # position 0 is NIL: p >= 2
    nice_eff = np.minimum(L - pos, NICE[level])
    kind2 = three & ~(has_prev & (run[:npos] >= nice_eff))
    hs, ps = h[order], order
    far = np.zeros(npos, bool)                    # a 13th chain entry: same hash, inside the window, not position 0
    k = dmi.LIGHT_STEPS + 1
    far[k:] = (hs[k:] == hs[:-k]) & (ps[:-k] >= np.maximum(1, ps[k:] - dmi.MAX_DIST + 1))
    kind = np.where(kind2[order], 2, np.where(far & ~three[order], 1, 0))
    return order, kind


def wave_fills(data, level, parts, hash_bits=15):
    """What each wave's two regions hold after each of its turns, before the flush test: a list of (kind, fill, whether the
    wave has another turn to make) over all waves and turns, and the number of flushes that happen before a wave's last turn"""
    _, kind = kinds(data, level, hash_bits)
    npos = len(kind)
    fills, mid_flushes = [], 0
    turns = -(-npos // (parts * BLOCK)) if npos else 0
    pad = np.zeros(turns * parts * BLOCK, np.int64)
    pad[:npos] = kind
    t = pad.reshape(turns, parts, BLOCK // 64, 64) if turns else pad.reshape(0, parts, 4, 64)
    for which in (1, 2):
        c = (t == which).sum(axis=3)              # [turn, part, wave]
        fill = np.zeros(c.shape[1:], np.int64)
        for turn in range(turns):
            live = (np.arange(parts) + turn * parts) * BLOCK < npos  # the workgroup makes this turn
            nxt = (np.arange(parts) + (turn + 1) * parts) * BLOCK < npos  # ... and another one after it
            fill = fill + c[turn]
            fills += [(which, int(x), bool(m)) for x, m in zip(fill[live].reshape(-1), np.repeat(nxt[live], BLOCK // 64))]
            over = (fill > FLUSH_ABOVE) & live[:, None]
            mid_flushes += int((over & nxt[:, None]).sum())
            fill = np.where(over, 0, fill)
    return fills, mid_flushes


def share(data, level, which):
    _, kind = kinds(data, level)
    return float((kind == which).mean()) if len(kind) else 0.0


# ------------------------------------------------------------------------------------------------------- batches
BIG = (1 << 20) + 12345        # waves make 33 turns (compact records, nine slices) and flush in mid-loop
WIDE_GRID = GRID_WIDE * BLOCK  # npos of a multiple of the grid with wide records, in a batch with BIG
COMPACT_GRID = GRID_COMPACT * BLOCK
MIN_GRID = GRID_COMPACT_MIN * BLOCK
# level 9, compact records, the longest slice of batch "boundaries": some wave's run list holds exactly FLUSH_ABOVE - 1,
# FLUSH_ABOVE and FLUSH_ABOVE + 1 entries after a turn that is not its last (checked by the host test)
BOUNDARY_SIZES = (300000, 300001, 300002)
BOUNDARY_SHARE = 0.8
# wide records: 2048 workgroups per slice, so only a slice of more than four times WIDE_GRID positions has waves that queue
# more run positions than a region holds (level 9); it goes through the wide kernels alone
WIDE_LONG = 4 * WIDE_GRID + 70000


def wide_long():
    return [queue_heavy(WIDE_LONG)]


def batches():
    """name -> list of slices; batches of 1, 7, 9 and 61 slices, long and short slices together"""
    return {
        # nine slices: the long one, npos on a multiple of the wide grid and one either side, and the shortest
        "long_and_short": [mix(BIG, 0.9), queue_heavy(WIDE_GRID + 1), queue_heavy(WIDE_GRID + 2), queue_heavy(WIDE_GRID + 3),
                           b"", queue_heavy(3), queue_heavy(65), heavy_chain(66), mix(67)],
        # seven: npos on a multiple of the compact grid and one either side, the flush boundaries, heavy chains
        "boundaries": [queue_heavy(COMPACT_GRID + 1), queue_heavy(COMPACT_GRID + 2), queue_heavy(COMPACT_GRID + 3)]
                      + [mix(n, BOUNDARY_SHARE) for n in BOUNDARY_SIZES] + [heavy_chain(40000)],
        "one": [mix(100000)],
        # nine short ones: fewer workgroups per slice than the grid's cap, one turn each
        "short": [queue_heavy(1), queue_heavy(2), queue_heavy(5000), heavy_chain(5000), mix(5000), heavy_chain(20000),
                  queue_heavy(300), mix(30000), b""],
        # 61 slices, enough for the smallest grid: waves make up to 14 turns; npos on a multiple of that grid and one either side
        "many": [mix(60000 + 901 * k, 0.9, seed=k) for k in range(58)]
                + [queue_heavy(MIN_GRID + 1), queue_heavy(MIN_GRID + 2), queue_heavy(MIN_GRID + 3)],
    }
