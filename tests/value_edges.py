"""Inputs that put 16-bit pixel values and deltas on the edges where the encode kernels change their arithmetic.

The three implementations of stage (i) choose shortcuts by the values they see: encode_stream.hip works in packed 16-bit
arithmetic while every pixel of a group of tiles, of its 64-block look-ahead and the one pixel before it is < 0x4000, skips
the Q7 test (a delta outside [-2047, 2048]) unless one of them is >= 0x0800, and is exact otherwise; encode_tiles.hip decides
per wave, encode_kernels.hip is exact throughout.  Every builder here returns (name, image, expectations) and asserts, with
the CPU oracle's partition and statistics, the precondition that makes its case mean something: a case that no longer reaches
its regime, its pairs or its one violation fails on the CPU instead of silently testing less.

A case is described by a spec (a small dict).  Specs of the families that need a seeded search (a pixel position or a seed
with a certain partition around it) are resolved once by oracle/gen_value_edges_golden.py and stored, resolved, in
tests/golden/value_edges.json next to what the reference codec made of the image; build() never searches.

Families: tok (token and difficult-block thresholds), q7 (deltas of exactly +-2047 / 2048 / 2049 at chosen places of the final
order), one (the single large pixel of an 11-bit slice and where it sits relative to a group boundary of the streaming
kernel), fit (partner tests at their comparison edges) and full (the whole 16-bit range, unsigned and signed)."""
import functools
import json
import os
import types

import numpy as np

from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_JSON = os.path.join(HERE, "golden", "value_edges.json")

TILE_SIDES = (128, 256, 512, 1024)     # squares the streaming and the tile kernel take at block size 16
ALL_BS_SHAPE = (60, 64)                # 3840 pixels: divisible by 4, 5, 8, 12, 16, 32 and 64
OTHER_BS = (4, 8, 32, 64, 5, 12)
Q7_DELTAS = (-2049, -2048, -2047, 2047, 2048, 2049)


def violates(d):
    return d < -2047 or d > 2048


# ---------------------------------------------------------------------------------------------------- analysis
def analyse(img, bs=16):
    """The oracle's view of a slice: traversal, partition, final order and its deltas, and what kind of place every position of
    the final order is ('pair', 'lone_p0', 'lone_after_meshed_p0', 'lone_pk')."""
    img = np.ascontiguousarray(img)
    w, h = img.shape
    N = w * h
    NB = N // bs
    order = oracle.curve(w, h)
    flat = img.reshape(-1)
    trav = flat[order]
    po, jumps = oracle.partition(trav.astype(np.int32), order, bs)   # segmentation sees signed values of int16 input
    fin = flat[po].view(np.uint16).astype(np.int64)                  # tokens see the unsigned bytes
    d = np.diff(fin, prepend=0)
    role = np.zeros(NB, dtype=np.int8)                               # 0 alone, 1 leader, 2 partner
    for a_, b_ in jumps.items():
        role[a_], role[b_] = 1, 2
    emitted = np.flatnonzero(role != 2)
    length = np.where(role[emitted] == 1, 2 * bs, bs)
    start = np.concatenate([[0], np.cumsum(length)[:-1]])
    assert int(start[-1] + length[-1]) == N
    assert np.array_equal(po[start], order[emitted * bs]), "the final order is not the item order this analysis assumes"
    item_of = np.repeat(np.arange(len(emitted)), length)
    within = np.arange(N) - start[item_of]
    blk = emitted[item_of]
    after_meshed = (blk > 0) & (role[np.maximum(blk - 1, 0)] != 0)
    kind = np.where(role[blk] == 1, "pair", np.where(within > 0, "lone_pk", np.where(after_meshed, "lone_after_meshed_p0", "lone_p0")))
    out, st = oracle.encode(img, block_size=bs, deflate=False, return_stats=True)
    two = (d < -63) | (d > 64)
    bad = (d < -2047) | (d > 2048)
    assert int(two.sum()) == st.n_full and int(bad.sum()) == st.q7_violations and len(jumps) == st.n_jump
    inv = np.empty(N, dtype=np.int64)
    inv[order] = np.arange(N)
    # traversal deltas as the segmentation sees them (signed values of int16 input); P[0] = 0
    sd = np.diff(trav.astype(np.int64), prepend=trav[:1].astype(np.int64)).reshape(NB, bs)
    large = (sd < -64) | (sd > 64)
    chg = large[:, 1:].sum(axis=1)
    difficult = 2 * chg >= bs                                         # 8 large deltas among pixels 1..15 at block size 16
    assert int(difficult.sum()) == st.n_difficult
    return types.SimpleNamespace(img=img, bs=bs, N=N, NB=NB, order=order, inv=inv, trav=trav, po=po, jumps=jumps, fin=fin, d=d,
                                 role=role, emitted=emitted, start=start, kind=kind, blk=blk, within=within, stats=st,
                                 payload=out[13:], bad=np.flatnonzero(bad), sd=sd, large=large, chg=chg, difficult=difficult)


def stream_regimes(img, tpg):
    """(wide, big) of every group of the streaming kernel with tpg tiles per workgroup: a pixel >= 0x4000 / >= 0x0800 among the
    group's 256 tpg blocks, the 64 blocks after it and the last traversal pixel before it.  int16 input is always wide."""
    w, h = img.shape
    assert w == h and w in TILE_SIDES
    trav = img.reshape(-1)[oracle.curve(w, h)].view(np.uint16)
    nbg = 256 * tpg * 16
    out = []
    for lo in range(0, trav.size, nbg):
        m = int(trav[max(lo - 1, 0):min(trav.size, lo + nbg + 64 * 16)].max())
        out.append((img.dtype.kind == "i" or m >= 0x4000, m >= 0x0800))
    return out


def first_item_at(an, G):
    """index (into an.emitted) of the first emitted item whose leading block is >= G"""
    return int(np.searchsorted(an.emitted, G))


def along(shape, dtype, seq):
    """the image whose traversal reads seq"""
    w, h = shape
    img = np.zeros(w * h, dtype=dtype)
    img[oracle.curve(w, h)] = np.asarray(seq).astype(dtype)
    return img.reshape(w, h)


def _shape(spec):
    return tuple(spec["shape"])


def _regime_sets(img):
    if img.shape[0] == img.shape[1] and img.shape[0] in TILE_SIDES:
        return {tpg: stream_regimes(img, tpg) for tpg in (1, 2, 4)}
    return {}


# ---------------------------------------------------------------------------------------------------- tok
_LARGE = (-66, -65, 65, 66)
_CALM = (-63, 0, 0, 63, 64)


def _pick(rng, choices, v, centre):
    c = [x for x in choices if (x <= 0 if v - centre > 120 else x >= 0 if v - centre < -120 else True)] or list(choices)
    return int(c[int(rng.integers(0, len(c)))])


def build_tok(spec):
    """Traversal deltas from {-66, -65, -64, -63, 0, 63, 64, 65, 66} on five plateaus (1000, around 0x0800, around 0x4000, 0x8000,
    under 65535).  A block has 0, 6, 7, 8 or 9 large deltas (|d| >= 65) among its pixels 1..15 (8 make it difficult; at another
    block size: around half of it), with or without -64 among the others (two bytes, yet not large) and with an entering delta of
    -64, 64, 65 or 0.  The last 64 blocks of a plateau are calm and the ramp to the next one (steps of 2000) has too few steps
    per block to be difficult, so no pair reaches across plateaus and no delta of the final order leaves [-2047, 2048]."""
    shape, bs = _shape(spec), spec["bs"]
    rng = np.random.default_rng([spec["seed"], shape[0], shape[1], bs])
    N = shape[0] * shape[1]
    NB = N // bs
    centres = tuple(spec["plateaus"])                        # five on the tiled shapes, two or one where the slice has few blocks
    ends = np.round(np.cumsum({5: (0.32, 0.26, 0.14, 0.14, 0.14), 2: (0.5, 0.5), 1: (1.0,)}[len(centres)]) * NB).astype(int)
    seq = np.empty(N, dtype=np.int64)
    v = min(centres[0], 2048)                                # the first delta, from the implicit 0, stays inside the format
    thr = (bs + 1) // 2                                      # large deltas that make a block difficult
    for b in range(NB):
        idx = int(np.searchsorted(ends, b, side="right"))
        centre = centres[idx]
        k = min(bs - 1, max(0, (0, thr - 2, thr - 1, thr, thr + 1)[b % 5]))
        if ends[idx] - b <= 64 and idx < len(centres) - 1:
            k = 0
        with_m64 = (b // 5) % 2 == 1
        enter = (-64, 64, 65, 0)[(b // 10) % 4]
        where = set(rng.choice(np.arange(1, bs), size=k, replace=False).tolist())
        calm = _CALM + ((-64, -64) if with_m64 else ())
        ramp = False
        for i in range(bs):
            if abs(v - centre) > 700 or ramp:               # the ramp to the next plateau; its last block stays calm to its end
                ramp = True
                dl = int(np.clip(centre - v, -2000, 2000)) if 1 <= i < thr and abs(v - centre) > 700 else 0
            elif i == 0:
                dl = enter if abs(v + enter - centre) < 300 else 0
            elif i in where:
                dl = _pick(rng, _LARGE, v, centre)
            else:
                dl = _pick(rng, calm, v, centre)
            v += dl
            seq[b * bs + i] = v
    assert seq.min() >= 0 and seq.max() <= 65535
    for edge in set(centres) & {0x0800, 0x4000, 0x8000}:       # values on both sides of every edge, close to it
        assert ((seq >= edge - 200) & (seq < edge)).any() and ((seq >= edge) & (seq < edge + 200)).any(), edge
    assert seq.max() > 65535 - 400 or 65535 - 400 not in centres
    img = along(shape, np.uint16, seq)
    an = analyse(img, bs)
    exp = {"q7": 0}
    assert an.stats.q7_violations == 0
    on_plateau = np.abs(an.sd).max(axis=1) <= 66
    m64 = ((an.sd[:, 1:] == -64).sum(axis=1) > 0) & on_plateau
    drawn = set(np.unique(an.sd[on_plateau]))
    assert drawn == {-66, -65, -64, -63, 0, 63, 64, 65, 66} if NB >= 200 else drawn >= {-65, -64, 64, 65}
    for k in (thr - 1, thr):                                  # 7 and 8 at block size 16
        assert (m64 & (an.chg == k)).sum() > 0 and (~m64 & on_plateau & (an.chg == k)).sum() > 0, k
        assert (on_plateau & (an.chg == k) & (an.sd[:, 0] == -64)).sum() > 0, k
    assert an.stats.n_difficult >= NB // 8 and an.stats.n_jump > 0
    exp["n_difficult"] = int(an.stats.n_difficult)
    reg = _regime_sets(img)
    if reg:
        seen = set().union(*[set(r) for r in reg.values()])
        assert seen == {(False, False), (False, True), (True, True)}, seen
        exp["regimes"] = sorted(map(list, seen))
    return spec["name"], img, exp


# ---------------------------------------------------------------------------------------------------- q7
def _q7_base(spec):
    """blocks of texture (levels within 256 of the base: difficult, many pairs) among flat ones (a lone block after a meshed one)"""
    shape, bs = _shape(spec), spec["bs"]
    rng = np.random.default_rng([spec["seed"], shape[0], shape[1], bs])
    NB = shape[0] * shape[1] // bs
    level = {"packed": 0x2000, "wide": 0x5000}[spec["regime"]]
    tex = rng.integers(0, 256, (NB, bs))
    flat = 128 + rng.integers(-3, 4, (NB, bs))
    seq = (level + np.where(rng.random(NB)[:, None] < 0.6, tex, flat)).reshape(-1)
    # the slice starts from the implicit 0: climb in steps the format carries, too few per block to make a block difficult
    val, ramp, thr = 0x0800, [0x0800], (bs + 1) // 2
    while val < level + 128 or len(ramp) % bs:
        if val < level + 128 and 1 <= len(ramp) % bs < thr:
            val = min(val + 2048, level + 128)
        ramp.append(val)
    seq[:len(ramp)] = ramp
    return along(shape, np.uint16, seq), len(ramp)


def _q7_plant(img, an, f, delta):
    """position f of the final order gets the value delta above its predecessor; the one after it comes back by 2047"""
    out = img.copy()
    u = int(an.fin[f - 1])
    flat = out.reshape(-1)
    flat[an.po[f]] = u + delta
    flat[an.po[f + 1]] = u + delta - (2047 if delta > 0 else -2047)
    return out


def _q7_check(spec, base_an, img, f):
    an = analyse(img, spec["bs"])
    ok = (an.jumps == base_an.jumps and an.kind[f] == spec["place"] and int(an.d[f]) == spec["delta"]
          and an.bad.tolist() == ([f] if violates(spec["delta"]) else []))
    return ok, an


def resolve_q7(spec):
    base, _ = _q7_base(spec)
    an = analyse(base, spec["bs"])
    cand = np.flatnonzero(an.kind == spec["place"])
    cand = cand[(cand >= 1) & (cand < an.N - 1)]
    rng = np.random.default_rng(7)
    for f in rng.permutation(cand)[:400]:
        if _q7_check(spec, an, _q7_plant(base, an, int(f), spec["delta"]), int(f))[0]:
            return dict(spec, at=int(f))
    raise AssertionError(f"no place found for {spec['name']}")


def build_q7(spec):
    """One delta of exactly spec['delta'] at position spec['at'] of the final order, which is a place of kind spec['place'];
    every other delta is inside [-2047, 2048], the partition is the one of the slice without it, and every pixel is inside
    [0x0800, 0x4000) ('packed': packed arithmetic with the Q7 test) or, after the climb from the implicit 0 in the first blocks,
    >= 0x4000 ('wide')."""
    base, climb = _q7_base(spec)
    an0 = analyse(base, spec["bs"])
    img = _q7_plant(base, an0, spec["at"], spec["delta"])
    ok, an = _q7_check(spec, an0, img, spec["at"])
    assert ok, spec["name"]
    want = int(violates(spec["delta"]))
    assert an.stats.q7_violations == want
    if spec["regime"] == "packed":
        assert img.min() >= 0x0800 and img.max() < 0x4000
    else:
        assert an.trav[climb:].min() >= 0x4000                   # all but the climb from the implicit 0
    for tpg, reg in _regime_sets(img).items():
        assert set(reg) == {(spec["regime"] == "wide", True)}
    return spec["name"], img, {"q7": want, "at": spec["at"]}


# ---------------------------------------------------------------------------------------------------- one
_ONE_VALUES = {"v11": (4095, 2047), "v14": (65535, 65475)}     # the large pixel and what its traversal predecessor is set to


def _one_classes(NB):
    return {"tpg1": [G for G in range(256, NB, 512)], "tpg2": [G for G in range(512, NB, 1024)], "tpg4": [G for G in range(1024, NB, 1024)]}


def _one_make(spec, seed, G):
    """-> (image, analysis, traversal position of the large pixel) or None if the structure the placement needs is not there"""
    shape, bs = _shape(spec), spec["bs"]
    place, (big, prev) = spec["place"], _ONE_VALUES[spec["value"]]
    base = np.random.default_rng(seed).integers(0, 2048, shape).astype(np.uint16)
    an = analyse(base, bs)

    def structure(a):
        it = first_item_at(a, G)
        tpos = int(a.inv[a.po[a.start[it] - 1]])          # traversal position of the final-order predecessor of the boundary
        if place == "pred_pair":
            return (tpos if a.role[G - 1] == 2 and a.role[G] == 1 and tpos // bs < G - 1 else None)
        if place == "pred_lone":
            return (tpos if a.role[G - 1] == 2 and a.role[G] == 0 and tpos // bs < G - 1 else None)
        if place == "before":
            return (tpos if a.role[G - 1] == 0 and a.role[G] != 2 and tpos == G * bs - 1 else None)
        return {"inside": (G + min(128, a.NB // 4)) * bs + 7, "lookahead": (G + 10) * bs + 7}[place]

    tpos = structure(an)
    if tpos is None:
        return None
    seq = an.trav.astype(np.int64).copy()
    seq[tpos] = big
    if place.startswith("pred") or spec["value"] == "v11":
        seq[tpos - 1] = prev
    if place == "pred_pair" or place == "pred_lone":
        if spec["value"] == "v14":
            seq[G * bs] = 5
    img = along(shape, np.uint16, seq)
    an2 = analyse(img, bs)
    if structure(an2) != tpos:
        return None
    return img, an2, tpos


def _one_expect(spec, img, an, tpos, G):
    """the precondition of a case of this family, or None if (seed, G) does not give it"""
    bs = spec["bs"]
    place, value = spec["place"], spec["value"]
    threshold = 0x0800 if value == "v11" else 0x4000
    assert int((an.trav.view(np.uint16) >= threshold).sum()) == (1 if (value == "v11" or not place.startswith("pred")) else 2)
    exp = {"q7": int(an.stats.q7_violations), "G": G}
    if place.startswith("pred"):
        f = int(an.start[first_item_at(an, G)])
        if value == "v11":       # the slice's one violation is the first delta after the boundary
            if an.bad.tolist() != [f]:
                return None
        elif int(an.d[f]) != 5 - 65535:
            return None
    elif value == "v11" and an.stats.q7_violations != 1:
        return None
    if place == "before" and value == "v11" and an.bad.tolist() != [int(an.start[first_item_at(an, G)])]:
        return None
    # who sees the pixel, by the flags of the streaming kernel: in the predecessor cases the group that ends at G and not the
    # one that starts there; `before` and `inside`: the group that starts at G (through `before` alone / among its own blocks);
    # `lookahead`: that group and, through its look-ahead, the one that ends at G
    reg = _regime_sets(img)
    col = 1 if value == "v11" else 0
    for tpg, r in reg.items():
        if G % (256 * tpg):
            continue
        g = G // (256 * tpg)
        if place.startswith("pred"):
            assert not r[g][col] and r[g - 1][col]
        elif place in ("lookahead", "before", "inside"):
            assert r[g][col]
            assert r[g - 1][col] == (place != "inside")      # (`before` sits in the last block of the group that ends at G)
        exp.setdefault("boundary_of_tpg", []).append(tpg)
    return exp


def resolve_one(spec):
    NB = spec["shape"][0] * spec["shape"][1] // spec["bs"]
    Gs = _one_classes(NB)[spec["boundary"]] if "boundary" in spec else [NB // 2]
    for seed in range(1, 400):
        for G in Gs:
            made = _one_make(spec, seed, G)
            if made is not None and _one_expect(spec, made[0], made[1], made[2], G) is not None:
                return dict(spec, seed=seed, G=G)
    raise AssertionError(f"no seed found for {spec['name']}")


def build_one(spec):
    """11-bit noise of seed spec['seed'] with one pixel >= 0x0800 (4095, after a 2047) or >= 0x4000 (65535), placed relative to the
    group boundary at block spec['G']: inside the group that starts there, in its first 64 blocks (the look-ahead of the group
    before), on the last traversal pixel before it (`before`), or -- pred_pair, pred_lone -- on the pixel that precedes the
    boundary in the FINAL order while block G-1 is the partner of an earlier leader, so that no regime flag of the group sees it;
    the first item after the boundary is then a meshed pair or a lone block.  With 4095 the slice has exactly one Q7 violation,
    the first delta after the boundary; with 65535 that delta is 5 - 65535, whose low 16 bits read +6."""
    made = _one_make(spec, spec["seed"], spec["G"])
    assert made is not None, spec["name"]
    img, an, tpos = made
    exp = _one_expect(spec, img, an, tpos, spec["G"])
    assert exp is not None, spec["name"]
    if "boundary" in spec:
        want = {"tpg1": [1], "tpg2": [1, 2], "tpg4": [1, 2, 4]}[spec["boundary"]]
        assert exp["boundary_of_tpg"] == want
    return spec["name"], img, exp


# ---------------------------------------------------------------------------------------------------- fit
def fit_margins(an):
    """For every difficult block A and candidate B = A + j (j = 1..63): up = #(B[t] - A[t] >= 65) + #(A[t+1] - B[t] >= 65) and
    cur = the large deltas of A with the entering one; B fits if up + 1 < cur - 2.  Returns the margins (up + 1) - (cur - 2) and
    the two difference arrays of the tested candidates."""
    bs, NB = an.bs, an.NB
    px = an.trav.astype(np.int64).reshape(NB, bs)
    cur = an.large.sum(axis=1)
    diff_blocks = np.flatnonzero(an.difficult)
    diff_blocks = diff_blocks[diff_blocks > 0]
    margins, d1s, d2s = [], [], []
    for j in range(1, 64):
        A = diff_blocks[diff_blocks + j < NB]
        d1 = px[A + j] - px[A]
        d2 = px[A][:, 1:] - px[A + j][:, :-1]
        up = (d1 >= 65).sum(axis=1) + (d2 >= 65).sum(axis=1)
        margins.append(up + 1 - (cur[A] - 2))
        d1s.append(d1.reshape(-1))
        d2s.append(d2.reshape(-1))
    return np.concatenate(margins), np.concatenate(d1s), np.concatenate(d2s)


def build_fit(spec):
    """Noise over five levels that lie 64 or 65 apart below spec['top'], in blocks that repeat the previous pixel with
    probability 0, 0.3 or 0.5: candidate partners whose differences B[t] - A[t] and A[t+1] - B[t] are exactly 64 and 65 and whose
    count sits on, one below and one above the fit threshold.  top 0x3FFF: every pixel < 0x4000 but A + 65 crosses it."""
    shape, bs = _shape(spec), spec["bs"]
    rng = np.random.default_rng([spec["seed"], shape[0], shape[1], bs])
    NB = shape[0] * shape[1] // bs
    levels = spec["top"] - np.array([0, 64, 129, 193, 258])
    pick = levels[rng.integers(0, 5, (NB, bs))].reshape(-1)
    hold = (rng.random((NB, bs)) < np.array([0.0, 0.3, 0.5])[rng.integers(0, 3, NB)][:, None]).reshape(-1)
    hold[0] = False
    src = np.maximum.accumulate(np.where(hold, 0, np.arange(pick.size)))
    img = along(shape, np.uint16, pick[src])
    an = analyse(img, bs)
    margins, d1, d2 = fit_margins(an)
    for m in (-1, 0, 1):
        assert (margins == m).sum() > 0, m
    for dd in (d1, d2):
        assert (dd == 64).sum() > 0 and (dd == 65).sum() > 0
    lone_difficult = int((an.difficult & (an.role == 0)).sum())
    assert an.stats.n_jump >= NB // 64 and lone_difficult >= NB // 64      # both outcomes of the partner search
    q7 = int(an.trav[0] > 2048)                                # the first delta, from the implicit 0, is the only one that can be large
    assert an.bad.tolist() == ([0] if q7 else [])
    top = spec["top"]
    regime = {1000 + 258: (False, False), 0x0800 + 129: (False, True), 0x3FFF: (False, True), 0x4000 + 129: (True, True)}[top]
    for tpg, reg in _regime_sets(img).items():
        assert set(reg) == {regime}
    if top == 0x0800 + 129:
        assert img.min() < 0x0800 <= img.max()
    if top == 0x3FFF:
        assert img.max() == 0x3FFF
    elif top > 0x4000:
        assert img.min() < 0x4000 <= img.max()
    return spec["name"], img, {"q7": q7, "n_jump": int(an.stats.n_jump), "lone_difficult": lone_difficult}


# ---------------------------------------------------------------------------------------------------- full
def build_full(spec):
    shape, bs, what = _shape(spec), spec["bs"], spec["what"]
    rng = np.random.default_rng([spec["seed"], shape[0], shape[1]])
    N = shape[0] * shape[1]
    if what == "u16_noise":
        img = rng.integers(0, 65536, shape).astype(np.uint16)
        img.reshape(-1)[:2] = (0, 65535)
    elif what == "checker":                                     # the traversal moves to a 4-neighbour: every delta is +-65535
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        img = np.where((yy + xx) % 2 == 0, 0, 65535).astype(np.uint16)
    elif what == "all_max":                                     # the first delta, from the implicit 0, is 65535
        img = np.full(shape, 65535, dtype=np.uint16)
    elif what == "i16_noise":
        img = rng.integers(-32768, 32768, shape).astype(np.int16)
        img.reshape(-1)[:2] = (-32768, 32767)
    elif what == "i16_zero":                                    # around zero: the unsigned bytes jump between 0 and 65535
        img = rng.integers(-300, 300, shape).astype(np.int16)
    elif what == "i16_steps":                                   # runs at -32768 and 32767 along the traversal, a few values between
        runs = rng.integers(1, 40, N)
        seq = np.repeat(np.where(np.arange(N) % 2 == 0, -32768, 32767), runs)[:N]
        seq = np.where(rng.random(N) < 0.02, rng.integers(-32768, 32768, N), seq)
        img = along(shape, np.int16, seq)
    else:
        raise KeyError(what)
    an = analyse(img, bs)
    lo, hi = int(img.min()), int(img.max())
    if what != "i16_zero":
        assert hi == (65535 if img.dtype == np.uint16 else 32767)
    if what in ("u16_noise", "checker"):
        assert lo == 0
    if what in ("i16_noise", "i16_steps"):
        assert lo == -32768
    if what == "i16_zero":
        assert lo < 0 < hi
    if what == "checker":
        assert set(np.unique(np.abs(np.diff(an.trav.astype(np.int64))))) <= {0, 65535} and set(np.unique(np.abs(an.d))) == {0, 65535}
    if what == "all_max":
        assert an.d[0] == 65535 and not an.d[1:].any()
    assert an.stats.q7_violations > 0
    return spec["name"], img, {"q7": int(an.stats.q7_violations)}


# ---------------------------------------------------------------------------------------------------- the cases
E2E = ("tok_256", "q7_128_packed_pair_2049", "q7_256_wide_lone_after_meshed_p0_m2048", "one_256_v14_pred_pair_tpg4", "fit_256_top3fff",
       "full_256_u16_noise", "full_256_i16_steps", "full_128_i16_zero", "tok_60x64_bs12", "full_60x64_bs5_i16_steps")


def _shape_tag(shape):
    return str(shape[0]) if shape[0] == shape[1] else f"{shape[0]}x{shape[1]}"


def specs():
    """Every case, unresolved.  Block size 16 everywhere; the other block sizes on a small subset of every family, on the one
    shape they all divide."""
    out = []

    def add(family, name, shape, bs=16, **kw):
        out.append(dict(family=family, name=name, shape=list(shape), bs=bs, **kw))

    generic = ((64, 64), ALL_BS_SHAPE, (80, 48))
    # tok
    five = [1000, 0x0800, 0x4000, 0x8000, 65535 - 400]
    for n in (128, 256, 512):
        add("tok", f"tok_{n}", (n, n), seed=1, plateaus=five)
    for shp, two in zip(generic, ([1000, 0x4000], [0x0800, 0x8000], [0x4000, 65535 - 400])):
        add("tok", f"tok_{_shape_tag(shp)}", shp, seed=2, plateaus=two)
    for bs, some in zip(OTHER_BS, ([0x0800, 0x4000], [0x4000, 0x8000], [0x4000], [0x0800], [1000, 65535 - 400], [0x8000, 0x4000])):
        add("tok", f"tok_{_shape_tag(ALL_BS_SHAPE)}_bs{bs}", ALL_BS_SHAPE, bs, seed=3, plateaus=some)
    # q7
    places = ("lone_p0", "lone_pk", "pair", "lone_after_meshed_p0")

    def q7(shape, bs, regime, place, delta, seed=1):
        tag = f"q7_{_shape_tag(shape)}" + (f"_bs{bs}" if bs != 16 else "") + f"_{regime}_{place}_{delta}".replace("-", "m")
        add("q7", tag, shape, bs, regime=regime, place=place, delta=delta, seed=seed, search=True)

    for regime in ("packed", "wide"):
        for place in places:
            for delta in Q7_DELTAS:
                q7((128, 128), 16, regime, place, delta)
            for delta in (-2048, 2049):
                q7((256, 256), 16, regime, place, delta)
    for regime, place, delta in (("packed", "pair", 2049), ("packed", "lone_p0", -2049), ("wide", "pair", -2049), ("wide", "lone_after_meshed_p0", -2048)):
        q7((512, 512), 16, regime, place, delta)
    for shp in generic:
        q7(shp, 16, "packed", "pair", 2049)
        q7(shp, 16, "wide", "lone_after_meshed_p0", -2048)
    for bs in OTHER_BS:
        q7(ALL_BS_SHAPE, bs, "packed", "pair", 2049)
        q7(ALL_BS_SHAPE, bs, "wide", "lone_after_meshed_p0", -2048)
    # one
    for n in (256, 512):
        for value in ("v11", "v14"):
            for boundary in ("tpg1", "tpg2", "tpg4"):
                for place in ("pred_pair", "pred_lone"):
                    add("one", f"one_{n}_{value}_{place}_{boundary}", (n, n), value=value, place=place, boundary=boundary, search=True)
            for place, boundary in (("inside", "tpg4"), ("lookahead", "tpg2" if n == 256 else "tpg4"), ("before", "tpg1" if n == 256 else "tpg4")):
                add("one", f"one_{n}_{value}_{place}_{boundary}", (n, n), value=value, place=place, boundary=boundary, search=True)
    for value in ("v11", "v14"):
        add("one", f"one_64_{value}_inside", (64, 64), value=value, place="inside", search=True)
        for bs in OTHER_BS:
            add("one", f"one_{_shape_tag(ALL_BS_SHAPE)}_bs{bs}_{value}_inside", ALL_BS_SHAPE, bs, value=value, place="inside", search=True)
    # fit
    for n in (128, 256):
        for top in (1000 + 258, 0x0800 + 129, 0x3FFF, 0x4000 + 129):
            add("fit", f"fit_{n}_top{top:04x}", (n, n), top=top, seed=1)
    add("fit", "fit_512_top3fff", (512, 512), top=0x3FFF, seed=1)
    for shp in generic:
        add("fit", f"fit_{_shape_tag(shp)}_top3fff", shp, top=0x3FFF, seed=2)
    for bs in (8, 32, 64, 12):     # (at block sizes 4 and 5 a partner fits block 0 only: up + 1 < cur - 2 needs cur >= 4)
        add("fit", f"fit_{_shape_tag(ALL_BS_SHAPE)}_bs{bs}_top4081", ALL_BS_SHAPE, bs, top=0x4000 + 129, seed=3)
    # full
    kinds = ("u16_noise", "checker", "all_max", "i16_noise", "i16_zero", "i16_steps")
    for n in (128, 256, 512):
        for what in kinds:
            add("full", f"full_{n}_{what}", (n, n), what=what, seed=1)
    add("full", "full_1024_u16_noise", (1024, 1024), what="u16_noise", seed=1, no_reference=True)
    for what in kinds:
        add("full", f"full_{_shape_tag(ALL_BS_SHAPE)}_{what}", ALL_BS_SHAPE, what=what, seed=2)
    add("full", "full_64_u16_noise", (64, 64), what="u16_noise", seed=2)
    add("full", "full_80x48_i16_noise", (80, 48), what="i16_noise", seed=2)
    for bs in OTHER_BS:
        for what in ("u16_noise", "i16_steps"):
            add("full", f"full_{_shape_tag(ALL_BS_SHAPE)}_bs{bs}_{what}", ALL_BS_SHAPE, bs, what=what, seed=3)
    assert len({s["name"] for s in out}) == len(out)
    for s in out:                                             # one case per family (and both dtypes) also goes end to end with DEFLATE
        if s["name"] in E2E:
            s["e2e"] = True
    assert sum(1 for s in out if s.get("e2e")) == len(E2E)
    return out


RESOLVERS = {"q7": resolve_q7, "one": resolve_one}
BUILDERS = {"tok": build_tok, "q7": build_q7, "one": build_one, "fit": build_fit, "full": build_full}


def resolve(spec):
    """the spec with what its seeded search found (position, seed, boundary block); a spec that needs no search as it is"""
    if not spec.get("search"):
        return dict(spec)
    r = RESOLVERS[spec["family"]](spec)
    del r["search"]
    return r


def build(spec):
    """(name, image, expectations) of a resolved spec; asserts the case's precondition"""
    assert "search" not in spec, "resolve the spec first (oracle/gen_value_edges_golden.py does, and stores it)"
    return BUILDERS[spec["family"]](spec)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN_JSON) as f:
        return json.load(f)


def cases():
    """name -> record of tests/golden/value_edges.json: the resolved spec and what the reference made of the image"""
    return {c["spec"]["name"]: c for c in golden()["cases"]}


@functools.lru_cache(maxsize=None)
def built(name):
    """(image, expectations) of a stored case; the builder's precondition is asserted on the way"""
    _, img, exp = build(cases()[name]["spec"])
    img.setflags(write=False)
    return img, exp


def is_tile_shape(spec):
    s = spec["shape"]
    return spec["bs"] == 16 and s[0] == s[1] and s[0] in TILE_SIDES
