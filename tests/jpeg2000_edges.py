"""Undamaged JPEG 2000 inputs with one case planted on each rule edge of the encoder (csrc/jpeg2000_kernels.hip) and of the decoder
(csrc/jpeg2000_decode_kernels.hip), for what jpeg2000_model.matrix() and phantoms() do not reach.  No device is needed here:
tests/test_jpeg2000_edges_host.py proves with the models' traces that every case reaches what it plants, tests/test_gpu_jpeg2000_edges.py
holds the kernels to the files, and tools/debug/j2k_host_emu and j2k_dec_host_emu run the set under the sanitizers.

    cases() -> [Case(name, group, raster, kw for jpeg2000_model.encode, planted)], planted = ((trace key, item), ...)
    files() -> {name: jpeg2000_model.encode(raster, **kw)}, traces() -> {name: the encoder model's trace}, each computed once;
    files(traced=True) -> the files of the run that made traces()
    batches() -> the cases by (shape, dtype, kw): what one jpeg2000_encode_batch call can hold (every depth of "levels" has three frames)
    decode_batches() -> the cases by shape: what one jpeg2000_decode_batch call can hold
    adversary(w, h) -> the block that always offers the MQ coder its less probable symbol

Groups: "levels" (2, 3, 4, 6, 7, 8 decompositions on shapes whose lengths shrink to 2 and 1), "precision" (2, 3, 7, 9, 15 bits and
the two largest shifts), "tagtree" (trees of up to 5 levels with included and excluded leaves), "tier1" (neighbour patterns, sign
keys, candidate rows, run-length mode, one and the most bit-planes), "mq_t2" (segment lengths at 2^k - 1 and 2^k), "adversary".

Coefficients are planted exactly: at levels=0 a sample minus 2^(precision-1) is the LL coefficient; for the other bands a whole
Mallat plane is planted and from_plane() inverts it, asserting the raster's range and that dwt_53 returns the plane.

Every raster has at most 16 384 samples, with one exception: a tag tree that is odd at every level on both axes needs 9 x 9 leaves
(9, 5, 3, 2, 1), which at code-blocks of 32 is 257 x 257 samples and nothing smaller; its blocks hold one sample each, so it stays cheap.

The most bit-planes.  A coefficient is at most the L1 norm of its analysis filter times 2^(precision-1), plus rounding.  For the
5/3 high-pass filter of decomposition d, followed through the low-pass filters of the levels before it, the norm is 2, 2.5, 2.75,
2.80, 2.83, 2.85, 2.86 for d = 1 .. 7 (worst_gain()), so HH reaches 4, 6.25, 7.56, 7.87, 7.99, 8.11, 8.19 times 2^15 at 16 bits.  The
search over 0 / 65535 rasters at 1 to 3 levels (search_most_planes()) therefore cannot pass 18 planes, and that is what it finds
(7.56 < 8); but from 6 levels on the product passes 8 = 2^18 / 2^15, and 19 planes are reachable: worst_raster(97, 6) is the
sign pattern of the filter of the second HH coefficient of level 6 on a 97 x 97 raster (97 is the smallest length at which that
norm squared passes 8), and its HH coefficient of resolution 1 has 19 bits: 55 coding passes, 0 zero bit-planes, the whole Tier-1
word.  20 planes would need a norm of 16 and are excluded: the norms converge below 2.9.  HL / LH (Mb 18) need 8 for a 19th plane
and stay below 2.86 * 1.72 = 4.9; LL (Mb 17) needs 4 and stays below 1.72^2 = 2.96.  So no 16-bit raster overflows its Mb; at 2 or 3 bits
the rounding of the lifting steps is not small against the range, and this argument does not cover them.

Run-length mode "broken off for one reason in one row".  A significant sample makes the rows above and below it in its column
candidates of the propagation pass, so they are visited or significant by the cleanup: a column whose only flag is one significant
row does not exist.  What is planted and counted instead (trace key "rl_off", masks of the four rows): exactly one significant row,
each of the four; no significant row and exactly one visited row, which can only be row 0 or row 3 (the one significant neighbour
then lies in the stripe above or below; a neighbour that touches row 1 or 2 touches a second row); and neither, with the rows that
one significant neighbour sample touches: 0001 (stripe above), 0011, 0111, 1110, 1100 (previous column, found by the cleanup pass
itself), 1000 (stripe below, found by the propagation pass after this stripe was passed).  UNREACHABLE_RL_OFF names the rest.

Neighbour patterns: all 256 are reached in every orientation; pattern 0 only in the cleanup pass, because the propagation pass
skips a sample without significant neighbours.  All 81 sign keys are reached with both signs.  Nothing is argued unreachable there.

The slab rule.  adversary(64, 64) and adversary(32, 32) at 15 bit-planes give segments of 8197 and 2053 bytes, 0.420 and 0.417 (ADVERSARY_RATIO) of
j2k_slab_cap(w, h, mb) = (w * h * (mb + 2) + 3) // 4 + 64 (csrc/cct_internal.h); noise reaches about 0.44.
"""
import collections
import functools
import itertools

import numpy as np

import jpeg2000_decode_model as d
import jpeg2000_model as m
from jpeg2000_model import HH, HL, LH, LL

Case = collections.namedtuple("Case", "name group raster kw planted")
ORIENTS = (LL, HL, LH, HH)
ORIENT_NAMES = {LL: "LL", HL: "HL", LH: "LH", HH: "HH"}
MAX_SAMPLES = 16384
MOST_PLANES = 19
ADVERSARY_RATIO = {64: 0.420, 32: 0.417}  # measured: see test_jpeg2000_edges_host.test_adversary
SEGMENT_LENGTHS = tuple(sorted({(1 << k) - e for k in range(1, 14) for e in (0, 1)}))
# (w, h, bits, seed, n, last) per segment length: an LL block of w x h at levels 0 whose first n coefficients in raster order are
# rng(seed).integers(-2^bits + 1, 2^bits), the n-th replaced by `last`, the rest 0.  Found by bisection on n and a scan of `last`.
SEGMENT_BLOCKS = {
    1: (1, 1, 1, 0, 1, 1), 2: (4, 4, 2, 0, 1, 1), 3: (4, 4, 2, 0, 2, 3), 4: (5, 5, 2, 0, 3, -3), 7: (6, 6, 2, 0, 8, 3), 8: (6, 6, 2, 0, 11, 1),
    15: (6, 6, 5, 0, 12, -2), 16: (6, 6, 5, 0, 13, -31), 31: (8, 8, 5, 0, 28, 18), 32: (8, 8, 5, 0, 30, 10), 63: (10, 10, 5, 0, 72, 16),
    64: (11, 11, 5, 0, 72, 1), 127: (14, 14, 5, 0, 148, 16), 128: (14, 14, 5, 0, 150, 4), 255: (20, 20, 5, 0, 309, 16), 256: (20, 20, 5, 0, 311, 6),
    511: (28, 28, 5, 0, 638, 18), 512: (28, 28, 5, 0, 640, 20), 1023: (30, 30, 10, 0, 703, 5), 1024: (30, 30, 10, 0, 703, 39),
    2047: (43, 43, 10, 0, 1409, 12), 2048: (43, 43, 10, 0, 1411, 12), 4095: (60, 60, 10, 0, 2825, 8), 4096: (60, 60, 10, 0, 2825, 1),
    8191: (64, 64, 15, 0, 3901, 32), 8192: (64, 64, 15, 0, 3902, 2),
}
RL_OFF_NEIGHBOUR_MASKS = (0b0001, 0b0011, 0b0111, 0b1110, 0b1100, 0b1000)
# (significant, visited) masks of a full column without run-length mode that the argument above excludes
UNREACHABLE_RL_OFF = tuple((1 << k, 0) for k in range(4)) + ((0, 0b0010), (0, 0b0100))
# and with neither a significant nor a visited row, the masks of rows with a significant neighbour that no set of neighbours gives: one
# in the stripe above touches row 0, one in rows 0 .. 3 of the next columns rows 01, 012, 123, 23, one in the stripe below row 3, and the
# unions of these are 0001 0011 0111 1000 1001 1011 1100 1101 1110 1111
UNREACHABLE_NEIGHBOUR_MASKS = (0b0010, 0b0100, 0b0101, 0b0110, 0b1010)


# ---- placing exact coefficients --------------------------------------------------------------------------------------------

def dtype_of(precision):
    return np.uint8 if precision <= 8 else np.uint16


def from_plane(plane, levels, precision):
    """The raster whose `levels`-level transform is the Mallat plane."""
    plane = np.asarray(plane, np.int64)
    x = d.idwt_53(plane, levels) + (1 << (precision - 1))
    assert x.min() >= 0 and x.max() <= (1 << precision) - 1, (int(x.min()), int(x.max()))
    assert np.array_equal(m.dwt_53(x - (1 << (precision - 1)), levels), plane)
    return x.astype(dtype_of(precision))


def band_plane(orient, band):
    """The one-level Mallat plane that holds `band` as its `orient` subband and zeros elsewhere; LL: the band itself at no level."""
    h, w = band.shape
    if orient == LL:
        return band, 0
    plane = np.zeros((2 * h, 2 * w), np.int64)
    y0, x0 = (h if orient in (LH, HH) else 0), (w if orient in (HL, HH) else 0)
    plane[y0:y0 + h, x0:x0 + w] = band
    return plane, 1


def band_case(name, group, orient, band, codeblock, planted, precision=16):
    plane, levels = band_plane(orient, np.asarray(band, np.int64))
    return Case(f"{name}_{ORIENT_NAMES[orient]}_cb{codeblock}", group, from_plane(plane, levels, precision),
                dict(precision=precision, levels=levels, codeblock=codeblock), tuple(planted))


# ---- group "levels" ----------------------------------------------------------------------------------------------------------

LEVEL_SHAPES = ((1, 1), (2, 2), (3, 300), (300, 3), (257, 2), (33, 65))
DEEP_LEVELS = (2, 3, 4, 6, 7, 8)


def level_cases():
    """Per (shape, levels) one encoder batch of three frames (noise, ramp, checker) of one precision and code-block size, both of which
    rotate with the shape and the depth; at 8 levels three batches: both code-block sizes as codestreams and one as JP2."""
    out = []
    for si, (rows, cols) in enumerate(LEVEL_SHAPES):
        for levels in DEEP_LEVELS:
            cb0 = (64, 32)[(si + levels) % 2]
            for k, (cb, jp2) in enumerate(((cb0, False), (96 - cb0, False), (cb0, True)) if levels == 8 else ((cb0, False),)):
                precision = (16, 12, 8)[(si + levels + k) % 3]
                kw = dict(precision=precision, levels=levels, codeblock=cb, jp2=jp2)
                for content in ("noise", "ramp", "checker"):
                    img = m.raster_cases(rows, cols, precision, dtype_of(precision), seed=levels)[content]
                    out.append(Case(f"levels_{rows}x{cols}_{levels}_{content}_p{precision}_cb{cb}{'_jp2' if jp2 else ''}", "levels", img, kw, (("levels", levels),)))
    return out


# ---- group "precision" -------------------------------------------------------------------------------------------------------

ODD_PRECISIONS = (2, 3, 7, 9, 15)


def precision_cases():
    out = []
    for precision in ODD_PRECISIONS:
        for rows, cols, cb in ((5, 3, 64), (33, 65, 32)):
            for levels in (0, 2, 5):
                for content, img in m.raster_cases(rows, cols, precision, dtype_of(precision), seed=precision).items():
                    out.append(Case(f"precision_{precision}_{rows}x{cols}_{levels}_{content}", "precision", img,
                                    dict(precision=precision, levels=levels, codeblock=cb), (("precision", precision),)))
    rng = np.random.default_rng(5)
    for precision in (2, 8, 9, 16):
        for shift in (precision - 1, precision - 2):  # the stored samples have 1 and 2 bits
            img = rng.integers(0, 1 << (precision - shift), (33, 65)).astype(dtype_of(precision))
            out.append(Case(f"precision_{precision}_shift_{shift}", "precision", img, dict(precision=precision, shift=shift, levels=2, codeblock=32),
                            (("precision", precision),)))
    return out


# ---- group "tagtree" ---------------------------------------------------------------------------------------------------------

def leaf_raster(rows, cols, planes, levels=0, cb=32):
    """16 bits, levels 0 (or one level of a one-row raster: LL and HL side by side): block k of the grid of `cb` holds one sample of
    planes[k] bit-planes (0: every coefficient 0, the block is not included) at a position that moves with k."""
    plane = np.zeros((rows, cols), np.int64)
    bands = [(0, cols)] if levels == 0 else [(0, (cols + 1) // 2), ((cols + 1) // 2, cols)]
    k = 0
    for x0, x1 in bands:
        for by in range(0, rows, cb):
            for bx in range(x0, x1, cb):
                if planes[k]:
                    y, x = by + (5 * k) % min(cb, rows - by), bx + (11 * k) % min(cb, x1 - bx)
                    plane[y, x] = (1 << (planes[k] - 1)) * (-1 if k & 1 or planes[k] == 16 else 1)  # +2^15 is no 16-bit sample
                k += 1
    assert k == len(planes)
    return from_plane(plane, levels, 16)


def tree_patterns(ncw, nch):
    """{name: bit-planes per leaf in raster order, 0 = excluded}"""
    n = ncw * nch
    up = [1 + (k * 14) // max(1, n - 1) for k in range(n)]  # the zero bit-planes fall along the scan: every level's minimum differs
    quad = [0 if ((k % ncw) // 2 + (k // ncw) // 2) % 2 == 0 else up[k] for k in range(n)]  # whole parent quads excluded
    return {
        "only_last": [0] * (n - 1) + [3], "only_first": [5] + [0] * (n - 1), "alternating": [up[k] if k % 2 else 0 for k in range(n)],
        "one_excluded": [0 if k == n // 2 else up[k] for k in range(n)], "quads_excluded": quad, "zbp_falling": up, "zbp_rising": up[::-1],
    }


TREE_SHAPES = ((3, 300, 0), (300, 3, 0), (1, 600, 1), (97, 161, 0), (257, 257, 0))


def tree_depth(n):
    k = 1
    while n > 1:
        n, k = (n + 1) // 2, k + 1
    return k


def tagtree_cases():
    out = []
    for rows, cols, levels in TREE_SHAPES:
        bw = cols if levels == 0 else (cols + 1) // 2
        ncw, nch = -(-bw // 32), -(-rows // 32)
        depth = max(tree_depth(ncw), tree_depth(nch))
        for name, planes in tree_patterns(ncw, nch).items():
            planted = [("tt_levels", (ncw, nch, depth))]
            if name in ("zbp_falling", "zbp_rising", "one_excluded"):
                planted += [("tt_learnt", ("zbp", lv)) for lv in range(depth)]
            if name in ("alternating", "quads_excluded", "only_last"):
                planted += [("tt_learnt", ("incl", lv)) for lv in range(depth)]
            out.append(Case(f"tagtree_{rows}x{cols}_{name}", "tagtree", leaf_raster(rows, cols, planes * (levels + 1), levels),
                            dict(precision=16, levels=levels, codeblock=32), tuple(planted)))
    return out


# ---- group "tier1" -----------------------------------------------------------------------------------------------------------

def cell_centres(bh, bw, cb):
    """Centres of 3 x 3 cells, three apart, each whole inside one code-block of a bh x bw band."""
    out = []
    for by in range(0, bh, cb):
        for bx in range(0, bw, cb):
            hh, ww = min(cb, bh - by), min(cb, bw - bx)
            out += [(by + 1 + 3 * i, bx + 1 + 3 * j) for i in range(hh // 3) for j in range(ww // 3)]
    return out


def pattern_band(cb, centre):
    """64 x 64: cell k has the neighbours of pattern k at magnitude 2 (significant from plane 1 on) around a centre of magnitude
    `centre` (0 or 1), which plane 0 codes with exactly that pattern: patterns 1 .. 255 in the propagation pass, 0 in the cleanup."""
    band = np.zeros((64, 64), np.int64)
    cells = cell_centres(64, 64, cb)
    assert len(cells) >= 256
    for pat, (y, x) in zip(range(256), cells):
        for k, (dy, dx) in enumerate(m.NEIGHBOURS):
            if (pat >> k) & 1:
                band[y + dy, x + dx] = -2 if (pat * 7 + k) % 3 == 0 else 2
        band[y, x] = -centre if pat & 1 else centre
    return band


SIGN_KEYS = tuple(itertools.product((0, 1, -1), repeat=4))  # contributions of W, E, N, S


def sign_band(cb):
    """64 x 64: cell k has W, E, N, S of magnitude 2 with the signs of key k // 2 and a centre of magnitude 1, negative for odd k."""
    band = np.zeros((64, 64), np.int64)
    cells = cell_centres(64, 64, cb)
    assert len(cells) >= 162
    for k, (y, x) in zip(range(162), cells):
        w, e, n, s = SIGN_KEYS[k // 2]
        band[y, x - 1], band[y, x + 1], band[y - 1, x], band[y + 1, x] = 2 * w, 2 * e, 2 * n, 2 * s
        band[y, x] = -1 if k & 1 else 1
    return band


def sparse_band(h, w, density, bits, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(-(1 << bits) + 1, 1 << bits, (h, w))
    return np.where(rng.random((h, w)) < density, v, 0)


def run_band():
    """24 x 40, three planes.  Stripe 0: a lone sample of magnitude 4 in row r of column 3 + 6 r ends the top plane's run at r, and the
    column behind it has the neighbour rows 0011 / 0111 / 1110 / 1100; the columns between have runs of four zeros.  Row 3 of stripe 1
    under empty columns gives 0001 in stripe 2.  In stripe 3, S = 2 above T = 4 (rows 0 and 1 of stripe 4) becomes significant in the
    propagation pass of plane 1 after stripe 3 was passed: 1000 there.  Stripe 5: single significant rows with quiet surroundings."""
    b = np.zeros((24, 40), np.int64)
    for r in range(4):
        b[r, 3 + 6 * r] = 4 if r & 1 else -4
    b[7, 30] = 4
    b[17, 10], b[16, 10] = 4, 2
    b[20, 5], b[21, 15], b[22, 25], b[23, 35] = 4, -4, 5, -6
    return b


def _lift_linear(x):
    """jpeg2000_model._lift_53 without its rounding"""
    n = x.shape[0]
    if n == 1:
        return x.copy(), x[:0].copy()

    def at(i):
        i = np.abs(i)
        return x[np.where(i >= n, 2 * (n - 1) - i, i)]
    k = np.arange(-1, (n + 1) // 2)
    hi = at(2 * k + 1) - (at(2 * k) + at(2 * k + 2)) / 2
    return x[0::2] + (hi[:-1] + hi[1:]) / 4, hi[1:1 + n // 2]


def linear_analysis(n, levels):
    """The matrix of the 5/3 analysis without its rounding on a length-n signal, rows in Mallat order, and the low-pass lengths."""
    a, h, dims = np.eye(n), n, [n]
    for _ in range(levels):
        lo, hi = _lift_linear(a[:h])
        a[:h] = np.concatenate([lo, hi])
        h = (h + 1) // 2
        dims.append(h)
    return a, dims


def worst_gain(n, levels):
    """(L1 norm, row) of the high-pass coefficient of decomposition `levels` with the largest norm on a length-n signal."""
    a, dims = linear_analysis(n, levels)
    hi = a[dims[levels]:dims[levels - 1]]
    norms = np.abs(hi).sum(axis=1)
    return float(norms.max()), hi[int(norms.argmax())]


def worst_raster(n, levels):
    """n x n of 0 / 65535: the sign pattern of the HH coefficient of decomposition `levels` with the largest gain."""
    _, row = worst_gain(n, levels)
    return np.where(np.outer(row, row) > 0, 65535, 0).astype(np.uint16)


def planes_of(raster, precision, levels):
    """the most bit-planes of a subband per orientation"""
    rows, cols = raster.shape
    plane = m.dwt_53(raster.astype(np.int64) - (1 << (precision - 1)), levels)
    out = {}
    for bands in m.resolutions(rows, cols, levels):
        for orient, x0, y0, w, h in bands:
            if w and h:
                out[orient] = max(out.get(orient, 0), int(np.abs(plane[y0:y0 + h, x0:x0 + w]).max()).bit_length())
    return out


def search_most_planes(levels=(1, 2, 3), sizes=(8, 16, 24)):
    """The search over 0 / 65535 rasters at 1 to 3 levels: the sign patterns of every HH filter on small squares, both polarities."""
    best = 0
    for n in sizes:
        for lv in levels:
            a, dims = linear_analysis(n, lv)
            hi = a[dims[lv]:dims[lv - 1]]
            for r in hi:
                for c in hi:
                    for s in (1, -1):
                        best = max(best, planes_of(np.where(s * np.outer(r, c) > 0, 65535, 0), 16, lv)[HH])
    return best


TIER1_BLOCKS = ((1, 9, 64), (9, 1, 64), (5, 30, 32), (6, 30, 32), (7, 30, 32), (33, 65, 32), (65, 33, 64))  # (h, w, codeblock) of the band


def tier1_cases():
    out = []
    for orient in ORIENTS:
        for cb in (64, 32):
            for centre in (0, 1):
                planted = [("zc", (orient, pat, "sp")) for pat in range(1, 256)] + [("zc", (orient, 0, "cu"))]
                planted += [("zc_ctx", (orient, cx, centre)) for cx in range(9)]
                out.append(band_case(f"tier1_patterns_centre{centre}", "tier1", orient, pattern_band(cb, centre), cb, planted))
            out.append(band_case("tier1_signs", "tier1", orient, sign_band(cb), cb, [("sign", (SIGN_KEYS[k // 2], k & 1)) for k in range(162)]))
        planted = [("rl", r) for r in range(5)] + [("rl_off", (orient, 0, 0, mask)) for mask in RL_OFF_NEIGHBOUR_MASKS]
        out.append(band_case("tier1_runs", "tier1", orient, run_band(), 64, planted))
        for h, w, cb in TIER1_BLOCKS:
            for k, (density, bits) in enumerate(((0.04, 3), (0.3, 6), (0.12, 4))):
                band = sparse_band(h, w, density, bits, 100 * orient + k)
                band[h - 1, w - 1] = -3  # becomes significant in the last column and the last row: its neighbours are the border words
                planted = [("block", (min(w, cb), min(h, cb), orient)), ("edge_sig", "col"), ("edge_sig", "row")] if k == 1 else []
                out.append(band_case(f"tier1_sparse_{h}x{w}_{k}", "tier1", orient, band, cb, planted))
        for cb in (64, 32):
            for k, (density, bits) in enumerate(((0.02, 2), (0.12, 4), (0.5, 9))):
                out.append(band_case(f"tier1_sparse_{cb}_{k}", "tier1", orient, sparse_band(cb, cb, density, bits, 7 * orient + k), cb,
                                     [("block", (cb, cb, orient))]))
        one = np.sign(sparse_band(12, 10, 0.3, 3, 50 + orient))
        one[0, 0] = 1
        out.append(band_case("tier1_one_plane", "tier1", orient, one, 32, [("nplanes", 1), ("passes", 1)]))
    out.append(Case("tier1_17_planes_8x8", "tier1", worst_raster(8, 1), dict(precision=16, levels=1, codeblock=32), (("nplanes", 17), ("zbp", 2))))
    out.append(Case("tier1_18_planes_16x16", "tier1", worst_raster(16, 2), dict(precision=16, levels=2, codeblock=32), (("nplanes", 18), ("zbp", 1))))
    worst = worst_raster(97, 6)
    out.append(Case("tier1_19_planes_97x97", "tier1", worst, dict(precision=16, levels=6, codeblock=64),
                    (("nplanes", MOST_PLANES), ("passes", 3 * MOST_PLANES - 2), ("zbp", 0))))
    for name, img in (("inverse", 65535 - worst), ("transposed_half", (worst.T >> 1).astype(np.uint16))):   # its neighbours in the encoder's batch
        out.append(Case(f"tier1_19_planes_97x97_{name}", "tier1", img, dict(precision=16, levels=6, codeblock=64), (("levels", 6),)))
    return out


# ---- group "mq_t2" -----------------------------------------------------------------------------------------------------------

def segment_block(w, h, bits, seed, n, last):
    c = np.random.default_rng(seed).integers(-(1 << bits) + 1, 1 << bits, w * h)
    c[n:] = 0
    c[n - 1] = last
    return c.reshape(h, w)


def mq_t2_cases():
    out = []
    for length in SEGMENT_LENGTHS:
        w, h, *_ = SEGMENT_BLOCKS[length]
        out.append(Case(f"mq_t2_segment_{length}", "mq_t2", from_plane(segment_block(*SEGMENT_BLOCKS[length]), 0, 16),
                        dict(precision=16, levels=0, codeblock=64 if max(w, h) > 32 else 32), (("seglen", length),)))
    return out


# Headers and flushes that no raster is built for, but that these cases reach, each the smallest that does: a packet header with a
# 0xFF inside, one that ends on 0xFF and gets the zero byte, one whose last full byte is 0xFF with a partial byte behind it, one
# that ends on a full byte; the four outcomes of the flush (C lowered by 0x8000 or not, a final 0xFF dropped or not); coded bytes that end
# in 0xFF 0x7F when the flush begins; a two-byte segment; a carry that makes 0xFF.  The host test holds each case to its line.
ALSO_PLANTED = {
    "mq_t2_segment_8191": (("hdr_end", "full_ff"),), "mq_t2_segment_1023": (("hdr_end", "partial_after_ff"),),
    "levels_1x1_8_noise_p16_cb32": (("hdr_ff", "inside"), ("flush", (False, False))), "mq_t2_segment_1": (("hdr_end", "full"), ("flush", (True, True))),
    "levels_1x1_2_noise_p8_cb64": (("flush", (False, True)), ("seglen", 2)), "levels_2x2_2_noise_p16_cb32": (("flush", (True, False)),),
    "levels_33x65_3_ramp_p8_cb64": (("seg_tail", "ff7f"),), "levels_257x2_8_noise_p16_cb64": (("byteout", "carry_ff"),),
    "mq_t2_segment_4096": (("lblock", 6),), "mq_t2_segment_2048": (("lblock", 5),),
}


# ---- group "adversary" -------------------------------------------------------------------------------------------------------

def adversary(w, h, nplanes=15):
    """A copy of jpeg2000_model.t1_encode's traversal for LL that chooses each magnitude bit and each sign when the coder first asks for
    it: the less probable symbol of the context at that moment.  -> (signed coefficients h x w, the predicted segment)."""
    mq = m.MQEncoder()
    W = w + 2
    F = [0] * ((h + 2) * W)
    mag = [0] * (w * h)

    def lps(cx):
        return 1 - mq.mps[cx]

    def neighbours(i):
        return ((F[i - 1] & 1) + (F[i + 1] & 1), (F[i - W] & 1) + (F[i + W] & 1),
                (F[i - W - 1] & 1) + (F[i - W + 1] & 1) + (F[i + W - 1] & 1) + (F[i + W + 1] & 1))

    def contribution(i):
        return 0 if not F[i] & 1 else (-1 if F[i] & 2 else 1)

    def significant(i, y, x, p):
        mag[y * w + x] |= 1 << p
        hc = max(-1, min(1, contribution(i - 1) + contribution(i + 1)))
        vc = max(-1, min(1, contribution(i - W) + contribution(i + W)))
        flip = 0
        if hc < 0 or (hc == 0 and vc < 0):
            hc, vc, flip = -hc, -vc, 1
        cx = m.CTX_SIGN + (3 + vc if hc else vc)
        coded = lps(cx)
        if coded ^ flip:
            F[i] |= m.F_NEG
        mq.encode(cx, coded)
        F[i] |= m.F_SIG

    def zero_coding(i, y, x, p):
        cx = m.zc_context(LL, *neighbours(i))
        bit = lps(cx)
        mq.encode(cx, bit)
        if bit:
            significant(i, y, x, p)

    for p in range(nplanes - 1, -1, -1):
        if p != nplanes - 1:
            for y0 in range(0, h, 4):
                for x in range(w):
                    for y in range(y0, min(y0 + 4, h)):
                        i = (y + 1) * W + x + 1
                        if F[i] & m.F_SIG or sum(neighbours(i)) == 0:
                            continue
                        zero_coding(i, y, x, p)
                        F[i] |= m.F_VISIT
            for y0 in range(0, h, 4):
                for x in range(w):
                    for y in range(y0, min(y0 + 4, h)):
                        i = (y + 1) * W + x + 1
                        if (F[i] & (m.F_SIG | m.F_VISIT)) != m.F_SIG:
                            continue
                        cx = m.CTX_MAG + 2 if F[i] & m.F_REFINED else m.CTX_MAG + (1 if sum(neighbours(i)) else 0)
                        bit = lps(cx)
                        mq.encode(cx, bit)
                        mag[y * w + x] |= bit << p
                        F[i] |= m.F_REFINED
        for y0 in range(0, h, 4):
            for x in range(w):
                first = 0
                if y0 + 4 <= h:
                    idx = [(y0 + k + 1) * W + x + 1 for k in range(4)]
                    if all(not F[i] & (m.F_SIG | m.F_VISIT) and sum(neighbours(i)) == 0 for i in idx):
                        run = lps(m.CTX_RL)
                        mq.encode(m.CTX_RL, run)
                        if not run:
                            continue
                        hi, lo = lps(m.CTX_UNI), None
                        mq.encode(m.CTX_UNI, hi)
                        lo = lps(m.CTX_UNI)
                        mq.encode(m.CTX_UNI, lo)
                        r = 2 * hi + lo
                        significant(idx[r], y0 + r, x, p)
                        first = r + 1
                for y in range(y0 + first, min(y0 + 4, h)):
                    i = (y + 1) * W + x + 1
                    if F[i] & (m.F_SIG | m.F_VISIT):
                        continue
                    zero_coding(i, y, x, p)
        for i in range(len(F)):
            F[i] &= ~m.F_VISIT
    assert max(mag).bit_length() == nplanes
    coef = np.array([-v if F[(k // w + 1) * W + k % w + 1] & m.F_NEG else v for k, v in enumerate(mag)], np.int64).reshape(h, w)
    return coef, mq.flush()


def slab_cap(w, h, mb):
    """j2k_slab_cap of csrc/cct_internal.h"""
    return (w * h * (mb + 2) + 3) // 4 + 64


@functools.lru_cache(maxsize=None)
def adversaries():
    """{codeblock: (coefficients, predicted segment)}"""
    return {cb: adversary(cb, cb) for cb in (64, 32)}


def adversary_cases():
    return [Case(f"adversary_{cb}", "adversary", from_plane(coef, 0, 16), dict(precision=16, levels=0, codeblock=cb), (("seglen", len(seg)), ("nplanes", 15)))
            for cb, (coef, seg) in adversaries().items()]


# ---- the set -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cases():
    out = level_cases() + precision_cases() + tagtree_cases() + tier1_cases() + mq_t2_cases() + adversary_cases()
    assert set(ALSO_PLANTED) <= {c.name for c in out}
    out = [c._replace(planted=c.planted + ALSO_PLANTED.get(c.name, ())) for c in out]
    assert len({c.name for c in out}) == len(out)
    for c in out:
        assert c.raster.size <= MAX_SAMPLES or c.raster.shape == (257, 257), c.name
        assert c.raster.dtype == dtype_of(c.kw["precision"]), c.name
    return out


def parallel(fn, n):
    """[fn(0), .., fn(n - 1)] over up to 4 forked processes: pure-Python MQ coding is the whole run time of the host test.  fn is a
    function of a module; the children inherit what is cached here.  A process that has loaded the device library does not fork."""
    import multiprocessing
    import os
    import sys
    workers = min(4, os.cpu_count() or 1, n)
    if workers < 2 or "cct_hip" in sys.modules or "torch" in sys.modules:
        return [fn(k) for k in range(n)]
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        return pool.map(fn, range(n), 1)


CHUNKS = 16


def _encode_chunk(k):
    out = []
    for c in cases()[k::CHUNKS]:
        t = {}
        out.append((c.name, m.encode(c.raster, trace=t, **c.kw), t))
    return out


@functools.lru_cache(maxsize=None)
def _encoded():
    cases()
    done = {name: (f, t) for chunk in parallel(_encode_chunk, CHUNKS) for name, f, t in chunk}
    return {c.name: done[c.name] for c in cases()}


@functools.lru_cache(maxsize=None)
def _plain():
    return {c.name: m.encode(c.raster, **c.kw) for c in cases()}


def files(traced=False):
    """{name: file}: of a run without a trace, which takes half the time (the GPU test), or with traced=True of the run that traces() made"""
    return {name: f for name, (f, _) in _encoded().items()} if traced else _plain()


def traces():
    return {name: t for name, (_, t) in _encoded().items()}


def holds(trace, planted):
    """the planted items a trace lacks"""
    return [(key, item) for key, item in planted if not trace.get(key, {}).get(item)]


def kw_key(kw):
    return (kw["precision"], kw.get("shift", 0), kw["levels"], kw["codeblock"], bool(kw.get("jp2", False)))


@functools.lru_cache(maxsize=None)
def batches():
    """[(rows, cols, kw, [case])]: the cases that share a shape and the encoder's arguments, in the order of cases()"""
    groups = {}
    for c in cases():
        groups.setdefault((c.raster.shape, kw_key(c.kw)), []).append(c)
    return [(shape[0], shape[1], cs[0].kw, cs) for (shape, _), cs in groups.items()]


@functools.lru_cache(maxsize=None)
def decode_batches():
    """[(rows, cols, [case])]: the cases of one shape, whatever their coding: what one jpeg2000_decode_batch call can hold"""
    groups = {}
    for c in cases():
        groups.setdefault(c.raster.shape, []).append(c)
    return [(shape[0], shape[1], cs) for shape, cs in groups.items()]
