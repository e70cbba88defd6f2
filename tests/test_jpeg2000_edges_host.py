"""tests/jpeg2000_edges.py without a device: both models invert every case and their traces agree event for event; where Pillow has
the codec, OpenJPEG decodes every raw codestream to the raster; the census over the encoder model's traces shows every planted item,
one assertion per item, so that a changed raster generator or shape list is noticed here and not by a silently emptier GPU test; the
census of jpeg2000_model.matrix() and phantoms() is pinned too; every one-rule mutant of the model changes the file of some case.

Run time, measured alone on the 8-CPU machine this was written on: 37 s (7 s the traced encodes of the 540 cases, 15 s their traced
decodes, 19 s the traces of matrix() and phantoms(), 3 s the rest).  Pure-Python MQ coding sets all of it, so those three parts run over
up to four forked processes (jpeg2000_edges.parallel); in one process they add up to about 90 s.
"""
import functools
import types

import numpy as np
import pytest

import jpeg2000_decode_model as d
import jpeg2000_edges as e
import jpeg2000_model as m
from jpeg2000_model import HH, HL, LH, LL

SHARED_KEYS = ("zc", "zc_ctx", "sign", "rl", "mag_ctx", "nplanes", "block", "mq_state", "mq_ctx", "passes", "zbp", "seglen", "levels", "precision")


@functools.lru_cache(maxsize=None)
def census(group=None):
    tr = e.traces()
    return m.merge(tr[c.name] for c in e.cases() if group in (None, c.group))


def model_files():
    return e.files(traced=True)


def hvd(pattern):
    b = [(pattern >> k) & 1 for k in range(8)]  # jpeg2000_model.NEIGHBOURS: NW N NE W E SW S SE
    return b[3] + b[4], b[1] + b[6], b[0] + b[2] + b[5] + b[7]


# ---- the cases ---------------------------------------------------------------------------------------------------------------

def test_the_set_holds_every_group_shape_level_and_precision():
    cs = e.cases()
    assert {c.group for c in cs} == {"levels", "precision", "tagtree", "tier1", "mq_t2", "adversary"} and 300 <= len(cs) <= 600
    assert max(c.raster.size for c in cs if c.raster.shape != (257, 257)) <= e.MAX_SAMPLES
    lv = {(c.raster.shape, c.kw["levels"], c.kw["codeblock"]) for c in cs if c.group == "levels"}
    assert {s for s, _, _ in lv} == set(e.LEVEL_SHAPES) and {l for _, l, _ in lv} == {2, 3, 4, 6, 7, 8}
    assert {(s, l) for s, l, _ in lv} == {(s, l) for s in e.LEVEL_SHAPES for l in e.DEEP_LEVELS}
    assert all({cb for s, _, cb in lv if s == shape} == {32, 64} for shape in e.LEVEL_SHAPES) and all({cb for _, l, cb in lv if l == levels} == {32, 64} for levels in e.DEEP_LEVELS)
    assert all({cb for s, l, cb in lv if (s, l) == (shape, 8)} == {32, 64} for shape in e.LEVEL_SHAPES)
    assert sum(1 for c in cs if c.kw.get("jp2") and c.kw["levels"] == 8) == 18
    deep = [b for b in e.batches() if b[3][0].group == "levels"]
    assert len(deep) == 48 and all(len(b[3]) == 3 for b in deep)        # the encoder never runs a new depth on one frame alone
    assert {b[2]["precision"] for b in deep if b[2]["levels"] >= 6} == {8, 12, 16}
    assert all(len(b[3]) >= 3 for b in e.batches() if b[2]["levels"] >= 6)
    pr = [c for c in cs if c.group == "precision"]
    assert {(c.kw["precision"], c.raster.shape, c.kw["levels"]) for c in pr if "shift" not in c.kw} == {
        (p, s, l) for p in (2, 3, 7, 9, 15) for s in ((5, 3), (33, 65)) for l in (0, 2, 5)}
    assert {c.kw["precision"] - c.kw["shift"] for c in pr if "shift" in c.kw} == {1, 2}
    assert {c.raster.shape for c in cs if c.group == "tagtree"} == {(3, 300), (300, 3), (1, 600), (97, 161), (257, 257)}


def _decode_chunk(k):
    """-> what is wrong with the cases k, k + CHUNKS, ..: decoded at 16 bits allocated, at 8 where the precision fits, with the shift on the way back and without"""
    files, traces, wrong = model_files(), e.traces(), []
    for c in e.cases()[k::e.CHUNKS]:
        p, shift = c.kw["precision"], c.kw.get("shift", 0)
        t = {}
        got = d.decode(files[c.name], *c.raster.shape, bits=8 if p <= 8 else 16, shift=shift, trace=t)
        if isinstance(got, str) or got.dtype != c.raster.dtype or not np.array_equal(got, c.raster):
            wrong.append((c.name, "raster"))
        wrong += [(c.name, key) for key in SHARED_KEYS if (t.get(key) or {}) != (traces[c.name].get(key) or {})]
        if p <= 8:  # 8 bits of precision fit 16 allocated too
            got = d.decode(files[c.name], *c.raster.shape, bits=16, shift=shift)
            if got.dtype != np.uint16 or not np.array_equal(got, c.raster):
                wrong.append((c.name, "16 bits allocated"))
        if shift and not np.array_equal(d.decode(files[c.name], *c.raster.shape), c.raster.astype(np.uint16) << shift):
            wrong.append((c.name, "without the shift"))
    return wrong


def test_both_models_invert_every_case_and_their_traces_agree():
    e.traces()
    wrong = [w for chunk in e.parallel(_decode_chunk, e.CHUNKS) for w in chunk]
    assert not wrong, wrong[:10]


def test_pillow_decodes_every_raw_codestream():
    """OpenJPEG through Pillow scales precision p to the container: x << (8 - p) up to 8 bits, x << (16 - p) from 9 to 16.  JP2 files
    stay with the models: Pillow's box reader takes the 8-bit-per-component field its own way."""
    if not d.pillow_has_jpeg2000():
        pytest.skip("this Pillow has no JPEG 2000 codec")
    import io
    from PIL import Image
    files, n = model_files(), 0
    for c in e.cases():
        if c.kw.get("jp2"):
            continue
        p = c.kw["precision"]
        im = Image.open(io.BytesIO(files[c.name]))
        got = np.array(im).astype(np.int64)
        want = (c.raster.astype(np.int64) << c.kw.get("shift", 0)) << ((8 if p <= 8 else 16) - p)
        assert im.mode == ("L" if p <= 8 else "I;16") and np.array_equal(got, want), c.name
        n += 1
    assert n == len(e.cases()) - 18


# ---- the census --------------------------------------------------------------------------------------------------------------

def test_every_case_reaches_what_it_plants():
    tr = e.traces()
    for c in e.cases():
        assert not e.holds(tr[c.name], c.planted), (c.name, e.holds(tr[c.name], c.planted)[:5])
    assert all(c.planted for c in e.cases() if c.group in ("levels", "precision", "tagtree", "mq_t2", "adversary"))


def test_census_neighbour_patterns():
    zc = census("tier1")["zc"]
    for orient in e.ORIENTS:
        assert {pat for o, pat, _ in zc if o == orient} == set(range(256)), orient
        assert {pat for o, pat, kind in zc if o == orient and kind == "sp"} == set(range(1, 256)), orient   # 0 has no neighbour to propagate from
        assert (orient, 0, "cu") in zc
        assert len({hvd(pat) for o, pat, _ in zc if o == orient}) == 45
    ctx = census()["zc_ctx"]
    assert {(o, cx, bit) for o in e.ORIENTS for cx in range(9) for bit in (0, 1)} <= set(ctx)


def test_census_sign_keys():
    sign = census("tier1")["sign"]
    assert {(key, neg) for key in e.SIGN_KEYS for neg in (0, 1)} == set(sign) and len(sign) == 162


def test_census_mq_coder():
    c = census()
    assert {(cx, what) for cx in range(m.N_CTX) for what in ("mps", "lps")} == set(c["mq_ctx"])
    assert set(c["mq_state"]) == set(range(47))
    assert set(c["byteout"]) == {"stuff", "carry_ff", "carry", "plain"} and min(c["byteout"].values()) >= 10, c["byteout"]
    assert set(c["flush"]) == {(a, b) for a in (False, True) for b in (False, True)}
    assert c["seg_tail"]["ff7f"] >= 1
    assert set(c["mag_ctx"]) == {m.CTX_MAG, m.CTX_MAG + 1, m.CTX_MAG + 2}


def test_census_candidate_rows():
    """Propagation and refinement reach every mask.  The cleanup pass cannot: a row it skips (significant or visited) between
    two rows it codes would need a significant sample that touches the middle row alone, and a skipped row right above the block's
    lower edge under a coded one would need one below the block, so its masks are runs of adjacent rows, and in a partial stripe runs
    that end at the last row, or the first rows skipped as a whole (their cause lies in the stripe above)."""
    rows = set(census("tier1")["rows"])
    cleanup = {4: {0, 1, 2, 3, 4, 6, 7, 8, 12, 14, 15}, 3: {0, 1, 4, 6, 7}, 2: {0, 2, 3}, 1: {0, 1}}
    for orient in e.ORIENTS:
        for n in (1, 2, 3, 4):
            for kind in ("sp", "mr"):
                assert {mask for o, k, nn, mask in rows if (o, k, nn) == (orient, kind, n)} == set(range(1 << n)), (orient, kind, n)
            assert {mask for o, k, nn, mask in rows if (o, k, nn) == (orient, "cu", n)} == cleanup[n], (orient, n)
    assert {(n, mask) for _, k, n, mask in census()["rows"] if k == "cu"} == {(n, mask) for n in cleanup for mask in cleanup[n]}   # nor does any other case


def test_census_run_length_mode():
    c = census("tier1")
    assert set(c["rl"]) == {0, 1, 2, 3, 4}
    for orient in e.ORIENTS:
        off = {key[1:] for key in c["rl_off"] if key[0] == orient}
        assert {sig for sig, _, _ in off if bin(sig).count("1") == 1} == {1, 2, 4, 8}, orient                 # one significant sample, in each row
        assert {vis for sig, vis, _ in off if sig == 0 and bin(vis).count("1") == 1} == {1, 8}, orient       # one visited sample: rows 0 and 3 only
        alone = {nbr for sig, vis, nbr in off if sig == 0 and vis == 0}
        assert set(e.RL_OFF_NEIGHBOUR_MASKS) <= alone, orient                                                # one significant neighbour sample
        assert alone == set(range(1, 16)) - set(e.UNREACHABLE_NEIGHBOUR_MASKS), orient
    off = {key[1:] for key in census()["rl_off"]}                                                            # and in no other case either
    assert not {(sig, vis) for sig, vis, _ in off} & set(e.UNREACHABLE_RL_OFF)
    assert not {nbr for sig, vis, nbr in off if sig == 0 and vis == 0} & set(e.UNREACHABLE_NEIGHBOUR_MASKS)
    assert {"col", "row"} == set(c["edge_sig"])
    blocks = {(w, h) for w, h, _ in c["block"]}
    assert {(64, 64), (32, 32), (1, 9), (9, 1), (30, 5), (30, 6), (30, 7), (1, 32), (32, 1), (1, 1), (33, 64), (33, 1)} <= blocks, sorted(blocks)
    for orient in e.ORIENTS:
        assert {(64, 64, orient), (32, 32, orient), (1, 9, orient), (9, 1, orient)} <= set(c["block"])


def test_census_planes_passes_and_zero_planes():
    c = census()
    assert e.MOST_PLANES == 19 and set(c["nplanes"]) == set(range(1, 20)) - set() and max(c["nplanes"]) == 19
    assert set(c["passes"]) == {3 * n - 2 for n in range(1, 20)}
    assert set(c["zbp"]) == set(range(0, 19))       # 19 zero planes of Mb 19 would be a block of zeros, which is not included
    assert e.search_most_planes() == 18             # what 0 / 65535 rasters at 1 to 3 levels reach; the docstring says why
    gains = [e.worst_gain(220, lv)[0] for lv in range(1, 8)]
    assert [g * g >= 8 for g in gains] == [False] * 5 + [True] * 2 and max(gains) < 2.9
    assert e.worst_gain(96, 6)[0] ** 2 < 8 <= e.worst_gain(97, 6)[0] ** 2
    assert e.planes_of(e.worst_raster(97, 6), 16, 6)[HH] == 19


def test_census_tier2():
    c = census()
    assert set(c["lblock"]) == set(range(7))
    assert set(e.SEGMENT_LENGTHS) <= set(c["seglen"]) and len(e.SEGMENT_LENGTHS) == 26 and e.SEGMENT_LENGTHS[-1] == 8192
    assert set(e.SEGMENT_LENGTHS) <= set(census("mq_t2")["seglen"])
    assert set(c["hdr_end"]) == {"partial", "partial_after_ff", "full", "full_ff"} and c["hdr_ff"]["inside"] >= 10
    t = census("tagtree")
    assert {lv for _, _, lv in c["tt_levels"]} >= {1, 2, 3, 4, 5}
    assert {(10, 1, 5), (1, 10, 5), (6, 4, 4), (9, 9, 5)} <= set(t["tt_levels"])      # non-square; 9 x 9 is odd at every level
    assert {(name, lv) for name in ("incl", "zbp") for lv in range(5)} <= set(t["tt_learnt"])
    assert {("zbp", lv) for lv in range(4)} | {("incl", lv) for lv in range(3)} <= set(t["tt_low"])
    incl = set(t["included"])
    assert {(10, 1), (10, 10), (10, 5), (10, 9), (24, 1), (24, 23), (81, 1), (81, 80), (81, 81)} <= incl, sorted(incl)


def test_census_levels_and_precisions():
    c = census()
    assert set(c["levels"]) == set(range(9)) and set(c["precision"]) == {2, 3, 7, 8, 9, 12, 15, 16}
    assert {2, 1, 3, 5, 10, 19, 38, 75, 150, 300, 257, 129, 65, 33, 17, 9} <= set(c["lengths"])
    files = model_files()
    assert all(files[c.name][:4] == (b"\x00\x00\x00\x0c" if c.kw.get("jp2") else b"\xff\x4f\xff\x51") for c in e.cases())
    jp2 = next(c for c in e.cases() if c.kw.get("jp2"))
    assert jp2.kw["levels"] == 8 and files[jp2.name].index(b"\xff\x93") + 2 == 188   # of J2K_HDR_MAX = 192 (csrc/cct_internal.h)


def test_adversary():
    """The block that offers the coder its less probable symbol every time: encode() writes exactly the predicted segment, and the
    segment stays inside the slab the device grants, (w * h * (mb + 2) + 3) // 4 + 64 bytes."""
    files = model_files()
    for cb, (coef, seg) in e.adversaries().items():
        c = next(c for c in e.cases() if c.name == f"adversary_{cb}")
        assert np.array_equal(c.raster.astype(np.int64) - 32768, coef) and int(np.abs(coef).max()) < 1 << 15
        assert m.packet_data(files[c.name]) == m.packet([(1, 1, [(43, 2, seg)], 17)])
        ratio = len(seg) / e.slab_cap(cb, cb, 17)
        print(f"adversary {cb} x {cb}: {len(seg)} bytes of {e.slab_cap(cb, cb, 17)}, ratio {ratio:.4f}")
        assert round(ratio, 3) == e.ADVERSARY_RATIO[cb]
        assert ratio <= 1


# one job per phantom and per (precision, shape) of matrix(), the long ones (128 x 128, 130 x 70) first
MATRIX_JOBS = sorted([("phantoms", k) for k in range(6)] + [(p, k) for p in m.PRECISIONS for k in range(len(m.SHAPES))],
                     key=lambda job: (job[0] != "phantoms" and m.SHAPES[job[1]][0] * m.SHAPES[job[1]][1] < 9000, str(job)))


def _matrix_job(j):
    """the trace of one shape of matrix() at one precision, without its files (tests/test_jpeg2000_model.py holds those to Pillow), or of one phantom"""
    precision, k = MATRIX_JOBS[j]
    t = {}
    if precision == "phantoms":
        img, kw, f = m.phantoms()[k]
        assert m.encode(img, trace=t, **kw) == f  # the trace changes no byte
        return t
    rows, cols, cbs = m.SHAPES[k]
    for x in m.raster_cases(rows, cols, precision, m.PRECISIONS[precision]).values():
        for cb in cbs:
            for levels in m.LEVELS:
                m.encode(x, precision, 0, levels, cb, trace=t)
    return t


@functools.lru_cache(maxsize=None)
def matrix_census():
    assert len(m.phantoms()) == 6
    traces = e.parallel(_matrix_job, len(MATRIX_JOBS))
    return {p: m.merge(t for (q, _), t in zip(MATRIX_JOBS, traces) if q == p) for p in list(m.PRECISIONS) + ["phantoms"]}


def test_census_of_the_matrix_and_the_phantoms():
    """What jpeg2000_model.matrix() and phantoms() reach and what they do not, so that a change to them is noticed too."""
    per = matrix_census()
    c = m.merge(per.values())
    assert set(c["levels"]) == {0, 1, 5} and set(c["precision"]) == {8, 12, 16}
    assert max(lv for _, _, lv in c["tt_levels"]) == 4 and max(w * h for w, h, _ in c["tt_levels"]) == 16 and (3, 5, 4) in c["tt_levels"]
    assert max(c["passes"]) == 49 and max(c["nplanes"]) == 17
    for orient in e.ORIENTS:
        assert len({hvd(pat) for o, pat, _ in c["zc"] if o == orient}) == 45
    assert set(c["mq_state"]) == set(range(47)) and 45 not in per["phantoms"]["mq_state"]   # state 45: only through the matrix
    assert set(c["byteout"]) == {"stuff", "carry_ff", "carry", "plain"}
    assert all(11 <= per[p]["byteout"]["carry_ff"] <= 35 for p in m.PRECISIONS)
    assert len(c["flush"]) == 4 and set(c["lblock"]) == set(range(7))
    assert {n for n, k in c["included"] if k < n} and all(k in (0, n) or n <= 15 for n, k in c["included"])


# ---- mutants -----------------------------------------------------------------------------------------------------------------

def _swap(f, orients, a, b):
    """zc_context with the entries of (h, v, d) = a and b of one Table D.1 column exchanged"""
    def zc(orient, h, v, dd):
        if orient in orients and (h, v, dd) in (a, b):
            h, v, dd = b if (h, v, dd) == a else a
        return f(orient, h, v, dd)
    return zc


# (name, [(text of jpeg2000_model.py, replacement)]) or (name, a function that patches the loaded copy)
MUTANTS = (
    ("D.1 LL / LH: h 1, v 0: d 0 and d 1 exchanged (5, 6)", lambda mod: setattr(mod, "zc_context", _swap(mod.zc_context, (LL, LH), (1, 0, 0), (1, 0, 1)))),
    ("D.1 HL: v 1, h 0: d 0 and d 1 exchanged (5, 6)", lambda mod: setattr(mod, "zc_context", _swap(mod.zc_context, (HL,), (0, 1, 0), (0, 1, 1)))),
    ("D.1 HH: d 1: h + v 0 and 1 exchanged (3, 4)", lambda mod: setattr(mod, "zc_context", _swap(mod.zc_context, (HH,), (0, 0, 1), (1, 0, 1)))),
    ("sign key: W and N exchanged", [("hc = max(-1, min(1, contribution(i - 1) + contribution(i + 1)))\n        vc = max(-1, min(1, contribution(i - W) + contribution(i + W)))",
                                      "hc = max(-1, min(1, contribution(i - W) + contribution(i + 1)))\n        vc = max(-1, min(1, contribution(i - 1) + contribution(i + W)))")]),
    ("D.3: no flip for hc = 0, vc < 0", [("if hc < 0 or (hc == 0 and vc < 0):\n            hc, vc, flip = -hc, -vc, 1", "if hc < 0 or (hc == 0 and vc < 0):\n            hc, vc, flip = -hc, -vc, int(hc < 0)")]),
    ("run-length mode ignores the neighbour bits", [("if all(not F[i] & (F_SIG | F_VISIT) and sum(neighbours(i)) == 0 for i in idx):", "if all(not F[i] & (F_SIG | F_VISIT) for i in idx):")]),
    ("the visit mark is not cleared after the cleanup", [("            F[i] &= ~F_VISIT\n", "            pass\n")]),
    ("CTX_MAG + 1 without looking at the neighbours", [("cx = CTX_MAG + (1 if sum(neighbours(i)) else 0)", "cx = CTX_MAG + 1")]),
    ("stuffing test after the carry", [("    def _byteout(self):\n        tr = self.trace\n        if self.b == 0xFF:",
                                        "    def _byteout(self):\n        tr = self.trace\n        if self.c >= 0x8000000:\n            self.b, self.c = (self.b + 1) & 0xFF, self.c & 0x7FFFFFF\n        if self.b == 0xFF:")]),
    ("the flush keeps a final 0xFF", [("if self.b != 0xFF and self.pos >= 0:\n            self.out.append(self.b)\n        if tr is not None:\n            count(tr, \"flush\"", "if self.pos >= 0:\n            self.out.append(self.b)\n        if tr is not None:\n            count(tr, \"flush\"")]),
    ("a tag-tree parent is its first child", [("self.val.append([min(prev[yy * pw + xx] for yy in", "self.val.append([next(prev[yy * pw + xx] for yy in")]),
    ("`low` is not carried down a level", [("            low = max(low, self.low[lv][k])\n", "            low = self.low[lv][k]\n")]),
    ("Lblock starts at 4", [("grow = max(0, need - 3)", "grow = max(0, need - 4)"), ("bw.bits(len(data), 3 + grow + passes.bit_length() - 1)", "bw.bits(len(data), 4 + grow + passes.bit_length() - 1)")]),
    ("Table B.4: 35 / 36 instead of 36 / 37", [("elif n <= 36:", "elif n <= 35:"), ("bw.bits(n - 37, 7)", "bw.bits(n - 36, 7)")]),
    ("5/3 rounding + 1 >> 2", [("((d[:-1] + d[1:] + 2) >> 2)", "((d[:-1] + d[1:] + 1) >> 2)")]),
    ("the edge sample repeated instead of mirrored", [("        i = np.abs(i)\n        i = np.where(i >= n, 2 * (n - 1) - i, i)\n        return x[np.abs(i)]", "        return x[np.clip(i, 0, n - 1)]")]),
)
# "W and E exchanged in the sign key" changes no file and is not in the list: the horizontal contribution is the clamped sum of the
# two (T.800 Table D.2), which does not know which is which.  A device table indexed by position can still have them exchanged
# and agree; the nearest rule that can be wrong, W exchanged with N, is the fourth mutant.


def mutant_model(change):
    path = m.__file__
    with open(path) as f:
        text = f.read()
    if not callable(change):
        for old, new in change:
            assert text.count(old) == 1, old
            text = text.replace(old, new)
    mod = types.ModuleType("jpeg2000_model_mutant")
    mod.__file__ = path
    exec(compile(text, path, "exec"), mod.__dict__)
    if callable(change):
        change(mod)
    return mod


def test_every_mutant_changes_a_file():
    files = model_files()
    order = sorted(e.cases(), key=lambda c: (c.group not in ("tier1", "mq_t2"), c.raster.size))
    table = []
    for name, change in MUTANTS:
        mod = mutant_model(change)
        caught = None
        for c in order:
            try:
                same = mod.encode(c.raster, **c.kw) == files[c.name]
            except (OverflowError, ValueError, StopIteration):
                same = False
            if not same:
                caught = c.name
                break
        table.append((name, caught))
    print()
    for name, caught in table:
        print(f"{name:55s} {caught}")
    assert all(caught for _, caught in table), [name for name, caught in table if not caught]
    assert mutant_model([]).encode(order[40].raster, **order[40].kw) == files[order[40].name]  # the copy itself is the model
