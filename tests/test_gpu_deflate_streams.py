"""Device INFLATE (inflate_kernels.hip) on the hand-built streams of tests/deflate_streams.py: streams zlib's deflate never
writes.  The expectation is tests/golden/deflate_streams.json (zlib's verdict and the SHA-256 of its output, which
tests/test_deflate_streams_host.py holds CPython's zlib to); the preconditions that make a case reach its path are asserted
there as well.  Here every case goes through zlib_decompress_batch in one batch per geometry, forwards and reversed, and a
handful through the PNG reader and the .cct decoder."""
import hashlib
import json
import os

import numpy as np
import pytest

import deflate_streams as ds
import golden_inputs as gi
import png_files as pf

pytestmark = pytest.mark.gpu

with open(os.path.join(gi.GOLDEN, "deflate_streams.json")) as _f:
    RECORDS = {r["name"]: r for r in json.load(_f)["records"]}


@pytest.fixture(scope="module", params=[256, 512], ids=["inflate256", "inflate512"])
def hip(request):
    """both geometries of the INFLATE kernel, as in test_gpu_deflate.py"""
    import cct_hip
    from cct_hip import _ffi
    cct_hip.device_info()
    _ffi.check(_ffi.lib().cct_set_option(b"inflate_lanes", request.param))
    yield cct_hip
    _ffi.check(_ffi.lib().cct_set_option(b"inflate_lanes", 0))


def _batch(groups):
    """[(name, stream)] of the cases of these groups, in the order of the case list"""
    return [(c.name, c.stream) for c in ds.cases() if c.group in groups]


def _run(hip, items, max_out):
    """one batch; -> number of cases compared.  Status 0 with the fixture's bytes, or CCT_E_ZLIB, for every case."""
    outs, status = hip.zlib_decompress_batch([s for _, s in items], max_out=max_out, raise_errors=False)
    wrong = []
    for (name, _), out, st in zip(items, outs, status):
        rec = RECORDS[name]
        if rec["accept"]:
            ok = st == 0 and out is not None and len(out) == rec["out_len"] and hashlib.sha256(out).hexdigest() == rec["sha256"]
        else:
            ok = st == ds.E_ZLIB and out is None
        if not ok:
            wrong.append((name, int(st), None if out is None else len(out), rec.get("out_len")))
    assert not wrong, f"{len(wrong)} of {len(items)} cases: (name, status, bytes, bytes wanted) {wrong[:8]}"
    return len(items)


def _both_orders(hip, groups):
    items = _batch(groups)
    n = _run(hip, items, ds.max_out())
    _run(hip, items[::-1], ds.max_out())  # other neighbours, other byte alignments
    return n


# the graded order of the file: accepted streams, then refusals, then truncations
def test_accepted_streams(hip):
    assert _both_orders(hip, ("accept",)) == sum(1 for r in RECORDS.values() if r["group"] == "accept")


def test_refused_streams_between_accepted_ones(hip):
    """every refused stream with accepted neighbours: a refusal must not disturb the stream behind it"""
    good = _batch(("accept",))
    small = [g for g in good if RECORDS[g[0]]["stream_len"] < 1500]
    items = []
    for k, bad in enumerate(_batch(("refuse",))):
        items += [bad, small[k % len(small)]]
    assert _run(hip, items, ds.max_out()) == len(items)
    _run(hip, items[::-1], ds.max_out())


def test_truncated_streams_between_accepted_ones(hip):
    small = [g for g in _batch(("accept",)) if RECORDS[g[0]]["stream_len"] < 1500]
    items = []
    for k, bad in enumerate(_batch(("truncate",))):
        items += [bad, small[-1 - k]]
    assert _run(hip, items, ds.max_out()) == len(items)
    _run(hip, items[::-1], ds.max_out())


def test_all_cases_in_one_batch_both_orders(hip):
    n = _both_orders(hip, ("accept", "refuse", "truncate"))
    assert n == len(ds.cases()) == sum(1 for r in RECORDS.values() if r["group"] != "cap")


def test_capacity_edges(hip):
    """an output of exactly max_out fits; one byte and one 16-byte granule past the slot give CCT_E_CAP; the slots around them
    hold their own bytes.  (cap_one_byte_above_out_stride found the last flush of an over-long output reported as a bad Adler-32,
    CCT_E_ZLIB: the stored blocks flush whole 4 KiB pieces, so only the flush before the trailer crosses the slot's end.)"""
    m = ds.max_out()
    ring = next(c for c in ds.cases() if c.name == "ring_258_32768_to_200k")
    small = next(c for c in ds.cases() if c.name == "long_distance_codes")
    caps = ds.cap_cases()
    items = [(ring.name, ring.stream)]
    for name, stream, _ in caps:
        items += [(name, stream), (small.name, small.stream), (ring.name, ring.stream)]
    outs, status = hip.zlib_decompress_batch([s for _, s in items], max_out=m, raise_errors=False)
    want_status = {name: st for name, _, st in caps}
    for (name, _), out, st in zip(items, outs, status):
        rec = RECORDS[name]
        assert st == want_status.get(name, 0), (name, int(st))
        if st == 0:
            assert len(out) == rec["out_len"] and hashlib.sha256(out).hexdigest() == rec["sha256"], name
        else:
            assert out is None
    assert RECORDS["cap_exactly_max_out"]["out_len"] == m
    # the slot size the cases were sized for is the product's: a stream of out_stride bytes still fits, one more does not
    probe = [ds._stored_run(ds.out_stride(m), 63), ds._stored_run(ds.out_stride(m) + 1, 61)]
    _, st = hip.zlib_decompress_batch(probe, max_out=m, raise_errors=False)
    assert list(st) == [0, ds.E_CAP]


# ---- the other two entrances: the same paths with the payload each entrance expects ----------------------------------------
def _png_cases():
    """[(name, file, raster, precondition)]: 8-bit rasters whose filtered rows are the payload of a hand-built stream"""
    out = []
    rng = np.random.default_rng(70)
    img = rng.integers(0, 256, (24, 31), dtype=np.uint16)
    types = rng.integers(0, 5, 24)
    rows = pf.filtered(img, 8, types)
    out.append(("long-header", ds.zlib_stream([ds.long_header_block(rows)]), img, ds.pre_long_header))
    out.append(("long-header-16", ds.zlib_stream([ds.long_header_16_block(rows)]), img, lambda w: ds.pre_long_header(w, 16)))
    # long codes: filter type 0 rows over the twelve literals of the alphabet, end-of-block on the 15-bit code
    img = rng.integers(1, 12, (24, 31), dtype=np.uint16)
    body = list(pf.filtered(img, 8, [0] * 24))
    for v in range(3):
        b = ds.dynamic(ds.long_ll_lens(v), [0], body, final=True)
        out.append((f"long-codes-{v}", ds.zlib_stream([b]), img, lambda w, v=v: _long_seen(w, v)))
    # the copy list: filter type 1 (Sub) on every row and every byte 1: a run of 6400 ones, samples 1, 2, 3, ...
    img = np.tile(np.arange(1, 80, dtype=np.uint16), (80, 1))
    assert pf.filtered(img, 8, [1] * 80) == b"\x01" * 6400
    ll = list(ds.RUN_LL)
    ll[1], ll[97] = ll[97], 0
    out.append(("mlist-cap", ds.zlib_stream([ds.run_block([1], [ds.copy(3, 1)] * ds.N_RUN, ll=ll)]), img, ds.pre_mlist))
    return out


def _long_seen(w, v):
    want = {(ds.LONG_KINDS[(k + v) % 3], 13 + k) for k in range(3)} - {("len", 13), ("len", 14), ("len", 15)}
    seen = {(s.kind, s.nbits) for s in w["blocks"][0]["syms"] if s.nbits > ds.LL_BITS}
    assert w["error"] is None and want <= seen and seen


def test_png_entrance(hip):
    cases = _png_cases()
    for name, stream, img, pre in cases:
        w = ds.walk(stream)
        pre(w)
        assert ds.oracle_verdict(stream) == w["out"] == pf.filtered(img, 8, [w["out"][r * (img.shape[1] + 1)] for r in range(img.shape[0])])
    by_shape = {}
    for c in cases:
        by_shape.setdefault(c[2].shape, []).append(c)
    for shape, group in by_shape.items():
        files = [pf.make_png(img, 8, 0, stream=stream) for _, stream, img, _ in group]
        got = hip.png_read_batch(files)
        for k, (name, _, img, _) in enumerate(group):
            assert np.array_equal(got[k], img), name
        got = hip.png_read_batch(files[::-1])
        for k, (name, _, img, _) in enumerate(group[::-1]):
            assert np.array_equal(got[k], img), name + " (reversed)"


def test_cct_entrance(hip):
    """the payloads of real .cct files behind hand-built streams, device INFLATE on and off"""
    from cct_hip import _ffi
    from oracle import oracle
    L = _ffi.lib()
    cfg = hip.default_config()
    flat = np.full((128, 128), 1000, np.uint16)
    imgs = [gi.ct_phantom(3, 64), flat]
    raw = [oracle.encode(im, deflate=False) for im in imgs]
    assert all(r[12] == 0 for r in raw)
    pay = raw[0][13:]
    streams = [("long-header", ds.zlib_stream([ds.long_header_block(pay)]), ds.pre_long_header, 0),
               ("long-header-16", ds.zlib_stream([ds.long_header_16_block(pay)]), lambda w: ds.pre_long_header(w, 16), 0)]
    streams.append(("long-codes", _long_codes_stream(pay), _long_any, 0))
    # the copy list: the flat image's payload is one long run
    p1 = raw[1][13:]
    streams.append(("mlist-cap", _greedy_runs_stream(p1), ds.pre_mlist, 1))
    for name, stream, pre, k in streams:
        w = ds.walk(stream)
        pre(w)
        assert ds.oracle_verdict(stream) == raw[k][13:], name
    for k in (0, 1):
        files = [raw[k][:12] + b"\x01" + s for _, s, _, kk in streams if kk == k]
        for dev in (1, 0):
            _ffi.check(L.cct_set_option(b"device_inflate", dev))
            try:
                got = hip.decode_batch(files, cfg)
            finally:
                _ffi.check(L.cct_set_option(b"device_inflate", 1))
            for g in got:
                assert np.array_equal(g, imgs[k]), (k, dev)


def _long_any(w):
    seen = {(s.kind, s.nbits) for b in w["blocks"] for s in b["syms"] if s.nbits > ds.LL_BITS}
    assert w["error"] is None and {("lit", 13), ("len", 14), ("eob", 15), ("lit", 15)} <= seen, seen


def _long_codes_stream(pay):
    """any payload behind the 1 .. 14, 15, 15 ladder: the sixteen symbols are the payload's thirteen commonest bytes, lengths 3
    and 4 and end-of-block; every other byte travels in a one-byte stored block between the Huffman blocks, and the first run
    of five equal bytes of the alphabet is written as a literal and a copy (4, 1) on the 14-bit length code"""
    vals, counts = np.unique(np.frombuffer(pay, np.uint8), return_counts=True)
    common = [int(v) for v in vals[np.argsort(-counts, kind="stable")]][:13]
    assert len(common) == 13
    ll = ds.long_ll_lens(0, tuple(common[:12]), extra=common[12])
    at = next(i for i in range(1, len(pay) - 4) if pay[i:i + 4] == pay[i - 1:i] * 4 and ll[pay[i]])
    blocks, body, k = [], [], 0
    while k < len(pay):
        if k == at:
            body.append(ds.copy(4, 1))
            k += 4
            continue
        if ll[pay[k]]:
            body.append(pay[k])
        else:
            blocks += [ds.dynamic(ll, [1], body), ds.stored(pay[k:k + 1])]
            body = []
        k += 1
    blocks.append(ds.dynamic(ll, [1], body, final=True))
    assert ds.expand(blocks) == pay
    return ds.zlib_stream(blocks)


def _greedy_runs_stream(pay):
    """a payload that is mostly one long run as literals and (3, 1) copies, two bits each, in one dynamic block"""
    used = sorted(set(pay))
    body, k = [], 0
    while k < len(pay):
        if k >= 1 and pay[k:k + 3] == pay[k - 1:k] * 3:
            body.append(ds.copy(3, 1))
            k += 3
        else:
            body.append(pay[k])
            k += 1
    ll = [0] * 258
    ll[257] = 1
    rest = ds.balanced(used + [256], 257)
    for s in used + [256]:
        ll[s] = rest[s] + 1
    b = ds.dynamic(ll, [1], body, final=True)
    assert ds.expand([b]) == pay
    return ds.zlib_stream([b])
