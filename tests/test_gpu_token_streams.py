"""The decode kernel (csrc/decode_kernels.hip, token stream -> raster) on streams that no encoder of ours wrote: the
hand-built and damaged files of tests/token_streams.py, judged per file.  tests/test_token_streams_host.py checks the
writer, the judge and the balance of the damaged sets without a device.

The rule per file, with o the oracle's result and c the judge's (token_streams.classify):
  c is None, o is pixels      status 0 and the oracle's raster, byte for byte
  c is None, o is E_OVERFLOW  status CCT_E_OVERFLOW
  c names a defect            status CCT_E_STREAM (it outranks overflow), whatever o says
and never anything else."""
import collections
import ctypes as C
import zlib

import numpy as np
import pytest

import token_streams as ts

pytestmark = pytest.mark.gpu

WG_THREADS = (256, 512, 1024)  # every value the wg_threads option accepts
MAGIC = b"pact"


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    info = cct_hip.device_info()  # raises if the extension or the GPU is missing: no fallback
    assert "gfx950" in info["name"]
    return cct_hip


def _get(key):
    from cct_hip import _ffi
    v = C.c_int(0)
    _ffi.check(_ffi.lib().cct_get_option(key.encode(), C.byref(v)))
    return v.value


class options:
    """set library options for a block and put the old values back"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from cct_hip import _ffi
        self.old = {k: _get(k) for k in self.kw}
        for k, v in self.kw.items():
            _ffi.check(_ffi.lib().cct_set_option(k.encode(), v))
            assert _get(k) == v, f"the library does not accept {k} = {v}"

    def __exit__(self, *exc):
        from cct_hip import _ffi
        for k, v in self.old.items():
            _ffi.check(_ffi.lib().cct_set_option(k.encode(), v))


def decode(files, bs, out_dev=None):
    """cct_decode_batch on files of one shape -> (return code, status per file, rasters (n, N) or None with out_dev)"""
    from cct_hip import _ffi
    n = len(files)
    W, H = (files[0][4] << 8) | files[0][5], (files[0][6] << 8) | files[0][7]
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(f) for f in files], out=offs[1:])
    blob = b"".join(files)
    status = np.full(n, 0xDEAD, dtype=np.uint32)
    if out_dev is not None:
        rc = _ffi.lib().cct_decode_batch(blob, offs.ctypes.data, n, bs, MAGIC, out_dev.ptr, 1, out_dev.nbytes // 2, status.ctypes.data)
        return rc, status, None
    out = np.empty((n, W * H), dtype=np.uint16)
    rc = _ffi.lib().cct_decode_batch(blob, offs.ctypes.data, n, bs, MAGIC, out.ctypes.data, 0, out.size, status.ctypes.data)
    return rc, status, out


def decode_chunked(files, bs, max_px=1 << 25):
    """the same in calls of at most max_px pixels -> (status, [raster or None])"""
    W, H = (files[0][4] << 8) | files[0][5], (files[0][6] << 8) | files[0][7]
    step = max(1, max_px // (W * H))
    status, rasters = [], []
    for i in range(0, len(files), step):
        rc, st, out = decode(files[i:i + step], bs)
        bad = [int(s) for s in st if s]
        assert rc == (bad[0] if bad else 0), "the return value is the first status that is not OK"
        status += [int(s) for s in st]
        rasters += [out[k].tobytes() for k in range(len(st))]
    return status, rasters


# ------------------------------------------------------------------------------------- a. well-formed streams, every kernel variant

def _check_exact(case, opts, deflate):
    W, H, bs, fr, plan = case
    blob, img, info = ts.well_formed(case)
    f = ts.with_deflate(blob) if deflate else blob
    with options(**opts):
        rc, st, out = decode([f], bs)
    assert (rc, int(st[0])) == (0, 0), (case, opts, deflate, rc, st)
    got = out[0].reshape(W, H)
    if not np.array_equal(got, img):
        bad = np.flatnonzero(got.ravel() != img.ravel())
        pytest.fail(f"{case} {opts} deflate={deflate}: {len(bad)} wrong pixels, first at {bad[:5]}: "
                    f"{got.ravel()[bad[:5]]} instead of {img.ravel()[bad[:5]]}")


@pytest.mark.parametrize("case", ts.WELL_FORMED, ids=lambda c: f"{c[0]}x{c[1]}-bs{c[2]}-{'fractal' if c[3] else 'raster'}-{c[4]}")
def test_well_formed_streams_decode_exactly(hip, case):
    """device raster == the writer's image, raw and behind DEFLATE (device INFLATE on), with the precondition that makes
    the row the kernel variant it is meant to be"""
    W, H, bs, fr, plan = case
    blob, img, info = ts.well_formed(case)
    NB = info["NB"]
    assert _get("device_inflate") == 1
    assert len(blob) - 13 <= hip.batch.payload_stride(W, H, bs)
    variants = [dict()]
    if (W, H, bs) == (512, 512, 16):
        variants = [dict(tile_path=t, wg_threads=wg) for t in (1, 0) for wg in WG_THREADS] + [dict(runtime_block_size=1)]
        if plan in ("near", "far", "rand", "p50", "half"):
            assert info["n_jump"] > 2048  # DEC_JLIST_CAP: the jump list of the compiled kernel spills into the HBM workspace
        if plan == "half":
            assert info["n_jump"] == NB // 2 == 8192  # every slot a pair
    if (W, H, bs) == (1024, 1024, 4):
        assert NB == 262144 and 5 * NB > 100 * 1024  # role and slot tables in HBM
    for opts in variants:
        for deflate in (False, True):
            _check_exact(case, opts, deflate)
        want_path = 1 if (opts.get("runtime_block_size") or bs not in (4, 8, 16, 32, 64)) else 0
        assert _get("last_decode_path") == want_path, (case, opts)


def test_well_formed_set_reaches_both_ends_of_16_bits(hip):
    """values 0 and 65535 occur in the images that the test above compares"""
    imgs = [ts.well_formed(c)[1] for c in ts.WELL_FORMED if c[:3] in ((64, 64, 16), (512, 512, 16))]
    assert min(int(i.min()) for i in imgs) == 0 and max(int(i.max()) for i in imgs) == 65535


# ------------------------------------------------------------------------------------- b. the 16-bit edge

def _edge_cases(W, H, bs, plan="p50"):
    """[(label, file, image or None)]: the running value touches 0 / 65535 (decodes) or leaves by one (overflow) at the first
    pixel, the last pixel, inside a pair, and in the token just before / just after (and, for a full token, across) the
    segment boundary and a step boundary of every workgroup size, by a short and by a full token"""
    N = W * H
    slots = ts.layout(N // bs, plan, np.random.default_rng(11))
    _, start = ts.stream_positions(slots, bs)
    pair_k = next(int(s0) + 5 for (lead, j), s0 in zip(slots, start) if j and s0 > 64)
    out = []
    for target in (0, -1, 65535, 65536):
        for kind in (ts.SHORT, ts.FULL):
            places = [("last", dict(k=N - 1)), ("pair", dict(k=pair_k))]
            if target <= 0:
                places.append(("first", dict(k=0)))
            for b in ts.boundaries_for(WG_THREADS):
                if b + 8 >= N:
                    continue  # the payload of this shape ends before that step boundary
                if b == ts.SEG and target > 0:
                    continue  # the ramp to the upper edge is still under way at offset 16
                places += [(f"off{b - 2}", dict(k=None, at_offset=b - 2)), (f"off{b - 1}", dict(k=None, at_offset=b - 1)),
                           (f"off{b}", dict(k=None, at_offset=b))]
            for name, kw in places:
                k0 = kw.pop("k")
                got = next(filter(None, (ts.edge_stream(W, H, bs, True, plan, np.random.default_rng(seed), k0, target, kind, **kw)
                                         for seed in (11, 12, 13, 14))))  # 11 unless a jump byte of that layout stands at at_offset
                f, img, k = got
                tok = "short" if kind == ts.SHORT else "full"
                out.append((f"{W}x{H}/{bs} value {target} by {tok} token at {name} (pixel {k})", f, img))
    return out


@pytest.mark.parametrize("shape", [(256, 256, 16), (128, 128, 4), (96, 65, 5)], ids=lambda s: f"{s[0]}x{s[1]}-bs{s[2]}")
def test_sixteen_bit_edge(hip, shape):
    """0 and 65535 decode; -1 and 65536 are CCT_E_OVERFLOW, as the oracle says, wherever in the stream the one pixel stands
    (both pass-B loops: block size 16 and block sizes below 16; the run-time block size kernel)"""
    from cct_hip import _ffi
    W, H, bs = shape
    cases = _edge_cases(W, H, bs)
    for label, f, img in cases:  # the preconditions: what the oracle says about these files
        verdict, raster = ts.oracle_verdict(f, bs)
        assert verdict == ("pixels" if img is not None else "overflow"), label
        assert img is None or raster == img.tobytes(), label
        assert ts.classify_fast(f[13:], W * H, bs) is None, label
    wrong = []
    for wg in WG_THREADS:
        with options(wg_threads=wg):
            status, rasters = decode_chunked([f for _, f, _ in cases], bs)
        for (label, f, img), st, ras in zip(cases, status, rasters):
            want = 0 if img is not None else _ffi.E_OVERFLOW
            if st != want or (img is not None and ras != img.tobytes()):
                wrong.append(f"wg_threads {wg}: {label}: status {st} instead of {want}"
                             + ("" if st != 0 or img is None else ", wrong raster"))
    assert not wrong, f"{len(wrong)} of {3 * len(cases)}:\n" + "\n".join(wrong[:20])


def test_overflow_is_kept_when_the_sum_wraps_32_bits(hip):
    """1024x1024 pixels of +2048 each: the running value leaves 16 bits at pixel 32 and the sum of all deltas is 2^31,
    which wraps a 32-bit prefix sum back to where in-range values live: still CCT_E_OVERFLOW, as the oracle says"""
    from cct_hip import _ffi
    W = H = 1024
    f = ts.header(W, H, 16, True) + bytes([0xE8, 0x00]) * (W * H) + b"\x3b"
    assert (W * H * 2048) % (1 << 32) == 1 << 31
    assert ts.oracle_verdict(f, 16)[0] == "overflow" and ts.classify_fast(f[13:], W * H, 16) is None
    # the same with the wrap landing exactly on 0: 2^21 pixels would be needed, so wrap downwards instead: -2047 each
    g = ts.header(W, H, 16, True) + bytes([0xE8, 0x01]) * (W * H) + b"\x3b"
    assert ts.oracle_verdict(g, 16)[0] == "overflow"
    for wg in WG_THREADS:
        with options(wg_threads=wg):
            rc, st, _ = decode([f, g], 16)
        assert rc == _ffi.E_OVERFLOW and [int(s) for s in st] == [_ffi.E_OVERFLOW] * 2, (wg, rc, st)


# ------------------------------------------------------------------------------------- c. damaged streams

def _expected(files, W, H, bs):
    """[(judge's verdict, oracle's verdict, oracle's raster or None, status the device owes)]"""
    from cct_hip import _ffi
    out = []
    for name, tag, f, base in files:
        c = ts.classify_fast(f[13:], W * H, bs, base)
        o, ras = ts.oracle_verdict(f, bs)
        assert not (c is None and o == "stream"), (name, tag)  # (tests/test_token_streams_host.py holds this too)
        out.append((c, o, ras, _ffi.E_STREAM if c else _ffi.E_OVERFLOW if o == "overflow" else 0))
    return out


def _disagreements(files, expected, status, rasters, note):
    out = []
    for (name, tag, f, _), (c, o, ras, want), st, got in zip(files, expected, status, rasters):
        if st != want:
            out.append(f"{note} {tag} {name}: judge {c}, oracle {o}: status {st} instead of {want}")
        elif want == 0 and got != ras:
            out.append(f"{note} {tag} {name}: judge {c}, oracle {o}: status 0 but not the oracle's raster")
    return out


@pytest.mark.parametrize("shape", ts.DAMAGED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-bs{s[2]}")
def test_damaged_streams(hip, shape):
    """every damaged file of the shape in as few calls as possible, under every workgroup size (the aimed edits sit on the step
    boundaries of each): decoded exactly, CCT_E_OVERFLOW or CCT_E_STREAM as the rule in this file's header says"""
    W, H, bs = shape
    files = ts.damaged_set(W, H, bs, WG_THREADS)
    stride = hip.batch.payload_stride(W, H, bs)
    assert all(len(f) - 13 <= stride for _, _, f, _ in files)
    expected = _expected(files, W, H, bs)
    assert collections.Counter(e[3] for e in expected)[0] > len(files) // 10
    wrong = []
    for wg in WG_THREADS:
        with options(wg_threads=wg):
            status, rasters = decode_chunked([f for _, _, f, _ in files], bs)
        wrong += _disagreements(files, expected, status, rasters, f"wg_threads {wg}")
        if (W, H) == (512, 512) and wg == 1024:
            with options(tile_path=0):
                status, rasters = decode_chunked([f for _, _, f, _ in files], bs)
            wrong += _disagreements(files, expected, status, rasters, "tile_path 0")
    if W * H == 4096:  # the same files behind DEFLATE, through the device INFLATE
        zfiles = [f[:12] + b"\x01" + zlib.compress(f[13:], 1) for _, _, f, _ in files]
        status, rasters = decode_chunked(zfiles, bs)
        wrong += _disagreements(files, expected, status, rasters, "behind DEFLATE")
    assert not wrong, f"{len(wrong)} disagreements:\n" + "\n".join(wrong[:30])


def test_jump_bytes_behind_the_last_pixel_do_not_exist(hip):
    """Named case: a well-formed stream followed by jump bytes.  The decoder reads N pixels and nothing behind them, so the
    file decodes -- also when the jump list of an earlier slice in the same call left records behind, and when two of those
    jump bytes stand next to each other."""
    W, H, bs = 64, 64, 16
    files, imgs = [], []
    for k, plan in enumerate(("none", "far", "none", "near", "jump63", "rand", "p50")):
        blob, img, _ = ts.well_formed((W, H, bs, True, plan))
        # a few tokens with jump bytes among them; or 40 jump bytes: two in a row, in segments that hold no pixel token at all
        tail = bytes([0x81, 0xBF, 0x80, 0x01, 0x82]) if k < 5 else bytes([0x81, 0x82] * 20)
        files.append(blob[:-1] + tail + b"\x3b")
        imgs.append(img)
        assert ts.classify(files[-1][13:], W * H, bs) is None and ts.oracle_verdict(files[-1], bs)[1] == img.tobytes()
    for _ in range(3):
        rc, st, out = decode(files, bs)
        assert rc == 0 and not st.any(), (rc, st)
        for k, img in enumerate(imgs):
            assert out[k].tobytes() == img.tobytes(), k


# ------------------------------------------------------------------------------------- d. a bad file and its neighbours

@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("shape", [(64, 64, 16), (512, 512, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_bad_file_does_not_reach_its_neighbours(hip, shape, slots):
    """Good files and files of every defect name in turn, decoded into a device buffer longer than n * N pixels and filled with
    a sentinel: every good file has status 0 and its exact raster, the tail behind n * N pixels keeps the sentinel, the call
    returns the first status that is not OK, and an all-good call right after, on the same decode slot, is exact (the
    workspaces carry nothing over).  What a refused file's own raster holds is unspecified and not looked at."""
    from cct_hip import _ffi
    from cct_hip.batch import DeviceBuffer
    W, H, bs = shape
    N = W * H
    good = [ts.well_formed((W, H, bs, True, plan))[:2] for plan in ts.PLANS]
    dam = ts.damaged_set(W, H, bs, WG_THREADS)
    exp = {}
    for name, tag, f, base in dam[: 400 if N > 4096 else len(dam)]:
        c = ts.classify_fast(f[13:], N, bs, base)
        key = c or ("overflow" if ts.oracle_verdict(f, bs)[0] == "overflow" else None)
        if key and key not in exp:
            exp[key] = (f, _ffi.E_STREAM if c else _ffi.E_OVERFLOW)
    assert set(exp) == set(ts.DEFECTS) | {"overflow"}
    bad = [exp[k] for k in sorted(exp)]
    tail = 4096

    def run(files, want_status, images):
        n = len(files)
        buf = DeviceBuffer(2 * (n * N + tail))
        buf.upload(np.full(n * N + tail, 0xA5C3, np.uint16))
        rc, st, _ = decode(files, bs, out_dev=buf)
        got = buf.download(np.uint16, n * N + tail)
        buf.free()
        assert [int(s) for s in st] == want_status, (st, want_status)
        assert rc == next((s for s in want_status if s), 0)
        assert (got[n * N:] == 0xA5C3).all(), "the memory behind the output was written"
        for k, img in enumerate(images):
            if img is not None:
                assert got[k * N:(k + 1) * N].tobytes() == img.tobytes(), f"file {k} (good) has a wrong raster"

    with options(decode_slots=slots):
        # raw: good, bad, good, bad, ...
        files, want, images = [], [], []
        for k, (f, st) in enumerate(bad):
            files += [good[k % len(good)][0], f]
            want += [0, st]
            images += [good[k % len(good)][1], None]
        files.append(good[-1][0]); want.append(0); images.append(good[-1][1])
        run(files, want, images)
        run([g[0] for g in good], [0] * len(good), [g[1] for g in good])
        # behind DEFLATE: a broken zlib stream, a wrong Adler-32 and the defects, between good files
        z = [ts.with_deflate(g[0]) for g in good]
        broken = z[1][:13] + b"\x00\x01\x02" + z[1][16:]
        adler = z[2][:-1] + bytes([z[2][-1] ^ 0x55])
        files = [z[0], broken, z[1], adler, z[2]]
        want = [0, _ffi.E_ZLIB, 0, _ffi.E_ZLIB, 0]
        images = [good[0][1], None, good[1][1], None, good[2][1]]
        for k, (f, st) in enumerate(bad):
            files += [ts.with_deflate(f), z[3 + k % 4]]
            want += [st, 0]
            images += [None, good[3 + k % 4][1]]
        run(files, want, images)
        run(z, [0] * len(z), [g[1] for g in good])
