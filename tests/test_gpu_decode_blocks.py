"""The block path of the decode kernel (csrc/decode_kernels.hip, decode_kernel<16, true, true>): pass B stages a step's pixel
values by ordinal and places whole 4x4 blocks, a slot that straddles two steps by the later one.  Every test decodes the
same files under tile_path 1 (the block path) and tile_path 0 (the traversal table, one store per pixel) and holds both to
the writer's image or the oracle; the read-only option last_decode_block_path says which of the two ran.

The shapes are the smallest ones whose traversal is made of 64x64 tiles: 128x64 and 64x128 (one tile orientation), 128x128
(three) and 256x256 (four).  The workload's own shape, 512x512, is covered by tests/test_gpu_token_streams.py.  The writer,
the judge and the rule per file are those of tests/token_streams.py and of the head of tests/test_gpu_token_streams.py."""
import numpy as np
import pytest

import token_streams as ts
from test_gpu_token_streams import WG_THREADS, _disagreements, _expected, _get, decode, decode_chunked, options

pytestmark = pytest.mark.gpu

BS = 16
TILED_SHAPES = [(128, 64), (64, 128), (128, 128), (256, 256)]
STEP = 256 * ts.SEG  # payload bytes of a step at 256 lanes; the steps of 512 and 1024 lanes begin on multiples of it
_streams = {}


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    info = cct_hip.device_info()  # raises if the extension or the GPU is missing: no fallback
    assert "gfx950" in info["name"]
    return cct_hip


def stream(W, H, plan):
    """(file, image, info) of one shape and plan, built once"""
    key = (W, H, plan)
    if key not in _streams:
        rng = np.random.default_rng([W, H, BS, 5, ts.PLANS.index(plan)])
        _streams[key] = ts.build(W, H, BS, True, plan, rng, bias=0.5 if plan == "far" else 0.0, return_info=True)
    return _streams[key]


def borders_inside_slots(blob, info, step=STEP):
    """[(payload offset of a step border, pixel ordinal there, the slot it falls into is a pair)] for the borders that fall
    strictly inside a slot: the first pixel token of the step is not the first of a slot"""
    off, isj, _ = ts.token_table(blob[13:])
    pix_off = off[~isj]
    _, start = ts.stream_positions(info["slots"], BS)
    out = []
    for b in range(step, len(blob) - 13 - 1, step):
        ordinal = int(np.searchsorted(pix_off, b))  # pixel tokens that start before the border
        if ordinal % BS:
            slot = int(np.searchsorted(start, ordinal, side="right")) - 1
            out.append((b, ordinal, bool(info["slots"][slot][1])))
    return out


def both_paths(files, wg, want_rasters=None, note=""):
    """decode under tile_path 1 and 0 -> (status, rasters) of the block path; both paths must agree on every status, on every
    raster whose status is 0, and must report which of them ran"""
    res = {}
    for path in (1, 0):
        status, rasters = [None] * len(files), [None] * len(files)
        for flag in sorted({f[12] for f in files}):  # a call takes raw files or files behind DEFLATE, not both
            idx = [k for k, f in enumerate(files) if f[12] == flag]
            with options(tile_path=path, wg_threads=wg):
                st, ras = decode_chunked([files[k] for k in idx], BS)
                assert _get("last_decode_block_path") == path, (note, wg, path)
            for k, s, r in zip(idx, st, ras):
                status[k], rasters[k] = s, r
        res[path] = (status, rasters)
    (st1, ras1), (st0, ras0) = res[1], res[0]
    assert st1 == st0, (note, wg, [(k, a, b) for k, (a, b) in enumerate(zip(st1, st0)) if a != b][:10])
    for k, st in enumerate(st1):
        if st == 0:
            assert ras1[k] == ras0[k], f"{note} wg_threads {wg}: file {k} differs between the block path and the traversal table"
            if want_rasters is not None and want_rasters[k] is not None:
                assert ras1[k] == want_rasters[k], f"{note} wg_threads {wg}: file {k} is not the expected raster"
    return st1, ras1


# ------------------------------------------------------------------------------------- exactness

@pytest.mark.parametrize("shape", TILED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_step_borders_fall_inside_single_and_pair_slots(shape):
    """host precondition of the test below: every payload spans at least three steps at 256 lanes, and among the plans of
    a shape a step border falls strictly inside a single slot and one inside a pair slot"""
    W, H = shape
    inside = []
    for plan in ts.PLANS:
        blob, _, info = stream(W, H, plan)
        assert len(blob) - 13 - 1 > 2 * STEP, (shape, plan)
        inside += [(plan,) + x for x in borders_inside_slots(blob, info)]
    assert any(not pair for *_, pair in inside) and any(pair for *_, pair in inside), inside


@pytest.mark.parametrize("plan", ts.PLANS)
@pytest.mark.parametrize("shape", TILED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_block_path_decodes_exactly(hip, shape, plan):
    """raster of the block path == the writer's image == raster of the traversal-table path: every pairing plan, every
    workgroup size, raw and behind DEFLATE"""
    W, H = shape
    blob, img, info = stream(W, H, plan)
    assert len(blob) - 13 <= hip.batch.payload_stride(W, H, BS)
    files = [blob, ts.with_deflate(blob)]
    for wg in WG_THREADS:
        st, _ = both_paths(files, wg, [img.tobytes()] * 2, f"{shape} {plan}")
        assert st == [0, 0], (shape, plan, wg, st)


# ------------------------------------------------------------------------------------- step borders

def test_jump_byte_on_the_first_byte_of_a_step(hip):
    """a jump byte at payload offsets 16, 4096, 8192 and 16384: the pair's two slots are the first of a step of every
    workgroup size, and the slot before them ends with the step"""
    W = H = 128
    jump_at = ts.boundaries_for(WG_THREADS)
    files, want = [], []
    for plan, seed in (("p50", 1), ("none", 2), ("near", 3)):
        blob, img = ts.build(W, H, BS, True, plan, np.random.default_rng([W, H, 21, seed]), full_p=0.3, jump_at=jump_at)
        assert all((blob[13 + b] & 0xC0) == 0x80 for b in jump_at) and len(blob) - 13 > jump_at[-1] + 64
        files += [blob, ts.with_deflate(blob)]
        want += [img.tobytes()] * 2
    for wg in WG_THREADS:
        st, _ = both_paths(files, wg, want, "jump on a step border")
        assert not any(st), (wg, st)


def _edge_files(W, H):
    """[(label, file, image or None)]: the running value reaches 0 / 65535 (decodes) or -1 / 65536 (overflow) in a token that
    starts two bytes before, one byte before and on the first byte of a step of every workgroup size: a short token at
    b - 1 is the last pixel of a step, a full token at b - 2 too, a full token at b - 1 has its second byte in the next step,
    and a token at b is the first pixel of the next step"""
    out = []
    for target in (0, -1, 65535, 65536):
        for kind in (ts.SHORT, ts.FULL):
            for b in ts.boundaries_for(WG_THREADS)[1:]:
                for at in (b - 2, b - 1, b):
                    got = next(filter(None, (ts.edge_stream(W, H, BS, True, "p50", np.random.default_rng(seed), None, target, kind, at_offset=at)
                                             for seed in (31, 32, 33, 34, 35, 36))))
                    f, img, k = got
                    off, isj, isf = ts.token_table(f[13:])
                    t = int(np.searchsorted(off, at))
                    assert off[t] == at and not isj[t] and bool(isf[t]) == (kind == ts.FULL)  # the token does start there
                    out.append((f"value {target} by a {'short' if kind == ts.SHORT else 'full'} token at offset {at} (pixel {k})", f, img))
    return out


def test_values_at_the_step_border(hip):
    """0 and 65535 decode, -1 and 65536 are CCT_E_OVERFLOW on the last pixel of a step and on the first pixel of the next,
    also where the full token that carries the value straddles the border"""
    from cct_hip import _ffi
    W = H = 128
    cases = _edge_files(W, H)
    for label, f, img in cases:  # what the oracle and the judge say about these files
        verdict, raster = ts.oracle_verdict(f, BS)
        assert verdict == ("pixels" if img is not None else "overflow"), label
        assert img is None or raster == img.tobytes(), label
        assert ts.classify_fast(f[13:], W * H, BS) is None, label
    want = [0 if img is not None else _ffi.E_OVERFLOW for _, _, img in cases]
    for wg in WG_THREADS:
        st, _ = both_paths([f for _, f, _ in cases], wg, [None if img is None else img.tobytes() for _, _, img in cases], "16-bit edge")
        wrong = [f"{label}: status {s} instead of {w}" for (label, _, _), s, w in zip(cases, st, want) if s != w]
        assert not wrong, (wg, wrong[:10])


# ------------------------------------------------------------------------------------- damaged streams

def _damaged(W, H):
    """damaged files of one well-formed 128x128 base whose jump bytes stand on step borders:
    [(name, tag, file, Base)] as token_streams.damaged_set returns them"""
    N = W * H
    rng = np.random.default_rng([W, H, BS, 91])
    bounds = ts.boundaries_for(WG_THREADS)
    jump_at = [b - (k % 2) for k, b in enumerate(bounds)]
    blob, _ = ts.build(W, H, BS, True, "p50", rng, full_p=0.3, reserved_p=0.03, bias=0.2, jump_at=jump_at)
    base = ts.Base(blob[13:], N, BS)
    items = ts.damage(blob, N, BS, rng, n_flips=150, n_bytes=12, n_cuts=8, n_jump_edits=8, n_append=12, boundaries=bounds)
    return [(name, f"{W}x{H} #{k}", f, base) for k, (name, f) in enumerate(items)]


def test_damaged_streams_on_the_block_path(hip):
    """flips, cuts, jump edits, bytes appended behind pixel N - 1 and the edits aimed at the step borders: per file the status
    of the block path is the status of the traversal-table path and the one the rule owes; rasters where the status is 0.
    The files are decoded in one batch: a refused file sits between decodable ones"""
    W = H = 128
    files = _damaged(W, H)
    assert len(files) > 300
    expected = _expected(files, W, H, BS)
    kinds = {e[3] for e in expected}
    assert len(kinds) == 3 and sum(1 for e in expected if e[3] == 0) > len(files) // 10  # decodable, overflow and stream
    assert any(name == "append" and e[3] == 0 for (name, _, _, _), e in zip(files, expected))
    wrong = []
    for wg in WG_THREADS:
        st, ras = both_paths([f for _, _, f, _ in files], wg, None, "damaged")
        wrong += _disagreements(files, expected, st, ras, f"wg_threads {wg}")
    assert not wrong, f"{len(wrong)} disagreements:\n" + "\n".join(wrong[:30])


# ------------------------------------------------------------------------------------- output placement

def test_output_that_is_not_8_byte_aligned(hip):
    """rasters written 2 bytes behind an 8-byte boundary of a device buffer (the block path then stores pixel by pixel): exact,
    and the memory in front of and behind the rasters keeps its sentinel"""
    from cct_hip import _ffi
    from cct_hip.batch import DeviceBuffer
    W = H = 128
    N = W * H
    picks = [stream(W, H, plan) for plan in ("p50", "none", "half")]
    files = [p[0] for p in picks]
    n, tail = len(files), 4096
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(f) for f in files], out=offs[1:])
    for wg in WG_THREADS:
        for lead in (1, 4, 5):  # elements in front of the rasters: 2 bytes off, aligned, 2 bytes off the other way round
            buf = DeviceBuffer(2 * (lead + n * N + tail))
            assert buf.ptr % 8 == 0
            buf.upload(np.full(lead + n * N + tail, 0xA5C3, np.uint16))
            status = np.full(n, 0xDEAD, dtype=np.uint32)
            with options(tile_path=1, wg_threads=wg):
                rc = _ffi.lib().cct_decode_batch(b"".join(files), offs.ctypes.data, n, BS, b"pact", buf.ptr + 2 * lead, 1, n * N,
                                                 status.ctypes.data)
                assert _get("last_decode_block_path") == 1
            got = buf.download(np.uint16, lead + n * N + tail)
            buf.free()
            assert rc == 0 and not status.any(), (wg, lead, rc, status)
            assert (got[:lead] == 0xA5C3).all() and (got[lead + n * N:] == 0xA5C3).all(), "memory outside the rasters was written"
            for k, (_, img, _) in enumerate(picks):
                assert got[lead + k * N: lead + (k + 1) * N].tobytes() == img.tobytes(), (wg, lead, k)


# ------------------------------------------------------------------------------------- fallback

@pytest.mark.parametrize("shape", [(64, 64), (192, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_without_tiles_take_the_traversal_table(hip, shape):
    """a shape whose traversal is not made of 64x64 tiles decodes exactly and reports that the block path did not run"""
    W, H = shape
    for plan in ("p50", "far"):
        blob, img, _ = stream(W, H, plan)
        for wg in WG_THREADS:
            for f in (blob, ts.with_deflate(blob)):
                with options(tile_path=1, wg_threads=wg):
                    rc, st, out = decode([f, f], BS)
                    assert _get("last_decode_block_path") == 0
                assert rc == 0 and not st.any(), (shape, plan, wg, rc, st)
                assert out[0].tobytes() == img.tobytes() and out[1].tobytes() == img.tobytes(), (shape, plan, wg)
