"""Device DICOM RLE Lossless codec (cct_dicom_rle_encode_batch / _decode_batch) against tests/dicom_rle_model.py: frames
byte for byte, rasters from the device's, the model's and libtiff's frames, hand-built segments, packet heads on every
offset of a decoder tile, the lenient rules and the one refusal over several tiles and across a batch of the tile chain,
per-frame refusals, and the RLE column of tools/evaluate.py."""
import functools
import importlib.util
import os
import struct

import numpy as np
import pytest

import dicom_rle_model as m

pytestmark = pytest.mark.gpu

E_STREAM = 4
TILE = 2048  # csrc/cct_internal.h RLE_TILE


@functools.lru_cache(maxsize=None)
def cases(bits):
    """[(rows, cols, names, rasters (n, rows, cols), model frames)] over ROWS x COLS, computed once"""
    out = []
    for rows in m.ROWS:
        for cols in m.COLS:
            c = m.raster_cases(rows, cols, bits)
            out.append((rows, cols, list(c), np.stack(list(c.values())), [m.encode_frame(x) for x in c.values()]))
    return out


@functools.lru_cache(maxsize=None)
def phantoms():
    from cct_hip.synth import ct_phantom
    imgs = np.stack([ct_phantom(seed, n=128) for seed in range(4)]).astype(np.uint16)
    return imgs, [m.encode_frame(x) for x in imgs]


@pytest.mark.parametrize("bits", [8, 16])
def test_encode_equals_the_model(bits):
    import cct_hip
    odd = even = 0
    for rows, cols, names, imgs, want in cases(bits):
        got = cct_hip.dicom_rle_encode_batch(imgs)  # one mixed batch per shape
        for name, g, w in zip(names, got, want):
            assert g == w, (rows, cols, name)
        for img in imgs:
            seg = sum(len(m.encode_row(r.tobytes())) for r in m.planes_of(img)[0])
            odd += seg & 1
            even += 1 - (seg & 1)
    assert odd and even  # padded and unpadded segments both occurred


def test_encode_phantoms_from_host_and_device():
    import cct_hip
    imgs, want = phantoms()
    assert cct_hip.dicom_rle_encode_batch(imgs) == want
    d = cct_hip.DeviceBuffer.from_numpy(imgs)
    try:
        assert cct_hip.dicom_rle_encode_batch(d, shape=imgs.shape) == want
        assert cct_hip.dicom_rle_encode_batch(d, shape=imgs.shape[1:]) == want[:1]
    finally:
        d.free()
    low = (imgs & 0xFF).astype(np.uint8)
    assert cct_hip.dicom_rle_encode_batch(low) == [m.encode_frame(x) for x in low]


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("source", ["device", "model", "libtiff"])
def test_decode_returns_the_rasters(bits, source):
    import cct_hip
    if source == "libtiff" and not m.have_libtiff():
        pytest.skip("Pillow without libtiff: no second PackBits encoder")
    for rows, cols, names, imgs, model_frames in cases(bits):
        if source == "device":
            frames = cct_hip.dicom_rle_encode_batch(imgs)
        elif source == "model":
            frames = model_frames
        else:
            frames = [m.libtiff_frame(x) for x in imgs]
        back = cct_hip.dicom_rle_decode_batch(frames, rows, cols, bits=bits)
        assert back.dtype == imgs.dtype and back.shape == imgs.shape
        for name, b, x in zip(names, back, imgs):
            assert np.array_equal(b, x), (rows, cols, name)


def test_decode_phantoms_to_host_and_device():
    import cct_hip
    imgs, frames = phantoms()
    assert np.array_equal(cct_hip.dicom_rle_decode_batch(frames, 128, 128), imgs)
    d = cct_hip.DeviceBuffer(imgs.nbytes)
    try:
        assert cct_hip.dicom_rle_decode_batch(frames, 128, 128, out_dev=d) == imgs.shape
        assert np.array_equal(d.download(np.uint16, imgs.size).reshape(imgs.shape), imgs)
    finally:
        d.free()
    if m.have_libtiff():
        assert np.array_equal(cct_hip.dicom_rle_decode_batch([m.libtiff_frame(x) for x in imgs], 128, 128), imgs)


def frame8(seg):
    """an 8-bit frame around one segment, no pad byte added"""
    return struct.pack("<16I", 1, 64, *([0] * 14)) + bytes(seg)


def test_decode_hand_built_segments():
    import cct_hip
    rows, cols = 4, 10
    want = np.arange(1, 41, dtype=np.uint8)
    lit = lambda a, b: bytes([b - a - 1]) + want[a:b].tobytes()  # noqa: E731
    runs = np.repeat(np.array([3, 4, 5], np.uint8), [15, 15, 10])
    segs = {
        "noops": (bytes([128, 128]) + lit(0, 20) + bytes([128]) + lit(20, 40) + bytes([128, 128]), want),
        "literals_cross_rows": (lit(0, 15) + lit(15, 33) + lit(33, 40), want),
        "runs_cross_rows": (bytes([257 - 15, 3, 257 - 15, 4, 257 - 10, 5]), runs),
        "pad_and_spare": (lit(0, 40) + bytes([0, 9, 8, 7, 200, 1, 128]), want),
        "run_longer_than_the_plane": (lit(0, 30) + bytes([257 - 100, 6]), np.concatenate([want[:30], np.full(10, 6, np.uint8)])),
        "literal_cut_at_completion": (lit(0, 30) + bytes([19]) + want[30:40].tobytes(), want),
    }
    frames = [frame8(s) for s, _ in segs.values()]
    for (name, (_, w)), f in zip(segs.items(), frames):
        assert np.array_equal(m.decode_frame(f, rows, cols, 8).ravel(), w), name  # the model agrees with the expectation
    back = cct_hip.dicom_rle_decode_batch(frames, rows, cols, bits=8)
    for (name, (_, w)), b in zip(segs.items(), back):
        assert np.array_equal(b.ravel(), w), name
    # 16 bits: the high segment is a literal cut by the next segment's offset exactly at completion
    hi, lo = want, want[::-1].copy()
    seg0 = lit(0, 30) + bytes([19]) + hi[30:40].tobytes()  # 42 bytes
    seg1 = bytes([39]) + lo.tobytes()
    f16 = struct.pack("<16I", 2, 64, 64 + len(seg0), *([0] * 13)) + seg0 + seg1
    img = (hi.astype(np.uint16) << 8 | lo).reshape(rows, cols)
    assert np.array_equal(m.decode_frame(f16, rows, cols, 16), img)
    assert np.array_equal(cct_hip.dicom_rle_decode_batch([f16], rows, cols)[0], img)


def test_decode_packet_heads_on_every_tile_offset():
    """Segments several tiles long made of 129-byte literal packets behind a prefix of 0 .. 128 packet bytes: the heads land
    on every offset of a tile.  A second family puts a replicate header on the last byte of the first tile."""
    import cct_hip
    rows, cols = 49, 128
    N = rows * cols
    rng = np.random.default_rng(5)

    def prefix(s):  # s bytes of packets
        return b"" if s == 0 else bytes([128]) if s == 1 else bytes([s - 2]) + rng.integers(0, 256, s - 1, dtype=np.uint8).tobytes()

    def literals(k):
        return b"".join(bytes([127]) + rng.integers(0, 256, 128, dtype=np.uint8).tobytes() for _ in range(k))

    frames = []
    for s in range(129):
        frames.append(frame8(prefix(s) + literals(49)))
        head = prefix(s) + literals(14)  # s + 1806 bytes
        gap = TILE - 1 - len(head)       # 113 .. 241 bytes up to the last byte of the tile
        assert gap >= 2
        head += prefix(min(gap, 129))
        if gap > 129:
            head += prefix(gap - 129)
        assert len(head) == TILE - 1
        frames.append(frame8(head + bytes([257 - 100, 0x5A]) + literals(49)))
    assert all(len(f) > 64 + 3 * TILE for f in frames)
    want = np.stack([m.decode_frame(f, rows, cols, 8) for f in frames])
    back = cct_hip.dicom_rle_decode_batch(frames, rows, cols, bits=8)
    bad = [i for i in range(len(frames)) if not np.array_equal(back[i], want[i])]
    assert not bad, bad


def test_decode_refusals_leave_the_rest_alone():
    import cct_hip
    from cct_hip import _ffi
    rows, cols = 5, 37
    N = rows * cols
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 4, (4, rows, cols)).astype(np.uint16) * 0x0101
    good = [m.encode_frame(x) for x in imgs]
    hi, lo = m.planes_of(imgs[0])
    short = m.frame_of_segments([m.encode_row(hi.tobytes()), m.encode_row(lo.tobytes()[:-1])])  # the low segment one byte short
    g = good[1]
    seg1 = struct.unpack("<I", g[8:12])[0]
    patch = lambda at, v: g[:at] + struct.pack("<I", v) + g[at + 4:]  # noqa: E731
    batch = [good[0], short, good[1], patch(0, 1), patch(4, 60), good[2], patch(8, 40), patch(8, len(g) + 10), g[:10], good[3]]
    bad_at = [1, 3, 4, 6, 7, 8]
    assert seg1 > 64
    for i, f in enumerate(batch):
        if i in bad_at:
            with pytest.raises(ValueError):
                m.decode_frame(f, rows, cols, 16)
    n = len(batch)
    sentinel = np.full((n + 1, rows, cols), 0xA5A5, np.uint16)
    d = cct_hip.DeviceBuffer.from_numpy(sentinel)
    try:
        shape, status = cct_hip.dicom_rle_decode_batch(batch, rows, cols, out_dev=d, raise_errors=False)
        assert shape == (n, rows, cols)
        assert list(status) == [E_STREAM if i in bad_at else 0 for i in range(n)]
        got = d.download(np.uint16, sentinel.size).reshape(sentinel.shape)
    finally:
        d.free()
    for i, k in ((0, 0), (2, 1), (5, 2), (9, 3)):
        assert np.array_equal(got[i], imgs[k]), i
    assert (got[n] == 0xA5A5).all()  # the slot behind the batch
    for i in (3, 4, 6, 7, 8):
        assert (got[i] == 0xA5A5).all(), i  # refused by the header walk: never sent to the device
    res, status = cct_hip.dicom_rle_decode_batch(batch, rows, cols, raise_errors=False)
    assert list(status) == [E_STREAM if i in bad_at else 0 for i in range(n)]
    for i, k in ((0, 0), (2, 1), (5, 2), (9, 3)):
        assert np.array_equal(res[i], imgs[k]), i
    with pytest.raises(_ffi.CorruptStreamError):
        cct_hip.dicom_rle_decode_batch(batch, rows, cols)
    with pytest.raises(_ffi.CorruptStreamError):
        cct_hip.dicom_rle_decode_batch([g[:10]], rows, cols)


# ---- lenient semantics and refusals beyond one tile and one chain batch ---------------------------------------------------

def packets_prefix(s, rng):
    """s bytes of packets: nothing, a no-op, or one literal"""
    return b"" if s == 0 else bytes([128]) if s == 1 else bytes([s - 2]) + rng.integers(0, 256, s - 1, dtype=np.uint8).tobytes()


def literal(n, rng):
    """a literal packet of n bytes whose data never reads as a no-op head"""
    return bytes([n - 1]) + rng.integers(0, 128, n, dtype=np.uint8).tobytes()


def verdict(frame, rows, cols, bits):
    """dicom_rle_model.decode_frame: the raster, or None for a ValueError (CCT_E_STREAM)"""
    try:
        return m.decode_frame(frame, rows, cols, bits)
    except ValueError:
        return None


@functools.lru_cache(maxsize=None)
def several_tiles():
    """name -> (frame, raster or None) at 49 x 128, 8 bits: segments of more than 3 tiles of 129-byte literal packets"""
    rows, cols = 49, 128
    N = rows * cols
    rng = np.random.default_rng(31)
    full = [literal(128, rng) for _ in range(49)]
    good = b"".join(full)
    assert len(good) == 49 * 129 > 3 * TILE
    segs = {"undamaged": good}
    # 47 full packets, one of 100, a full one, and a last that claims 101 bytes: 28 complete the plane
    head = b"".join(full[:47]) + literal(100, rng) + full[47]
    tail = literal(101, rng)
    assert len(head) > 3 * TILE and 47 * 128 + 100 + 128 + 28 == N
    segs["literal_cut_at_completion"] = head + tail[:1 + 28]
    segs["literal_cut_one_byte_before_completion"] = head + tail[:1 + 27]
    # a replicate header as the last byte of the segment gives nothing
    head = b"".join(full[:48]) + literal(126, rng)
    segs["replicate_header_without_value"] = head + bytes([255])
    segs["replicate_header_with_value"] = head + bytes([255, 9])
    segs["replicate_header_behind_a_complete_plane"] = good + bytes([200])
    # 4095 bytes that give N - 50, then a run of 100 whose header is the last byte of tile 1 and whose value opens tile 2
    parts = []
    for k in range(30):
        parts.append(full[k])
        if k < 19:
            parts.append(bytes([257 - (128 if k < 18 else 78), 40 + k]))
        parts.append(bytes([128]) * (7 if k < 7 else 6))
    head = b"".join(parts)
    assert len(head) == 2 * TILE - 1 and 30 * 128 + 18 * 128 + 78 == N - 50
    segs["run_past_the_plane_from_the_last_byte_of_tile_1"] = head + bytes([257 - 100, 0x5A]) + full[30]
    # spare packets behind completion fill tile 4
    segs["a_spare_tile"] = good + b"".join(literal(128, rng) for _ in range(17))
    assert len(segs["a_spare_tile"]) > 4 * TILE + 129
    # one packet head changed: every later head moves, the plane comes out short, long or equal
    spare = good + literal(128, rng)
    for k in range(40):
        j = int(rng.integers(16, 49))  # heads 129 j: tiles 1 .. 3
        h = int(rng.choice([int(rng.integers(0, 127)), int(rng.integers(128, 256))]))
        sg = spare if k % 3 == 0 else good  # with and without a spare packet to make up for what the change loses
        assert TILE <= 129 * j < 4 * TILE and sg[129 * j] == 127
        segs[f"head_{j}_becomes_{h}{'_spare_packet' if k % 3 == 0 else ''}"] = sg[:129 * j] + bytes([h]) + sg[129 * j + 1:]
    return rows, cols, {name: (frame8(sg), verdict(frame8(sg), rows, cols, 8)) for name, sg in segs.items()}


def test_decode_lenient_over_several_tiles():
    import cct_hip
    rows, cols, cases_ = several_tiles()
    good = cases_["undamaged"][1]
    heads = [w for name, (_, w) in cases_.items() if name.startswith("head_")]
    assert sum(w is None for w in heads) >= 10 and sum(w is not None and not np.array_equal(w, good) for w in heads) >= 10
    for name in ("literal_cut_at_completion", "replicate_header_with_value", "replicate_header_behind_a_complete_plane",
                 "run_past_the_plane_from_the_last_byte_of_tile_1", "a_spare_tile"):
        assert cases_[name][1] is not None, name
    for name in ("literal_cut_one_byte_before_completion", "replicate_header_without_value"):
        assert cases_[name][1] is None, name
    assert (cases_["run_past_the_plane_from_the_last_byte_of_tile_1"][1].ravel()[-50:] == 0x5A).all()
    back, status = cct_hip.dicom_rle_decode_batch([f for f, _ in cases_.values()], rows, cols, bits=8, raise_errors=False)
    for (name, (_, w)), b, st in zip(cases_.items(), back, status):
        assert st == (E_STREAM if w is None else 0), name
        if w is not None:
            assert np.array_equal(b, w), name


CHAIN_ROWS, CHAIN_COLS = 256, 520
CHAIN_BATCH = 64  # csrc/dicom_rle_kernels.hip CHAIN_TILES


def chain_segment(s, rng):
    """A segment of more than 64 tiles that gives exactly 256 x 520 bytes: s bytes of packets, then 129-byte literals, every
    tile entered at another offset.  Behind the first whole literal whose head lies in tile 63, and in tile 64, sit a literal
    of 64 bytes and a no-op.  -> (segment, {63: (head of the whole literal, head of the short one), 64: ...})"""
    N = CHAIN_ROWS * CHAIN_COLS
    seg = bytearray(packets_prefix(s, rng))
    out, marks = max(s - 1, 0), {}
    while N - out > 128 + 64:
        tile = len(seg) // TILE
        seg += literal(128, rng)
        out += 128
        if tile in (CHAIN_BATCH - 1, CHAIN_BATCH) and tile not in marks:
            marks[tile] = (len(seg) - 129, len(seg))
            seg += literal(64, rng) + bytes([128])
            out += 64
    while out < N:
        n = min(128, N - out)
        seg += literal(n, rng)
        out += n
    assert sorted(marks) == [CHAIN_BATCH - 1, CHAIN_BATCH] and len(seg) > (CHAIN_BATCH + 1) * TILE
    return bytes(seg), marks


def chain_damages(seg, marks):
    """name -> segment: a whole literal made one byte shorter (its last byte becomes a no-op, the plane ends one byte short),
    and the 64-byte literal made one longer (it takes the no-op as data, the plane is complete one byte early)"""
    out = {"undamaged": seg}
    for tile, (whole, short) in marks.items():
        assert seg[whole] == 127 and seg[short] == 63 and seg[short + 65] == 128 and whole // TILE == tile
        out[f"one_byte_short_in_tile_{tile}"] = seg[:whole] + bytes([126]) + seg[whole + 1:whole + 128] + bytes([128]) + seg[whole + 129:]
        out[f"one_byte_long_in_tile_{tile}"] = seg[:short] + bytes([64]) + seg[short + 1:]
    return out


@functools.lru_cache(maxsize=None)
def chain_cases():
    """[(name, frame, bits, raster or None, name of its undamaged frame)]"""
    rng = np.random.default_rng(64)
    out, segs = [], {}
    for s in (0, 1, 64, 127, 128):
        seg, marks = chain_segment(s, rng)
        segs[s] = chain_damages(seg, marks)
        for name, sg in segs[s].items():
            out.append((f"prefix_{s}_{name}", frame8(sg), 8, f"prefix_{s}_undamaged"))
    for s, t in ((0, 127), (1, 64), (64, 0), (127, 128), (128, 1)):  # the high segment of odd length: the low one starts on an odd offset
        for name in ("undamaged", f"one_byte_short_in_tile_{CHAIN_BATCH}", f"one_byte_long_in_tile_{CHAIN_BATCH - 1}"):
            hi, lo = segs[s][name], segs[t]["undamaged"]
            if len(hi) % 2 == 0:
                hi += bytes([128])
            out.append((f"high_{s}_{name}_low_{t}", struct.pack("<16I", 2, 64, 64 + len(hi), *([0] * 13)) + hi + lo, 16, f"high_{s}_undamaged_low_{t}"))
    return [(name, f, bits, verdict(f, CHAIN_ROWS, CHAIN_COLS, bits), base) for name, f, bits, base in out]


@pytest.mark.parametrize("bits", [8, 16])
def test_decode_chain_batches_entered_off_zero(bits):
    import cct_hip
    mine = [c for c in chain_cases() if c[2] == bits]
    good = {c[0]: c[3] for c in mine if c[0] == c[4]}
    assert len(good) == 5
    for name, f, _, w, base in mine:
        assert (w is None) == ("short" in name), name
        if "long" in name:
            assert not np.array_equal(w, good[base]), name
    back, status = cct_hip.dicom_rle_decode_batch([c[1] for c in mine], CHAIN_ROWS, CHAIN_COLS, bits=bits, raise_errors=False)
    for (name, _, _, w, _), b, st in zip(mine, back, status):
        assert st == (E_STREAM if w is None else 0), name
        if w is not None:
            assert np.array_equal(b, w), name
    with pytest.raises(cct_hip._ffi.CorruptStreamError):
        cct_hip.dicom_rle_decode_batch([c[1] for c in mine], CHAIN_ROWS, CHAIN_COLS, bits=bits)
    assert np.array_equal(cct_hip.dicom_rle_decode_batch([c[1] for c in mine if c[3] is not None], CHAIN_ROWS, CHAIN_COLS, bits=bits),
                          np.stack([c[3] for c in mine if c[3] is not None]))


def test_decode_short_long_segments_leave_the_rest_alone():
    """segments of 66 tiles that end one byte short, between good frames, into a device buffer that holds a sentinel"""
    import cct_hip
    by_name = {c[0]: c for c in chain_cases() if c[2] == 8}
    order = ["prefix_0_undamaged", f"prefix_64_one_byte_short_in_tile_{CHAIN_BATCH - 1}", "prefix_127_undamaged",
             f"prefix_1_one_byte_short_in_tile_{CHAIN_BATCH}", f"prefix_128_one_byte_short_in_tile_{CHAIN_BATCH}", "prefix_1_undamaged"]
    batch = [by_name[k] for k in order]
    n = len(batch)
    sentinel = np.full((n + 1, CHAIN_ROWS, CHAIN_COLS), 0xA5, np.uint8)
    d = cct_hip.DeviceBuffer.from_numpy(sentinel)
    try:
        shape, status = cct_hip.dicom_rle_decode_batch([c[1] for c in batch], CHAIN_ROWS, CHAIN_COLS, bits=8, out_dev=d, raise_errors=False)
        got = d.download(np.uint8, sentinel.size).reshape(sentinel.shape)
    finally:
        d.free()
    assert shape == (n, CHAIN_ROWS, CHAIN_COLS)
    assert list(status) == [0, E_STREAM, 0, E_STREAM, E_STREAM, 0]
    for i, c in enumerate(batch):
        assert (c[3] is None) == (status[i] != 0)
        if c[3] is not None:
            assert np.array_equal(got[i], c[3]), c[0]
    assert (got[n] == 0xA5).all()  # the slot behind the batch


def test_evaluate_tool_fills_the_rle_column(tmp_path):
    from cct_hip.synth import ct_phantom
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("evaluate_tool", os.path.join(root, "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    imgs = [ct_phantom(seed, n=128).astype(np.uint16) for seed in (1, 2)]
    for k, img in enumerate(imgs):
        np.save(tmp_path / f"slice{k}.npy", img)
    out = tmp_path / "out.csv"
    assert tool.main([str(tmp_path), "--results", str(out), "--rle", "device"]) == 0
    lines = out.read_text().splitlines()
    head = lines[0].split(",")
    cells = [dict(zip(head, ln.split(","))) for ln in lines[1:]]
    assert len(cells) == 2
    for cell, img in zip(cells, imgs):
        assert int(cell["RLE"]) == len(m.encapsulate([m.encode_frame(img)]))
    assert tool.main([str(tmp_path), "--results", str(out)]) == 0
    assert [ln.split(",")[head.index("RLE")] for ln in out.read_text().splitlines()[1:]] == ["NA", "NA"]


PASS_BYTES = 512 << 20  # csrc/api_dicom_rle.cpp RLE_PASS_BYTES


def test_encode_in_two_passes_equals_single_frames():
    """9 uint8 rasters of 4096 x 8192: the device stride of a frame is 64 + 2 * 2^25 bytes rounded to words, so a pass takes 7
    of them and the batch runs as 7 + 2.  Single frames are pinned to the model at small shapes; here the batch is pinned
    to them on both sides of the pass border."""
    import cct_hip
    rows, cols, n = 4096, 8192, 9
    dstride = (cct_hip._ffi.lib().cct_dicom_rle_bound(rows, cols, 8) + 3) & ~3
    per_pass = PASS_BYTES // dstride
    assert per_pass == 7 and per_pass < n <= 2 * per_pass
    rng = np.random.default_rng(21)
    imgs = np.empty((n, rows, cols), np.uint8)
    for i in range(n):
        imgs[i] = 10 + i  # a constant plane and i + 1 rows of noise: frames differ in content and in coded size
        imgs[i, 17 * i:17 * i + i + 1] = rng.integers(0, 256, (i + 1, cols), dtype=np.uint8)
    got = cct_hip.dicom_rle_encode_batch(imgs)
    assert len(set(len(f) for f in got)) == n
    for i in (0, 6, 7, 8):
        assert got[i] == cct_hip.dicom_rle_encode_batch(imgs[i:i + 1])[0], i


def test_decode_in_two_passes_keeps_refused_slots():
    """9 frames of 8192 x 8192 uint16, one value each: a pass holds 2 * 2^29 bytes of rasters, 8 of them, so the batch runs
    as 8 + 1.  A row of one value is 64 replicate packets of 128, a segment 1 MiB.  One frame of each pass ends two bytes
    early: CCT_E_STREAM for those two, and their slots in host memory stay as they were."""
    import cct_hip
    from cct_hip import _ffi
    rows = cols = 8192
    n, N = 9, rows * cols
    assert (2 * PASS_BYTES) // (2 * N) == 8
    value = lambda i: ((i + 1) << 8) | (0x80 + i)  # noqa: E731

    def frame(i, cut=0):
        hi, lo = (np.tile(np.array([129, b], np.uint8), rows * cols // 128).tobytes() for b in (value(i) >> 8, value(i) & 0xFF))
        return struct.pack("<16I", 2, 64, 64 + len(hi), *([0] * 13)) + hi + lo[:len(lo) - cut]

    bad = (3, 8)
    frames = [frame(i, 2 if i in bad else 0) for i in range(n)]
    assert len(frames[0]) == 64 + (2 << 20)
    want_status = [E_STREAM if i in bad else 0 for i in range(n)]

    def check(res):
        for i in range(n):
            if i not in bad:
                for r in (0, rows // 2, rows - 1):
                    assert (res[i, r] == value(i)).all(), (i, r)

    res, status = cct_hip.dicom_rle_decode_batch(frames, rows, cols, raise_errors=False)
    assert list(status) == want_status
    check(res)
    # the C entry point, into a buffer that holds a sentinel
    res[:] = 0xA5A5
    blob = b"".join(frames)
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum([len(f) for f in frames], out=offs[1:])
    status = np.zeros(n, np.uint32)
    rc = _ffi.lib().cct_dicom_rle_decode_batch(blob, offs.ctypes.data, n, rows, cols, 16, res.ctypes.data, 0, res.size, status.ctypes.data)
    assert rc == E_STREAM and list(status) == want_status
    check(res)
    for i in bad:
        assert (res[i] == 0xA5A5).all(), i
