"""Device DICOM RLE Lossless codec (cct_dicom_rle_encode_batch / _decode_batch) against tests/dicom_rle_model.py: frames
byte for byte, rasters from the device's, the model's and libtiff's frames, hand-built segments, packet heads on every
offset of a decoder tile, per-frame refusals, and the RLE column of tools/evaluate.py."""
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
