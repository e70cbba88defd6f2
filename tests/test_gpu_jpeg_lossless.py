"""Device JPEG Lossless codec (cct_jpegll_encode_batch / _decode_batch) against tests/jpeg_lossless_model.py: files byte for
byte over shapes, precisions and restart intervals, rasters back from the device's and the model's files with every
predictor, point transforms, foreign Huffman tables and extra segments, long intervals, per-file refusals, Pillow on the
8-bit files, and the JPL column of tools/evaluate.py."""
import functools
import importlib.util
import io
import os

import numpy as np
import pytest

import jpeg_lossless_model as m

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_STREAM, E_MIXED, E_JPEG = 3, 4, 10, 13
PRECISIONS = {8: np.uint8, 12: np.uint16, 16: np.uint16}
CODE16 = ([1] * 14 + [0, 3], list(range(17)))  # categories 14 .. 16 get 16-bit words: 31 bits a sample with the extra bits


@functools.lru_cache(maxsize=None)
def cases(precision):
    """[(rows, cols, names, rasters (n, rows, cols))] over ROWS x COLS"""
    out = []
    for rows in m.ROWS:
        for cols in m.COLS:
            c = m.raster_cases(rows, cols, precision, PRECISIONS[precision])
            out.append((rows, cols, list(c), np.stack(list(c.values()))))
    return out


@functools.lru_cache(maxsize=None)
def phantoms():
    from cct_hip.synth import ct_phantom
    return np.stack([ct_phantom(seed, n=128) for seed in range(4)]).astype(np.uint16)


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_encode_equals_the_model(precision):
    import cct_hip
    for rows, cols, names, imgs in cases(precision):
        for rr in (0, 1, 2):
            got = cct_hip.jpeg_lossless_encode_batch(imgs, precision=precision, restart_rows=rr)  # one mixed batch per shape
            for name, g, x in zip(names, got, imgs):
                assert g == m.encode_frame(x, precision, restart_rows=rr), (rows, cols, rr, name)
                assert len(g) <= cct_hip._ffi.lib().cct_jpegll_bound(rows, cols, rr)


def test_encode_known_answers():
    import cct_hip
    img = np.array([[0, 65535, 0, 32768, 0, 32767, 65535, 1]], dtype=np.uint16)
    want = "ffd8ffc3000b100001000801011100ffc4001700010101010000000000000000000000001001020fffda00080101000100004a77ff00f6bfffd9"
    assert cct_hip.jpeg_lossless_encode_batch(img)[0].hex() == want
    fib = m.fibonacci_raster()  # code lengths limited from 17 to 16
    f = cct_hip.jpeg_lossless_encode_batch(fib)[0]
    at = f.index(b"\xff\xc4")
    assert f[at + 5:at + 21] == bytes([1] * 14 + [0, 3]) and f[at + 21:at + 38] == bytes(range(16, -1, -1))
    assert f == m.encode_frame(fib, 16)
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch([f], 1, 6763)[0], fib)
    alt = np.where(np.arange(2048) % 2 == 0, 0, 65535).astype(np.uint16).reshape(2, 1024)  # differences of +1 and -1 modulo 2^16
    f = cct_hip.jpeg_lossless_encode_batch(alt)[0]
    assert f == m.encode_frame(alt, 16)
    noise = np.random.default_rng(8).integers(0, 65536, (4, 1500)).astype(np.uint16)  # long enough for stuffed bytes
    f = cct_hip.jpeg_lossless_encode_batch(noise)[0]
    assert f == m.encode_frame(noise, 16)
    assert f[f.index(b"\xff\xda") + 10:-2].count(b"\xff\x00") > 10


def test_encode_phantoms_from_host_and_device():
    import cct_hip
    imgs = phantoms()
    want = [m.encode_frame(x, 16) for x in imgs]
    assert cct_hip.jpeg_lossless_encode_batch(imgs) == want
    d = cct_hip.DeviceBuffer.from_numpy(imgs)
    try:
        assert cct_hip.jpeg_lossless_encode_batch(d, shape=imgs.shape) == want
        assert cct_hip.jpeg_lossless_encode_batch(d, shape=imgs.shape[1:]) == want[:1]
        assert cct_hip.jpeg_lossless_encode_batch(d, shape=imgs.shape, restart_rows=16) == [m.encode_frame(x, 16, restart_rows=16) for x in imgs]
    finally:
        d.free()
    low = np.minimum(imgs >> 4, 255).astype(np.uint8)
    assert cct_hip.jpeg_lossless_encode_batch(low) == [m.encode_frame(x, 8) for x in low]
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch(want, 128, 128), imgs)


def test_encode_overflow_is_per_frame():
    import cct_hip
    L = cct_hip._ffi.lib()
    imgs = np.random.default_rng(2).integers(0, 4096, (4, 6, 70)).astype(np.uint16)
    imgs[1, 5, 69] = 4096
    imgs[3, 0, 0] = 65535
    stride = L.cct_jpegll_bound(6, 70, 0)
    out = np.zeros((4, stride), np.uint8)
    sizes, status = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    rc = L.cct_jpegll_encode_batch(imgs.ctypes.data, 0, 4, 6, 70, 16, 12, 0, out.ctypes.data, stride, sizes.ctypes.data, status.ctypes.data)
    assert rc == E_OVERFLOW and list(status) == [0, E_OVERFLOW, 0, E_OVERFLOW]
    for i in (0, 2):
        assert out[i, :sizes[i]].tobytes() == m.encode_frame(imgs[i], 12)
    with pytest.raises(OverflowError):
        cct_hip.jpeg_lossless_encode_batch(imgs, precision=12)


def test_device_files_open_in_pillow():
    if not m.pillow_opens_sof3():  # probed with a file of the model, before any device work
        pytest.skip("this Pillow's libjpeg does not open SOF3")
    import cct_hip
    from PIL import Image
    imgs = np.minimum(phantoms() >> 4, 255).astype(np.uint8)
    noise = np.random.default_rng(4).integers(0, 256, (3, 19, 23)).astype(np.uint8)
    for batch in (imgs, noise):
        for rr in (0, 1, 4):
            for f, x in zip(cct_hip.jpeg_lossless_encode_batch(batch, restart_rows=rr), batch):
                assert np.array_equal(np.array(Image.open(io.BytesIO(f))), x), rr


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_decode_the_devices_files(precision):
    import cct_hip
    bits = 8 if precision == 8 else 16
    for rows, cols, names, imgs in cases(precision):
        for rr in (0, 1, 2):
            files = cct_hip.jpeg_lossless_encode_batch(imgs, precision=precision, restart_rows=rr)
            back = cct_hip.jpeg_lossless_decode_batch(files, rows, cols, bits=bits)
            assert back.dtype == imgs.dtype and back.shape == imgs.shape
            for name, b, x in zip(names, back, imgs):
                assert np.array_equal(b, x), (rows, cols, rr, name)


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_decode_the_models_files_every_predictor(precision):
    import cct_hip
    bits = 8 if precision == 8 else 16
    for rows, cols in ((1, 1), (2, 3), (3, 65), (17, 63), (17, 257)):
        c = m.raster_cases(rows, cols, precision, PRECISIONS[precision])
        files, want, tags = [], [], []
        for k, (name, img) in enumerate(c.items()):
            for ss in range(1, 8):
                for pt in (0, 2):
                    rr = (ss + pt // 2 + k) % 4  # restart rows 0 .. 3 rotate over the cases
                    files.append(m.encode_frame(img, precision, ss, pt, rr))
                    want.append((img >> pt) << pt)
                    tags.append((name, ss, pt, rr))
        back = cct_hip.jpeg_lossless_decode_batch(files, rows, cols, bits=bits)
        for tag, b, w in zip(tags, back, want):
            assert np.array_equal(b, w), (rows, cols, tag)


def test_decode_foreign_tables_and_segments():
    import cct_hip
    rng = np.random.default_rng(6)
    rows, cols = 9, 70
    noise = rng.integers(0, 65536, (rows, cols)).astype(np.uint16)
    const = np.full((rows, cols), 32768, np.uint16)
    own = m.huffman_table(np.bincount(m.categories(m.differences(noise, 16)[0])[0].ravel(), minlength=17))
    junk = ([0, 1] + [0] * 14, [5])
    app = [m.segment(0xE0, b"JFIF\0\1\2"), m.segment(0xFE, b"a comment"), m.segment(0xEF, bytes(1000))]
    files = [
        m.encode_frame(noise, 16, table=m.FLAT5),
        m.encode_frame(noise, 16, table=CODE16),
        m.encode_frame(noise, 16, 5, 0, 3, table=CODE16),
        m.encode_frame(const, 16, table=([1] + [0] * 15, [0])),  # one symbol, one bit a sample
        m.encode_frame(noise, 16, pre_segments=app),
        # table 0 defined wrong, then redefined; the tables of ids 1 and 2 ride along
        m.encode_frame(noise, 16, table=own, dht_segments=[m.dht_payload([(1, *junk), (0, *m.FLAT5)]), m.dht_payload([(2, *CODE16)]),
                                                           m.dht_payload([(0, *own)])]),
        # the scan names id 3, defined in the middle of a segment of three
        m.encode_frame(noise, 16, 4, 0, 2, table=m.FLAT5, table_id=3,
                       dht_segments=[m.dht_payload([(0, *junk), (3, *m.FLAT5), (1, *CODE16)])], pre_segments=app[:1]),
    ]
    want = [noise, noise, noise, const, noise, noise, noise]
    assert len(files[3]) < 200
    for f, w in zip(files, want):
        assert np.array_equal(m.decode_frame(f, rows, cols), w)
    back = cct_hip.jpeg_lossless_decode_batch(files, rows, cols)
    for i, w in enumerate(want):
        assert np.array_equal(back[i], w), i
    frames = cct_hip.dicom_fragments(cct_hip.dicom_encapsulate(files))  # odd files keep their pad byte
    assert any(len(a) != len(b) for a, b in zip(frames, files))
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch(frames, rows, cols), np.stack(want))


def test_decode_long_intervals():
    """64 x 520: an interval of many subsequences, code words across every subsequence border, and the one-bit frame"""
    import cct_hip
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 65536, (64, 520)).astype(np.uint16)
    const = np.full((64, 520), 128, np.uint8)
    files = [m.encode_frame(noise, 16), m.encode_frame(noise, 16, table=CODE16), m.encode_frame(noise, 16, 7, 0, 0), m.encode_frame(noise, 16, 6, 3, 5)]
    assert 8 * len(files[1]) > 30 * noise.size  # close to 31 bits a sample
    back = cct_hip.jpeg_lossless_decode_batch(files, 64, 520)
    for i in range(3):
        assert np.array_equal(back[i], noise), i
    assert np.array_equal(back[3], (noise >> 3) << 3)
    one = m.encode_frame(const, 8, table=([1] + [0] * 15, [0]))
    assert len(one) < 64 * 520 // 8 + 64
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch([one, cct_hip.jpeg_lossless_encode_batch(const)[0]], 64, 520, bits=8),
                          np.stack([const, const]))
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch(cct_hip.jpeg_lossless_encode_batch(noise[None]), 64, 520)[0], noise)


def test_decode_a_stream_that_never_resynchronises():
    """words of one length, 5 bits, and no extra bits: a lane that enters a 1 024-bit subsequence at its start is out of
    phase in four subsequences of five and stays so, every correction moves one subsequence on per round.  650
    subsequences, three windows of the decoder, its worst case."""
    import cct_hip
    const = np.full((256, 520), 128, np.uint8)
    f = m.encode_frame(const, 8, table=m.FLAT5)
    assert 8 * (len(f) - 80) > 649 * 1024
    restarts = m.encode_frame(const[:64], 8, restart_rows=16, table=m.FLAT5)
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch([f], 256, 520, bits=8)[0], const)
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch([restarts], 64, 520, bits=8)[0], const[:64])


def test_decode_refusals_leave_the_rest_alone():
    import cct_hip
    from cct_hip import _ffi
    rows, cols = 5, 37
    rng = np.random.default_rng(3)
    img = rng.integers(0, 4096, (rows, cols)).astype(np.uint16)
    others = rng.integers(0, 4096, (3, rows, cols)).astype(np.uint16)
    bad = m.damaged_files(img, 12)
    code = {"JPEG": E_JPEG, "MIXED": E_MIXED, "STREAM": E_STREAM}
    batch, want_status, want_img = [], [], []
    good = [m.encode_frame(others[0], 12), m.encode_frame(others[1], 12, 7, 0, 2), m.encode_frame(others[2], 12, 1, 0, 1)]
    for k, (name, (f, kind)) in enumerate(bad.items()):
        if k % 5 == 0:
            batch.append(good[(k // 5) % 3]); want_status.append(0); want_img.append(others[(k // 5) % 3])
        batch.append(f); want_status.append(code[kind]); want_img.append(None)
    batch.append(good[0]); want_status.append(0); want_img.append(others[0])
    n = len(batch)
    sentinel = np.full((n + 1, rows, cols), 0xA5A5, np.uint16)
    d = cct_hip.DeviceBuffer.from_numpy(sentinel)
    try:
        shape, status = cct_hip.jpeg_lossless_decode_batch(batch, rows, cols, out_dev=d, raise_errors=False)
        assert shape == (n, rows, cols)
        assert list(status) == want_status
        got = d.download(np.uint16, sentinel.size).reshape(sentinel.shape)
    finally:
        d.free()
    for i in range(n):
        if want_img[i] is not None:
            assert np.array_equal(got[i], want_img[i]), i
        elif want_status[i] != E_STREAM:
            assert (got[i] == 0xA5A5).all(), i  # refused by the marker walk: never sent to the device
    assert (got[n] == 0xA5A5).all()  # the slot behind the batch
    res, status = cct_hip.jpeg_lossless_decode_batch(batch, rows, cols, raise_errors=False)
    assert list(status) == want_status
    for i in range(n):
        if want_img[i] is not None:
            assert np.array_equal(res[i], want_img[i]), i
    with pytest.raises(ValueError):
        cct_hip.jpeg_lossless_decode_batch(batch, rows, cols)
    with pytest.raises(_ffi.CorruptStreamError):
        cct_hip.jpeg_lossless_decode_batch([good[0], bad["left_over"][0]], rows, cols)
    _, status = cct_hip.jpeg_lossless_decode_batch([good[0], good[1]], rows, cols, bits=8, raise_errors=False)
    assert list(status) == [E_MIXED, E_MIXED]  # precision 12 does not fit 8 bits


def test_evaluate_tool_appends_the_jpl_column(tmp_path):
    import cct_hip
    from cct_hip.synth import ct_phantom
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("evaluate_tool", os.path.join(root, "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    imgs = [ct_phantom(seed, n=128).astype(np.uint16) for seed in (1, 2)]
    for k, img in enumerate(imgs):
        np.save(tmp_path / f"slice{k}.npy", img)
    out = tmp_path / "out.csv"
    assert tool.main([str(tmp_path), "--results", str(out), "--jpl", "device"]) == 0
    with_jpl = out.read_text().splitlines()
    head = with_jpl[0].split(",")
    assert head == ["File", "Raw", "ZIP", "PNG", "RLE", "JP2", "CCT", "JPL"]
    for ln, img in zip(with_jpl[1:], imgs):
        assert int(ln.split(",")[-1]) == len(cct_hip.dicom_encapsulate([m.encode_frame(img, 16)]))
    assert tool.main([str(tmp_path), "--results", str(out)]) == 0
    plain = out.read_text().splitlines()
    assert plain[0] == "File,Raw,ZIP,PNG,RLE,JP2,CCT"
    assert plain == [ln.rsplit(",", 1)[0] for ln in with_jpl]  # the other columns are what they were


PASS_BYTES = 512 << 20  # csrc/api_jpeg_lossless.cpp JPL_PASS_BYTES


def test_batches_of_several_passes_equal_single_frames():
    """9 uint16 rasters of 4096 x 4096 at precision 16: the encoder holds cct_jpegll_bound + 4 bytes a sample per frame,
    about 188 MiB, so it runs as 2 + 2 + 2 + 2 + 1; the decoder holds 4 bytes a sample, 8 frames a pass as long as their
    files stay below a quarter of the pass, so it runs as 8 + 1.  Single frames are pinned to the model at small shapes."""
    import cct_hip
    from cct_hip import _ffi
    rows = cols = 4096
    n, N = 9, rows * cols
    dstride = (_ffi.lib().cct_jpegll_bound(rows, cols, 0) + 3) & ~3
    assert PASS_BYTES // (dstride + 4 * N) == 2
    rng = np.random.default_rng(22)
    ramp = (np.arange(rows, dtype=np.uint32)[:, None] * 3 + np.arange(cols, dtype=np.uint32)[None, :]).astype(np.uint16)
    noise = rng.integers(0, 8, (rows, cols), dtype=np.uint16)
    imgs = np.stack([ramp + (noise >> (i % 3)) + np.uint16(6000 * i) for i in range(n)])
    imgs[8, 0, 0] = 65535
    files = cct_hip.jpeg_lossless_encode_batch(imgs)
    assert len(set(len(f) for f in files)) >= 3
    for i in (0, 1, 2, 8):
        assert files[i] == cct_hip.jpeg_lossless_encode_batch(imgs[i:i + 1])[0], i
    assert sum(len(f) for f in files[:8]) <= PASS_BYTES // 4 and PASS_BYTES // (4 * N) == 8  # the decoder's first pass takes 8
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch(files, rows, cols), imgs)
    damaged = list(files)
    for i in (3, 8):  # the entropy-coded data ends early
        damaged[i] = files[i][:-1002] + files[i][-2:]
    back, status = cct_hip.jpeg_lossless_decode_batch(damaged, rows, cols, raise_errors=False)
    assert list(status) == [E_STREAM if i in (3, 8) else 0 for i in range(n)]
    for i in range(n):
        if i not in (3, 8):
            assert np.array_equal(back[i], imgs[i]), i
