"""Device JPEG-LS lossless codec (cct_jpegls_encode_batch / _decode_batch) against tests/jpeg_ls_model.py: the worked example
of T.87 Annex H.3, files byte for byte over shapes, precisions and restart intervals, rasters back from the device's and
the model's files, host and device input, per-frame overflow, phantom slices, the JLS column of tools/evaluate.py and the
argument checks."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import jpeg_ls_model as m

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_STREAM, E_MIXED, E_JPEGLS = 3, 4, 10, 16


def bits_of(precision):
    return 8 if precision <= 8 else 16


@functools.lru_cache(maxsize=None)
def cases(precision):
    """[(rows, cols, names, rasters (n, rows, cols), {restart rows: the model's files})] over ROWS x COLS: computed once"""
    out = []
    for rows in m.ROWS:
        for cols in m.COLS:
            c = m.raster_cases(rows, cols, precision)
            files = {rr: [m.encode_frame(x, precision, rr) for x in c.values()] for rr in m.RESTARTS}
            out.append((rows, cols, list(c), np.stack(list(c.values())), files))
    return out


@functools.lru_cache(maxsize=None)
def phantoms():
    from cct_hip.synth import ct_phantom
    return np.stack([ct_phantom(seed, n=128) for seed in range(4)]).astype(np.uint16)


def test_annex_h3():
    import cct_hip
    assert cct_hip.jpeg_ls_encode_batch(m.H3_RASTER) == [m.H3_FILE]
    assert np.array_equal(cct_hip.jpeg_ls_decode_batch([m.H3_FILE], 4, 4, bits=8)[0], m.H3_RASTER)
    assert cct_hip.jpeg_ls_info(m.H3_FILE) == (4, 4, 8)


@pytest.mark.parametrize("precision", m.PRECISIONS)
def test_encode_equals_the_model(precision):
    import cct_hip
    bound = cct_hip._ffi.lib().cct_jpegls_bound
    for rows, cols, names, imgs, files in cases(precision):
        for rr in m.RESTARTS:
            got = cct_hip.jpeg_ls_encode_batch(imgs, precision=precision, restart_rows=rr)  # one mixed batch per shape
            for name, g, f in zip(names, got, files[rr]):
                assert g == f, (rows, cols, rr, name)
                assert len(g) <= bound(rows, cols, rr)


def test_encode_the_census_rasters():
    """what raster_cases does not reach: codes of 64 bits, RUNindex past 16, the interruption contexts' halving, 1-bit noise"""
    import cct_hip
    for name, (x, p) in m.census_cases().items():
        for rr in (0, 3):
            f = cct_hip.jpeg_ls_encode_batch(x, precision=p, restart_rows=rr)[0]
            assert f == m.encode_frame(x, p, rr), (name, rr)
            assert np.array_equal(cct_hip.jpeg_ls_decode_batch([f], *x.shape, bits=bits_of(p))[0], x), (name, rr)
    ones = np.full((3, 200), 65535, np.uint16)  # one escape code far from the initial state, then runs of growing RUNindex
    assert cct_hip.jpeg_ls_encode_batch(ones)[0] == m.encode_frame(ones, 16)


@pytest.mark.parametrize("precision", m.PRECISIONS)
def test_decode_the_models_and_the_devices_files(precision):
    import cct_hip
    bits = bits_of(precision)
    for rows, cols, names, imgs, files in cases(precision):
        for rr in m.RESTARTS:
            back = cct_hip.jpeg_ls_decode_batch(files[rr], rows, cols, bits=bits)
            assert back.dtype == imgs.dtype and back.shape == imgs.shape
            for name, b, x in zip(names, back, imgs):
                assert np.array_equal(b, x), (rows, cols, rr, name)
        own = cct_hip.jpeg_ls_encode_batch(imgs, precision=precision, restart_rows=2)
        assert np.array_equal(cct_hip.jpeg_ls_decode_batch(own, rows, cols, bits=bits), imgs), (rows, cols)


def test_phantoms_from_host_and_device():
    import cct_hip
    imgs = phantoms()
    assert imgs.max() < 4096
    for p in (12, 16):
        want = [m.encode_frame(x, p) for x in imgs[:2]]
        files = cct_hip.jpeg_ls_encode_batch(imgs, precision=p)
        assert files[:2] == want
        d = cct_hip.DeviceBuffer.from_numpy(imgs)
        try:
            assert cct_hip.jpeg_ls_encode_batch(d, shape=imgs.shape, precision=p) == files
            assert cct_hip.jpeg_ls_encode_batch(d, shape=imgs.shape[1:], precision=p) == files[:1]
            rr16 = cct_hip.jpeg_ls_encode_batch(d, shape=imgs.shape, precision=p, restart_rows=16)
        finally:
            d.free()
        assert rr16 == cct_hip.jpeg_ls_encode_batch(imgs, precision=p, restart_rows=16) and rr16[0] == m.encode_frame(imgs[0], p, 16)
        assert np.array_equal(cct_hip.jpeg_ls_decode_batch(files, 128, 128), imgs)
        assert np.array_equal(cct_hip.jpeg_ls_decode_batch(rr16, 128, 128), imgs)
        out = cct_hip.DeviceBuffer.from_numpy(np.zeros_like(imgs))
        try:
            assert cct_hip.jpeg_ls_decode_batch(rr16, 128, 128, out_dev=out) == imgs.shape
            assert np.array_equal(out.download(np.uint16, imgs.size).reshape(imgs.shape), imgs)
        finally:
            out.free()
    low = np.minimum(imgs >> 4, 255).astype(np.uint8)
    files8 = cct_hip.jpeg_ls_encode_batch(low)
    assert files8[0] == m.encode_frame(low[0], 8)
    assert np.array_equal(cct_hip.jpeg_ls_decode_batch(files8, 128, 128, bits=8), low)
    frames = cct_hip.dicom_fragments(cct_hip.dicom_encapsulate(files8))  # odd files keep their pad byte
    assert np.array_equal(cct_hip.jpeg_ls_decode_batch(frames, 128, 128, bits=8), low)


def test_encode_overflow_is_per_frame():
    import cct_hip
    L = cct_hip._ffi.lib()
    imgs = np.random.default_rng(2).integers(0, 4096, (4, 6, 70)).astype(np.uint16)
    imgs[1, 5, 69] = 4096
    imgs[3, 0, 0] = 65535
    stride = L.cct_jpegls_bound(6, 70, 0)
    out = np.zeros((4, stride), np.uint8)
    sizes, status = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    rc = L.cct_jpegls_encode_batch(imgs.ctypes.data, 0, 4, 6, 70, 16, 12, 0, out.ctypes.data, stride, sizes.ctypes.data, status.ctypes.data)
    assert rc == E_OVERFLOW and list(status) == [0, E_OVERFLOW, 0, E_OVERFLOW] and sizes[1] == 0 and sizes[3] == 0
    for i in (0, 2):
        assert out[i, :sizes[i]].tobytes() == m.encode_frame(imgs[i], 12)
    with pytest.raises(OverflowError):
        cct_hip.jpeg_ls_encode_batch(imgs, precision=12)


def test_decode_refusals_leave_the_rest_alone():
    import cct_hip
    from cct_hip import _ffi
    rows, cols = 5, 63
    c = m.raster_cases(rows, cols, 8)
    good = m.encode_frame(c["spikes"], 8, 2)
    sof = good.index(b"\xff\xda")
    batch = [good, good[:sof + 7] + b"\x01" + good[sof + 8:], m.encode_frame(c["noise"], 8), good[:7] + b"\x00\x08" + good[9:],
             good[:-12] + good[-2:], b"junk", m.encode_frame(c["flats"], 8, 1)]
    want_status = [0, E_JPEGLS, 0, E_MIXED, E_STREAM, E_JPEGLS, 0]
    want_img = [c["spikes"], None, c["noise"], None, None, None, c["flats"]]
    n = len(batch)
    sentinel = np.full((n + 1, rows, cols), 0xA5, np.uint8)
    d = cct_hip.DeviceBuffer.from_numpy(sentinel)
    try:
        shape, status = cct_hip.jpeg_ls_decode_batch(batch, rows, cols, bits=8, out_dev=d, raise_errors=False)
        got = d.download(np.uint8, sentinel.size).reshape(sentinel.shape)
    finally:
        d.free()
    assert shape == (n, rows, cols) and list(status) == want_status
    for i in range(n):
        if want_img[i] is not None:
            assert np.array_equal(got[i], want_img[i]), i
        elif want_status[i] != E_STREAM:
            assert (got[i] == 0xA5).all(), i  # refused by the marker walk: never sent to the device
    assert (got[n] == 0xA5).all()  # the slot behind the batch
    with pytest.raises(ValueError):
        cct_hip.jpeg_ls_decode_batch(batch, rows, cols, bits=8)
    with pytest.raises(_ffi.CorruptStreamError):
        cct_hip.jpeg_ls_decode_batch([good, batch[4]], rows, cols, bits=8)
    with pytest.raises(ValueError):
        cct_hip.jpeg_ls_info(batch[1])
    p12 = m.encode_frame(m.raster_cases(rows, cols, 12)["noise"], 12)
    _, status = cct_hip.jpeg_ls_decode_batch([p12], rows, cols, bits=8, raise_errors=False)
    assert list(status) == [E_MIXED]  # precision 12 does not fit 8 bits


def test_evaluate_tool_appends_the_jls_column(tmp_path):
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
    assert tool.main([str(tmp_path), "--results", str(out), "--jls", "device"]) == 0
    with_jls = out.read_text().splitlines()
    assert with_jls[0].split(",") == ["File", "Raw", "ZIP", "PNG", "RLE", "JP2", "CCT", "JLS"]
    for ln, img in zip(with_jls[1:], imgs):
        assert int(ln.split(",")[-1]) == len(cct_hip.dicom_encapsulate(cct_hip.jpeg_ls_encode_batch(img, precision=16)))
    assert int(with_jls[1].split(",")[-1]) == len(cct_hip.dicom_encapsulate([m.encode_frame(imgs[0], 16)]))
    assert tool.main([str(tmp_path), "--results", str(out)]) == 0
    plain = out.read_text().splitlines()
    assert plain[0] == "File,Raw,ZIP,PNG,RLE,JP2,CCT"
    assert plain == [ln.rsplit(",", 1)[0] for ln in with_jls]  # the other columns are what they were


def test_argument_refusals_come_before_the_device(monkeypatch):
    import cct_hip
    from cct_hip import _ffi
    L = _ffi.lib()

    def touched(*a, **k):
        raise AssertionError("the device entry point was reached")

    img = np.zeros((4, 4), np.uint16)
    assert L.cct_jpegls_bound(0, 4, 0) == 0 and L.cct_jpegls_bound(4, 4, -1) == 0 and L.cct_jpegls_bound(4, 4, 0) > 34
    assert L.cct_jpegls_bound(17, 130, 2) >= 9 * ((64 * 2 * 130 + 2) // 7 + 4)
    with monkeypatch.context() as mp:
        mp.setattr(L, "cct_jpegls_encode_batch", touched)
        mp.setattr(L, "cct_jpegls_decode_batch", touched)
        for kw, exc in ((dict(precision=1), ValueError), (dict(precision=17), ValueError), (dict(restart_rows=-1), ValueError),
                        (dict(restart_rows=65536), ValueError), (dict(precision=12.5), TypeError)):
            with pytest.raises(exc):
                cct_hip.jpeg_ls_encode_batch(img, **kw)
        with pytest.raises(ValueError):
            cct_hip.jpeg_ls_encode_batch(img.astype(np.uint8), precision=9)
        with pytest.raises(TypeError):
            cct_hip.jpeg_ls_encode_batch(img.astype(np.int32))
        assert cct_hip.jpeg_ls_encode_batch(np.zeros((0, 4, 4), np.uint16)) == []
        for args, kw, exc in ((([m.H3_FILE], 0, 4), {}, ValueError), (([m.H3_FILE], 4, 70000), {}, ValueError),
                              (([m.H3_FILE], 4, 4), dict(bits=12), ValueError), ((["text"], 4, 4), {}, TypeError)):
            with pytest.raises(exc):
                cct_hip.jpeg_ls_decode_batch(*args, **kw)
        with pytest.raises(TypeError):
            cct_hip.jpeg_ls_info("text")
    # the C entry points themselves: whole-call refusals, decided before a device is needed
    sizes, status = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    out = np.zeros(4096, np.uint8)
    enc = lambda **k: L.cct_jpegls_encode_batch(img.ctypes.data, 0, 1, k.get("rows", 4), 4, k.get("src_bits", 16), k.get("precision", 16),
                                                k.get("rr", 0), out.ctypes.data, k.get("stride", 4096), sizes.ctypes.data, status.ctypes.data)
    assert enc(rows=0) == _ffi.E_ARG and enc(src_bits=12) == _ffi.E_ARG and enc(precision=17) == _ffi.E_ARG and enc(rr=-1) == _ffi.E_ARG
    assert enc(stride=L.cct_jpegls_bound(4, 4, 0) - 1) == _ffi.E_CAP
