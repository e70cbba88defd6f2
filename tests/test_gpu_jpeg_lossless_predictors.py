"""The predictor argument of the device JPEG Lossless encoder (cct_jpegll_encode_batch_sv) against tests/jpeg_lossless_model.py:
files byte for byte under every selection value, differences that leave 16 bits, the per-frame choice of predictor 0 against
tests/jpeg_lossless_predictors.py, round trips through the device's own decoder, per-frame overflow, the unchanged default
and old entry point, and the --jpl-predictor option of tools/evaluate.py."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import golden_inputs as gi
import jpeg_lossless_model as m
import jpeg_lossless_predictors as jp

pytestmark = pytest.mark.gpu

E_OVERFLOW = 3


@functools.lru_cache(maxsize=None)
def cases(precision):
    """[(rows, cols, names, rasters (n, rows, cols))] over ROWS x COLS"""
    out = []
    for rows, cols in jp.SHAPES:
        c = m.raster_cases(rows, cols, precision, jp.PRECISIONS[precision])
        out.append((rows, cols, list(c), np.stack(list(c.values()))))
    return out


def encode_sv(imgs, precision, predictor, restart_rows=0):
    """cct_jpegll_encode_batch_sv on host rasters -> (return code, files, status, Ss per frame)"""
    import cct_hip
    L = cct_hip._ffi.lib()
    n, rows, cols = imgs.shape
    stride = L.cct_jpegll_bound(rows, cols, restart_rows)
    out = np.zeros((n, stride), np.uint8)
    sizes, status, sel = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rc = L.cct_jpegll_encode_batch_sv(imgs.ctypes.data, 0, n, rows, cols, 8 * imgs.dtype.itemsize, precision, predictor, restart_rows,
                                      out.ctypes.data, stride, sizes.ctypes.data, status.ctypes.data, sel.ctypes.data)
    return rc, [out[i, :sizes[i]].tobytes() for i in range(n)], list(status), list(sel)


@pytest.mark.parametrize("precision", sorted(jp.PRECISIONS))
def test_fixed_predictors_equal_the_model(precision):
    """rows 1: all Ra; cols 1: all Rb; 17 x 257 crosses four steps of the emit kernel and the histogram's grid stride"""
    import cct_hip
    for rows, cols, names, imgs in cases(precision):
        for rr in jp.RESTARTS:
            for ss in jp.PREDICTORS:
                got = cct_hip.jpeg_lossless_encode_batch(imgs, precision=precision, restart_rows=rr, predictor=ss)
                for name, g, x in zip(names, got, imgs):
                    assert g == m.encode_frame(x, precision, predictor=ss, restart_rows=rr), (rows, cols, rr, ss, name)


def test_differences_that_leave_16_bits():
    wrap = jp.wrap_rasters()
    imgs = np.stack(list(wrap.values()))
    wide = imgs.astype(np.int64)
    ra, rb, rc = wide[:, 1:, :-1], wide[:, :-1, 1:], wide[:, :-1, :-1]
    assert (ra + rb - rc).max() > 65535 and (ra + rb - rc).min() < 0  # what selection value 4 predicts inside the rasters
    for ss in jp.PREDICTORS:
        cat = np.concatenate([m.categories(m.differences(x, 16, ss)[0])[0].ravel() for x in imgs])
        assert (cat == 16).any()
        rc_, files, status, sel = encode_sv(imgs, 16, ss)
        assert rc_ == 0 and status == [0] * 3 and sel == [ss] * 3
        for name, f, x in zip(wrap, files, imgs):
            assert f == m.encode_frame(x, 16, predictor=ss), (name, ss)


@functools.lru_cache(maxsize=None)
def auto_batch():
    """128 x 128 uint16 at precision 12: the planted rasters tiled, a phantom and noise"""
    tiled = [np.tile(x, (8, 6))[:128, :128].astype(np.uint16) for x, _, _ in jp.planted().values()]
    noise = np.random.default_rng(11).integers(0, 4096, (128, 128)).astype(np.uint16)
    return np.stack(tiled + [gi.ct_phantom(1, 128).astype(np.uint16), noise])


def test_auto_takes_the_cheapest_per_frame():
    import cct_hip
    small = np.stack([x for x, _, _ in jp.planted().values()])  # the 16 x 24 rasters of the host test
    rc, files, status, sel = encode_sv(small, 8, 0)
    assert rc == 0 and status == [0] * 3 and sel == [want for _, _, want in jp.planted().values()] == [1, 2, 3]
    for f, x, s in zip(files, small, sel):
        assert jp.sos_predictor(f) == s and f == m.encode_frame(x, 8, predictor=s)
    imgs = auto_batch()
    for rr in (0, 16):
        picks = [jp.auto_pick(x, 12, rr) for x in imgs]
        rc, files, status, sel = encode_sv(imgs, 12, 0, rr)
        assert rc == 0 and status == [0] * len(imgs)
        assert sel == picks and [jp.sos_predictor(f) for f in files] == picks, rr
        assert len(set(sel)) >= 2  # frames of one call differ
        for f, x, s in zip(files, imgs, picks):
            assert f == m.encode_frame(x, 12, predictor=s, restart_rows=rr), (rr, s)
        assert cct_hip.jpeg_lossless_encode_batch(imgs, precision=12, restart_rows=rr, predictor="auto") == files
        assert cct_hip.jpeg_lossless_encode_batch(imgs, precision=12, restart_rows=rr, predictor=0) == files


def test_auto_over_the_small_shapes():
    """the choice where a frame is one row, one column or a few samples: every candidate sees the same first row and column"""
    for precision in sorted(jp.PRECISIONS):
        for rows, cols, names, imgs in cases(precision):
            if (rows, cols) not in ((1, 1), (1, 65), (17, 1), (2, 2), (3, 63), (17, 257)):
                continue
            rr = 2 if rows > 2 else 0
            rc, files, status, sel = encode_sv(imgs, precision, 0, rr)
            assert rc == 0
            for name, f, x, s in zip(names, files, imgs, sel):
                assert s == jp.auto_pick(x, precision, rr), (rows, cols, precision, name)
                assert f == m.encode_frame(x, precision, predictor=s, restart_rows=rr), (rows, cols, precision, name)


@pytest.mark.parametrize("predictor", [2, 3, 4, 5, 6, 7, "auto"])
def test_round_trip_through_the_device_decoder(predictor):
    import cct_hip
    imgs = auto_batch()
    files = cct_hip.jpeg_lossless_encode_batch(imgs, precision=12, restart_rows=0 if predictor in (2, 5) else 16, predictor=predictor)
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch(files, 128, 128), imgs)
    d = cct_hip.DeviceBuffer.from_numpy(imgs)
    try:
        assert cct_hip.jpeg_lossless_encode_batch(d, shape=imgs.shape, precision=12, restart_rows=0 if predictor in (2, 5) else 16,
                                                  predictor=predictor) == files
    finally:
        d.free()
    odd = m.raster_cases(17, 257, 16, np.uint16)
    x = np.stack(list(odd.values()))
    assert np.array_equal(cct_hip.jpeg_lossless_decode_batch(cct_hip.jpeg_lossless_encode_batch(x, restart_rows=5, predictor=predictor), 17, 257), x)


@pytest.mark.parametrize("predictor", [4, 0])
def test_overflow_is_per_frame(predictor):
    import cct_hip
    imgs = np.random.default_rng(2).integers(0, 4096, (4, 6, 70)).astype(np.uint16)
    imgs[1, 5, 69] = 4096
    imgs[3, 0, 0] = 65535
    rc, files, status, sel = encode_sv(imgs, 12, predictor)
    assert rc == E_OVERFLOW and status == [0, E_OVERFLOW, 0, E_OVERFLOW]
    assert files[1] == b"" and files[3] == b""
    assert all(1 <= s <= 7 for s in sel)  # filled for the frames that failed too
    for i in (0, 2):
        want = predictor or jp.auto_pick(imgs[i], 12)
        assert sel[i] == want and files[i] == m.encode_frame(imgs[i], 12, predictor=want), i
    if predictor:
        assert sel == [predictor] * 4
    with pytest.raises(OverflowError):
        cct_hip.jpeg_lossless_encode_batch(imgs, precision=12, predictor=predictor)


def test_default_and_old_entry_point_write_the_same_bytes():
    import cct_hip
    L = cct_hip._ffi.lib()
    for precision in (8, 12):
        rows, cols, names, imgs = cases(precision)[-1]  # 17 x 257
        for rr in (0, 5):
            want = [m.encode_frame(x, precision, restart_rows=rr) for x in imgs]
            assert cct_hip.jpeg_lossless_encode_batch(imgs, precision=precision, restart_rows=rr) == want
            assert cct_hip.jpeg_lossless_encode_batch(imgs, precision=precision, restart_rows=rr, predictor=1) == want
            rc, files, status, sel = encode_sv(imgs, precision, 1, rr)
            assert rc == 0 and files == want and sel == [1] * len(imgs)
            n, stride = len(imgs), L.cct_jpegll_bound(rows, cols, rr)
            out = np.zeros((n, stride), np.uint8)
            sizes, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            assert L.cct_jpegll_encode_batch(imgs.ctypes.data, 0, n, rows, cols, 8 * imgs.dtype.itemsize, precision, rr, out.ctypes.data,
                                             stride, sizes.ctypes.data, status.ctypes.data) == 0
            assert [out[i, :sizes[i]].tobytes() for i in range(n)] == want
    rc, files, status, sel = encode_sv(np.zeros((1, 4, 4), np.uint16), 16, 3)  # h_predictors may be NULL
    n1 = np.zeros(1, np.uint32)
    out = np.zeros(L.cct_jpegll_bound(4, 4, 0), np.uint8)
    assert L.cct_jpegll_encode_batch_sv(np.zeros((4, 4), np.uint16).ctypes.data, 0, 1, 4, 4, 16, 16, 3, 0, out.ctypes.data, out.size,
                                        n1.ctypes.data, np.zeros(1, np.uint32).ctypes.data, None) == 0
    assert out[:n1[0]].tobytes() == files[0]


def test_evaluate_tool_takes_the_predictor(tmp_path):
    import cct_hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("evaluate_tool", os.path.join(root, "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    imgs = [gi.ct_phantom(seed, n=128).astype(np.uint16) for seed in (1, 2)]
    for k, img in enumerate(imgs):
        np.save(tmp_path / f"slice{k}.npy", img)
    out = tmp_path / "out.csv"
    assert tool.main([str(tmp_path), "--results", str(out), "--jpl", "device"]) == 0
    default = out.read_text().splitlines()
    assert tool.main([str(tmp_path), "--results", str(out), "--jpl", "device", "--jpl-predictor", "1"]) == 0
    assert out.read_text().splitlines() == default  # without the option the CSV is what it was
    for ln, img in zip(default[1:], imgs):
        assert int(ln.split(",")[-1]) == len(cct_hip.dicom_encapsulate([m.encode_frame(img, 16)]))
    assert tool.main([str(tmp_path), "--results", str(out), "--jpl", "device", "--jpl-predictor", "auto"]) == 0
    auto = out.read_text().splitlines()
    assert auto[0] == default[0] and auto[0].split(",")[-1] == "JPL"
    for ln, was, img in zip(auto[1:], default[1:], imgs):
        f = m.encode_frame(img, 16, predictor=jp.auto_pick(img, 16))
        assert int(ln.split(",")[-1]) == len(cct_hip.dicom_encapsulate([f]))
        assert ln.rsplit(",", 1)[0] == was.rsplit(",", 1)[0]
    assert tool.main([str(tmp_path), "--results", str(out), "--jpl", "device", "--jpl-predictor", "7"]) == 0
    for ln, img in zip(out.read_text().splitlines()[1:], imgs):
        assert int(ln.split(",")[-1]) == len(cct_hip.dicom_encapsulate([m.encode_frame(img, 16, predictor=7)]))
