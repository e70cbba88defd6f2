"""The predictor argument of the JPEG Lossless encoder without a GPU: the cost by which predictor 0 ("auto") chooses, on rasters
planted for one answer each and on real data; the model's files of every selection value against libjpeg-turbo (through
Pillow); the refusals of jpeg_lossless_encode_batch(predictor=...) before any C entry point; and cct_jpegll_encode_batch_sv in
the header, the library and its own refusals."""
import io
import os
import re

import numpy as np
import pytest

import golden_inputs as gi
import jpeg_lossless_model as m
import jpeg_lossless_predictors as jp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = 9


def test_auto_pick_on_planted_rasters():
    for name, (img, P, want) in jp.planted().items():
        assert jp.auto_pick(img, P) == want, name
    costs = jp.auto_costs(jp.constant(), 8)
    assert len(set(costs)) == 1  # all seven tie: the lowest
    costs = jp.auto_costs(jp.vertical_stripes(), 8)
    assert costs[1] == costs[3] == costs[5] == min(costs) and sorted(costs)[3] > min(costs)  # 2, 4 and 6 tie below the rest
    costs = jp.auto_costs(jp.falling_plane(), 8)
    assert costs[2] == costs[3] == costs[4] == costs[6] == min(costs) and sorted(costs)[4] > min(costs)  # 3, 4, 5 and 7: the lowest


def test_auto_pick_on_real_data():
    ct = jp.golden_slice("slice0671")
    assert ct.shape == (512, 512) and int(ct.max()) < 4096
    assert jp.auto_pick(ct, 12) == 7
    assert jp.auto_pick(gi.ct_phantom(1, 128).astype(np.uint16), 12) == 1


def test_auto_cost_is_the_file_less_stuffing_and_padding():
    """the cost counts the coded bits and the HUFFVAL bytes: the file is that, the pad bits of the interval, a stuffed zero behind
    every 0xFF, and a fixed number of header bytes"""
    img = np.random.default_rng(9).integers(0, 256, (19, 23)).astype(np.uint8)
    for ss in jp.PREDICTORS:
        f = m.encode_frame(img, 8, ss)
        h = m.parse(f)
        data = m.intervals_of(f[h["s0"]:h["s1"]], 1)[0]
        cost = jp.auto_cost(img, 8, ss)
        assert 8 * (len(data) + len(h["table"][1])) - 7 <= cost <= 8 * (len(data) + len(h["table"][1]))
        assert jp.sos_predictor(f) == ss == h["ss"]


def test_model_files_of_every_predictor_open_in_pillow():
    if not m.pillow_opens_sof3():
        pytest.skip("this Pillow's libjpeg does not open SOF3")
    from PIL import Image
    rasters = [x for x, P, _ in jp.planted().values() if P == 8]
    rasters += list(m.raster_cases(17, 65, 8, np.uint8).values())
    for k, img in enumerate(rasters):
        for ss in jp.PREDICTORS:
            for rr in (0, jp.RESTARTS[1 + (k + ss) % 3]):
                f = m.encode_frame(img, 8, ss, 0, rr)
                assert np.array_equal(np.array(Image.open(io.BytesIO(f))), img), (k, ss, rr)


def test_predictor_refusals_come_before_the_device(monkeypatch):
    import cct_hip
    from cct_hip import _ffi
    L = _ffi.lib()

    def touched(*a, **k):
        raise AssertionError("the device entry point was reached")

    img = np.zeros((4, 4), np.uint16)
    with monkeypatch.context() as mp:
        mp.setattr(L, "cct_jpegll_encode_batch", touched)
        mp.setattr(L, "cct_jpegll_encode_batch_sv", touched)
        for bad in (8, -1, 255, "best", "", "1", "AUTO"):
            with pytest.raises(ValueError):
                cct_hip.jpeg_lossless_encode_batch(img, predictor=bad)
        for bad in (True, False, 1.0, None, (1,), b"auto"):
            with pytest.raises(TypeError):
                cct_hip.jpeg_lossless_encode_batch(img, predictor=bad)
        with pytest.raises(TypeError):  # the checks of the older arguments come first, as they did
            cct_hip.jpeg_lossless_encode_batch(img, precision=12.0, predictor=8)
        for ok in (1, 7, np.int64(3), 0, "auto"):  # an empty batch passes every check and makes no call
            assert cct_hip.jpeg_lossless_encode_batch(np.zeros((0, 4, 4), np.uint16), predictor=ok) == []
        for ok in (1, 4, "auto"):  # and a good predictor reaches the entry point
            with pytest.raises(AssertionError, match="was reached"):
                cct_hip.jpeg_lossless_encode_batch(img, predictor=ok)


def test_the_sv_entry_point_is_declared_exported_and_refuses():
    from cct_hip import _ffi
    L = _ffi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "compact_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+cct_jpegll_encode_batch_sv\s*\(", text)
    assert "cct_jpegll_encode_batch_sv" in _ffi.exported_symbols() and hasattr(L, "cct_jpegll_encode_batch_sv")
    assert L.cct_version() == 1
    img = np.zeros((4, 4), np.uint16)
    stride = L.cct_jpegll_bound(4, 4, 0)
    out = np.zeros(stride, np.uint8)
    sizes, status, sel = np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint32)

    def sv(predictor, n=1, precision=16, stride=stride):
        return L.cct_jpegll_encode_batch_sv(img.ctypes.data, 0, n, 4, 4, 16, precision, predictor, 0, out.ctypes.data, stride,
                                            sizes.ctypes.data, status.ctypes.data, sel.ctypes.data)

    for bad in (8, -1):
        assert sv(bad) == E_ARG
        assert f"predictor {bad}" in _ffi.last_error()
        assert sv(bad, n=0) == E_ARG  # before the empty batch is waved through
    for good in range(8):  # the other whole-call refusals and the empty batch answer as they do for the old entry point
        assert sv(good, precision=17) == E_ARG and "precision 17" in _ffi.last_error()
        assert sv(good, stride=stride - 1) == 6
        assert sv(good, n=0) == 0
