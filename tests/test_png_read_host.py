"""The yardstick of the device PNG reader, on the CPU: every file the GPU tests use (tests/png_files.py) opens in Pillow to the
expected samples, Pillow refuses the damaged files it is known to refuse, and the reader's host-only parts (cct_png_info, the
argument checks of cct_png_read_batch / png_read_batch) answer before any device call."""
import ctypes as C
import hashlib
import io
import json
import os

import numpy as np
import pytest
from PIL import Image

import golden_inputs as gi
import png_files as pf
import png_model as pm


def _pillow(file):
    im = Image.open(io.BytesIO(file))
    im.load()
    return np.asarray(im).astype(np.uint16)


@pytest.mark.parametrize("rows", pf.ROWS)
def test_pillow_reads_the_edge_files(rows):
    for cols in pf.COLS:
        for name, f, img in pf.edge_batch(rows, cols):
            assert np.array_equal(_pillow(f), img), name


def test_pillow_reads_the_chunk_layer_files():
    for name, f, img in pf.chunk_cases() + [pf.big_idat_case()]:
        assert np.array_equal(_pillow(f), img), name


def test_pillow_reads_the_good_files_and_refuses_what_it_is_known_to_refuse():
    cases = {name: (f, img, st) for name, f, img, st in pf.damaged_cases()}
    for name, (f, img, st) in cases.items():
        if st == 0:
            assert np.array_equal(_pillow(f), img), name
    for name in ("data-byte-flipped", "filter-byte-5"):
        with pytest.raises(OSError):
            _pillow(cases[name][0])
    # where the reader is stricter than Pillow (12.2) on purpose: Pillow checks no CRC behind the image data, and it opens a
    # stream with bytes to spare or with a whole row missing without an error
    for name in ("ancillary-byte-flipped-behind-the-idats", "stream-61-long", "stream-one-row-short"):
        _pillow(cases[name][0])
    assert sorted({st for _, _, _, st in pf.damaged_cases()}) == [0, pf.E_ZLIB, pf.E_STREAM, pf.E_MIXED, pf.E_PNG, pf.E_CRC]


def test_the_reference_preview_is_what_the_model_writes():
    fx = json.load(open(os.path.join(gi.GOLDEN, "png.json")))["preview"]
    png = pm.png_bytes(gi.load_slice(fx["slice"]), fx["level"], fx["shift"])
    assert len(png) == fx["size"] and hashlib.sha256(png).hexdigest() == fx["sha256"]
    assert np.array_equal(_pillow(png) >> fx["shift"], gi.load_slice(fx["slice"]))


def test_png_info():
    import cct_hip
    from cct_hip import _ffi
    assert _ffi.E_PNG == 11 and _ffi.E_CRC == 12
    for name, f, img in pf.edge_batch(65, 300)[::7] + pf.chunk_cases():
        depth = 8 if "d8" in name or int(f[24]) == 8 else 16
        assert cct_hip.png_info(f) == (img.shape[0], img.shape[1], depth), name
    for name, f, _, st in pf.damaged_cases():
        refused = name in ("bad-signature", "ihdr-not-first", "depth-4", "interlace-1") or name.startswith("colour-type")
        if refused:
            with pytest.raises(ValueError):
                cct_hip.png_info(f)
        elif not name.startswith("truncated"):
            assert cct_hip.png_info(f)[2] in (8, 16), name
    L = _ffi.lib()
    r, c, d = C.c_int(0), C.c_int(0), C.c_int(0)
    good = pf.damaged_cases()[0][1]
    assert L.cct_png_info(good, 32, C.byref(r), C.byref(c), C.byref(d)) == _ffi.E_PNG  # shorter than signature + IHDR
    assert L.cct_png_info(None, 0, C.byref(r), C.byref(c), C.byref(d)) == _ffi.E_ARG
    with pytest.raises(TypeError):
        cct_hip.png_info("not bytes")


def test_argument_refusals_come_before_any_device_call():
    """These run on a machine without a GPU: a device call would return CCT_E_DEVICE."""
    import cct_hip
    from cct_hip import _ffi
    L = _ffi.lib()
    f = pf.damaged_cases()[0][1]
    rows, cols = pf.DAMAGED_SHAPE
    offs = np.array([0, len(f)], dtype=np.uint64)
    out = np.zeros(rows * cols, dtype=np.uint16)
    st = np.zeros(1, dtype=np.uint32)

    def call(n=1, rows=rows, cols=cols, shift=0, cap=out.size):
        return L.cct_png_read_batch(f, offs.ctypes.data, n, rows, cols, shift, out.ctypes.data, 0, cap, st.ctypes.data)
    assert call(shift=16) == _ffi.E_ARG and call(shift=-1) == _ffi.E_ARG
    assert call(rows=0) == _ffi.E_ARG and call(cols=0) == _ffi.E_ARG and call(n=-1) == _ffi.E_ARG
    assert call(rows=1 << 15, cols=1 << 15, cap=1 << 40) == _ffi.E_ARG  # rows * (1 + 2 cols) above 2^30 - 512
    assert call(cap=out.size - 1) == _ffi.E_CAP
    assert call(n=0) == _ffi.OK
    for kw in ({"shift": 16}, {"shift": -1}):
        with pytest.raises(ValueError):
            cct_hip.png_read_batch([f], **kw)
    for kw in ({"shift": 1.5}, {"shift": True}, {"out_dev": out}):
        with pytest.raises(TypeError):
            cct_hip.png_read_batch([f], **kw)
    with pytest.raises(TypeError):
        cct_hip.png_read_batch(f)
    with pytest.raises(TypeError):
        cct_hip.png_read_batch([f, "text"])
    with pytest.raises(ValueError):
        cct_hip.png_read_batch([b"not a png"])
    assert cct_hip.png_read_batch([]).shape == (0, 0, 0)
