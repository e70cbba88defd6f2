"""CPU checks of the zlib level surface of the DEFLATE stage: config['encoder']['deflate_level'] -> the
CCT_FLAG_DEFLATE_LEVEL field, refusals before any device call, and the header / ABI declarations."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_inputs as gi


def _cfg(level=None):
    import cct_hip
    cfg = copy.deepcopy(cct_hip.default_config())
    if level is not None:
        cfg["encoder"]["deflate_level"] = level
    return cfg


def test_codec_params_maps_deflate_level():
    from cct_hip import _ffi, codec_params
    base = codec_params(_cfg())[0]
    assert base & _ffi.FLAG_LEVEL_MASK == 0  # absent: field 0 = level 9, the flags every existing caller sends
    assert codec_params(_cfg(-1))[0] == base | (6 << 8)
    for level in range(4, 10):
        flags = codec_params(_cfg(level))[0]
        assert flags == base | (level << 8) == base | _ffi.flag_deflate_level(level)
    assert codec_params(_cfg(9), np.int16)[0] == base | _ffi.FLAG_SIGNED_SEG | (9 << 8)


@pytest.mark.parametrize("level", [0, 1, 2, 3, 10, 15, -2, "6", 6.0, True])
def test_bad_levels_raise_value_error_before_the_device(level):
    import cct_hip
    with pytest.raises(ValueError):
        cct_hip.codec_params(_cfg(level))
    img = np.zeros((1, 16, 16), dtype=np.uint16)
    with pytest.raises(ValueError):
        cct_hip.encode_batch(img, _cfg(level))
    if not isinstance(level, (str, float, bool)):
        with pytest.raises(ValueError):
            cct_hip.zlib_compress_batch([b"abc"], level=level)


@pytest.mark.parametrize("level", [3, 10, 0, -2])
def test_zlib_compress_batch_level_refuses_without_a_gpu(level):
    from cct_hip import _ffi
    L = _ffi.lib()
    data = b"abcabcabc"
    offs = np.array([0, len(data)], dtype=np.uint64)
    out = np.zeros(4096, dtype=np.uint8)
    sizes = np.zeros(1, dtype=np.uint32)
    rc = L.cct_zlib_compress_batch_level(data, offs.ctypes.data, 1, level, out.ctypes.data, out.size, sizes.ctypes.data)
    assert rc == _ffi.E_ARG
    msg = _ffi.last_error()
    assert str(level) in msg
    if 0 <= level <= 3:
        assert "deflate_stored / deflate_fast: not on the device" in msg


@pytest.mark.parametrize("field", [1, 2, 3, 10, 15])
def test_encode_refuses_level_fields_without_a_gpu(field):
    from cct_hip import _ffi
    L = _ffi.lib()
    img = np.zeros((1, 16, 16), dtype=np.uint16)
    out = np.zeros(1 << 16, dtype=np.uint8)
    sizes, status, psz = (np.zeros(1, dtype=np.uint32) for _ in range(3))
    flags = _ffi.FLAG_DEFLATE | _ffi.FLAG_FRACTAL | _ffi.FLAG_SEGMENTATION | (field << 8)
    rc = L.cct_encode_batch(img.ctypes.data, 0, 1, 16, 16, 16, flags, -1, b"\0\0\0\0", 1, 2, out.ctypes.data, out.size,
                            sizes.ctypes.data, status.ctypes.data, psz.ctypes.data, None)
    assert rc == _ffi.E_ARG
    assert "level" in _ffi.last_error()


def test_header_declares_the_level_surface():
    text = open(os.path.join(gi.ROOT, "include", "compact_hip.h")).read()
    assert re.search(r"#define CCT_FLAG_DEFLATE_LEVEL\(l\) \(\(\(\(uint32_t\)\(l\)\) & 15u\) << 8\)", text)
    assert re.search(r"#define CCT_FLAG_LEVEL_MASK 0xF00u", text)
    assert "int cct_zlib_compress_batch_level(const uint8_t *h_in, const uint64_t *h_offsets, int n, int level," in text
    assert re.search(r"#define CCT_ABI_VERSION 1\b", text)
    from cct_hip import _ffi
    assert "cct_zlib_compress_batch_level" in _ffi.exported_symbols()
    assert hasattr(_ffi.lib(), "cct_zlib_compress_batch_level")
    assert C.c_int == _ffi._SIGS["cct_zlib_compress_batch_level"][0]
