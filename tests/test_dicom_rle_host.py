"""DICOM RLE Lossless without a device: the CPU model (tests/dicom_rle_model.py) against known answers written out by hand
and against libtiff's PackBits, the host-only encapsulation helpers of cct_hip, and the argument checks of
cct_dicom_rle_bound / _encode_batch / _decode_batch, which answer before any device call."""
import struct

import numpy as np
import pytest

import dicom_rle_model as m

needs_libtiff = pytest.mark.skipif(not m.have_libtiff(), reason="Pillow without libtiff: no second PackBits encoder")


def seq(n):
    """n bytes, no two neighbours equal"""
    return bytes(i % 256 for i in range(n))


def test_known_answers_equal_bytes():
    v = 7
    want = {1: [0, v], 2: [255, v], 128: [129, v], 129: [129, v, 0, v], 130: [129, v, 255, v], 256: [129, v, 129, v],
            257: [129, v, 129, v, 0, v]}
    for n, packets in want.items():
        assert m.encode_row(bytes([v]) * n) == bytes(packets), n


def test_known_answers_distinct_bytes():
    s = seq(257)
    assert m.encode_row(s[:128]) == bytes([127]) + s[:128]
    assert m.encode_row(s[:129]) == bytes([127]) + s[:128] + bytes([0]) + s[128:129]
    assert m.encode_row(s) == bytes([127]) + s[:128] + bytes([127]) + s[128:256] + bytes([0]) + s[256:]


def test_known_answers_single_literal_between_runs():
    assert m.encode_row(b"aab") == bytes([255, 97, 0, 98])
    assert m.encode_row(b"aabcc") == bytes([255, 97, 0, 98, 255, 99])
    assert m.encode_row(b"abb") == bytes([0, 97, 255, 98])


def test_known_answer_rows_do_not_merge():
    img = np.array([[1, 2, 3, 3], [3, 3, 4, 5]], np.uint8)
    seg = bytes([1, 1, 2, 255, 3, 255, 3, 1, 4, 5])
    assert m.encode_frame(img) == struct.pack("<16I", 1, 64, *([0] * 14)) + seg
    img16 = np.array([[0x0101, 0x0102]], np.uint16)  # high plane 1 1 -> (255, 1), low plane 1 2 -> (1, 1, 2) and a pad byte
    assert m.encode_frame(img16) == struct.pack("<16I", 2, 64, 66, *([0] * 13)) + bytes([255, 1, 1, 1, 2, 0])


@pytest.mark.parametrize("bits", [8, 16])
def test_model_round_trip(bits):
    for rows in m.ROWS:
        for cols in m.COLS:
            for name, img in m.raster_cases(rows, cols, bits).items():
                frame = m.encode_frame(img)
                assert len(frame) % 2 == 0
                back = m.decode_frame(frame, rows, cols, bits)
                assert back.dtype == img.dtype and np.array_equal(back, img), (rows, cols, name)


def test_model_decoder_rules():
    # no-ops, a literal across a row end, a run across a row end, spare bytes, a literal cut by the segment end
    seg = bytes([128, 2, 1, 2, 3, 128, 253, 9, 128, 0, 4]) + bytes([77, 77, 77])
    assert m.decode_segment(seg, 8) == bytes([1, 2, 3, 9, 9, 9, 9, 4])
    assert m.decode_segment(bytes([5, 1, 2, 3]), 3) == bytes([1, 2, 3])
    assert m.decode_segment(bytes([1, 1, 2, 250]), 2) == bytes([1, 2])  # a replicate header without its byte writes nothing
    with pytest.raises(ValueError):
        m.decode_segment(bytes([1, 1, 2, 250]), 3)
    with pytest.raises(ValueError):
        m.decode_frame(b"\0" * 10, 1, 1, 8)


@needs_libtiff
@pytest.mark.parametrize("bits", [8, 16])
def test_model_decoder_reads_libtiff_frames(bits):
    differs = 0
    for rows, cols in ((1, 1), (2, 65), (3, 300), (8, 300)):
        for name, img in m.raster_cases(rows, cols, bits).items():
            frame = m.libtiff_frame(img)
            differs += frame != m.encode_frame(img)
            assert np.array_equal(m.decode_frame(frame, rows, cols, bits), img), (rows, cols, name)
    assert differs, "libtiff wrote the model's packets everywhere: not a second encoder"


def test_pydicom_encoder_agrees():
    try:
        from pydicom.pixel_data_handlers.rle_handler import rle_encode_frame
    except ImportError:
        pytest.skip("pydicom is not installed: the encoder rule is checked against the hand-written answers only")
    for rows, cols in ((1, 1), (2, 129), (3, 300)):
        for bits in (8, 16):
            for name, img in m.raster_cases(rows, cols, bits).items():
                assert bytes(rle_encode_frame(img)) == m.encode_frame(img), (rows, cols, bits, name)


def test_encapsulate_and_fragments():
    import cct_hip
    frames = [b"", b"ab", b"abc", bytes(range(64)) + b"\x01"]
    for enc, frag in ((m.encapsulate, m.fragments), (cct_hip.dicom_encapsulate, cct_hip.dicom_fragments)):
        pd = enc(frames)
        assert len(pd) % 2 == 0 and pd.endswith(m.SEQ_DELIM)
        assert pd[:4] == m.ITEM_TAG and struct.unpack("<I", pd[4:8])[0] == 4 * len(frames)
        assert struct.unpack("<4I", pd[8:24]) == (0, 8, 18, 30)  # item heads count, odd fragments are padded
        back = frag(pd)
        assert back == [f + b"\0" * (len(f) & 1) for f in frames]
    assert cct_hip.dicom_encapsulate(frames) == m.encapsulate(frames)
    one = m.encode_frame(np.array([[1, 2, 3]], np.uint8))
    assert cct_hip.dicom_fragments(cct_hip.dicom_encapsulate([one])) == [one]
    assert cct_hip.dicom_fragments(cct_hip.dicom_encapsulate([])) == []


def test_fragments_refuses_malformed_items():
    import cct_hip
    good = m.encapsulate([b"abcd", b"ef"])
    bad = [good[:-8],                                                    # no sequence delimiter
           good + b"\0\0",                                               # bytes behind it
           good[:-4] + b"\x02\0\0\0",                                    # a delimiter with a length
           b"\xfe\xff\x00\xe1" + good[4:],                               # an unknown tag
           good[:20] + b"\xff\xff\xff\x7f" + good[24:],                  # an item running past the data
           m.SEQ_DELIM,                                                  # no Basic Offset Table
           m.ITEM_TAG + struct.pack("<I", 4) + b"\0\0\0\0" + good[16:],  # a table of one offset for two fragments
           good[:12] + struct.pack("<I", 10) + good[16:],                # a table that points elsewhere
           good[:3]]
    for k, d in enumerate(bad):
        for frag in (m.fragments, cct_hip.dicom_fragments):
            if k == 7 and frag is m.fragments:
                continue  # the model does not read the offsets
            with pytest.raises(ValueError):
                frag(d)
    with pytest.raises(TypeError):
        cct_hip.dicom_fragments("text")
    with pytest.raises(TypeError):
        cct_hip.dicom_encapsulate(b"one frame, not a list")


def test_whole_call_refusals_answer_without_a_device():
    from cct_hip import _ffi
    L = _ffi.lib()
    img = np.zeros((2, 4, 4), np.uint16)
    out = np.zeros((2, 4096), np.uint8)
    sizes = np.zeros(2, np.uint32)
    status = np.zeros(2, np.uint32)
    offs = np.array([0, 70, 140], np.uint64)
    frames = np.zeros(140, np.uint8)

    def enc(n=2, rows=4, cols=4, bits=16, stride=4096):
        return L.cct_dicom_rle_encode_batch(img.ctypes.data, 0, n, rows, cols, bits, out.ctypes.data, stride, sizes.ctypes.data)

    def dec(n=2, rows=4, cols=4, bits=16, cap=32):
        return L.cct_dicom_rle_decode_batch(frames.ctypes.data, offs.ctypes.data, n, rows, cols, bits, img.ctypes.data, 0, cap,
                                            status.ctypes.data)

    for call in (enc, dec):
        for bits in (0, 1, 12, 24, 32):
            assert call(bits=bits) == _ffi.E_ARG
        assert call(rows=0) == _ffi.E_ARG and call(cols=0) == _ffi.E_ARG and call(rows=-3) == _ffi.E_ARG
        assert call(n=-1) == _ffi.E_ARG
        assert call(rows=8192, cols=8193) == _ffi.E_ARG  # rows * cols above 2^26
        assert b"DICOM RLE" in L.cct_last_error()
    assert L.cct_dicom_rle_bound(4, 4, 16) == 64 + 2 * 2 * 16 and L.cct_dicom_rle_bound(4, 4, 8) == 64 + 2 * 16
    assert enc(stride=L.cct_dicom_rle_bound(4, 4, 16) - 1) == _ffi.E_CAP
    assert dec(cap=31) == _ffi.E_CAP and dec(cap=0) == _ffi.E_CAP
    for args in ((0, 4, 16), (4, 0, 16), (4, 4, 12), (8192, 8193, 8)):
        assert L.cct_dicom_rle_bound(*args) == 0
    assert L.cct_dicom_rle_bound(8192, 8192, 16) == 64 + 4 * (1 << 26)
    assert enc(n=0) == _ffi.OK and dec(n=0) == _ffi.OK  # nothing to do: no device either


@pytest.mark.parametrize("bits", [8, 16])
def test_bound_covers_the_adversarial_rows(bits):
    from cct_hip import _ffi
    L = _ffi.lib()
    worst = 0.0
    for rows in m.ROWS + (40,):
        for cols in m.COLS:
            bound = L.cct_dicom_rle_bound(rows, cols, bits)
            for name, img in m.raster_cases(rows, cols, bits).items():
                n = len(m.encode_frame(img))
                assert n <= bound, (rows, cols, name)
                worst = max(worst, n / bound)
    assert worst == 1.0  # rows of one byte reach it: the bound is tight


def test_python_argument_checks():
    import cct_hip
    with pytest.raises(TypeError):
        cct_hip.dicom_rle_encode_batch(np.zeros((1, 4, 4), np.float32))
    with pytest.raises(ValueError):
        cct_hip.dicom_rle_encode_batch(np.zeros((4,), np.uint16))
    with pytest.raises(ValueError):
        cct_hip.dicom_rle_encode_batch(np.zeros((1, 0, 4), np.uint16))
    with pytest.raises(ValueError):
        cct_hip.dicom_rle_encode_batch(np.zeros((1, 4, 4), np.uint16), shape=(1, 4, 4))
    assert cct_hip.dicom_rle_encode_batch(np.zeros((0, 4, 4), np.uint16)) == []
    with pytest.raises(ValueError):
        cct_hip.dicom_rle_decode_batch([b""], 4, 4, bits=12)
    with pytest.raises(ValueError):
        cct_hip.dicom_rle_decode_batch([b""], 0, 4)
    with pytest.raises(TypeError):
        cct_hip.dicom_rle_decode_batch(b"frame", 4, 4)
    with pytest.raises(TypeError):
        cct_hip.dicom_rle_decode_batch(["frame"], 4, 4)
    with pytest.raises(TypeError):
        cct_hip.dicom_rle_decode_batch([b""], 4.0, 4)
    res, st = cct_hip.dicom_rle_decode_batch([], 4, 4, bits=8, raise_errors=False)
    assert res.shape == (0, 4, 4) and res.dtype == np.uint8 and st.size == 0
