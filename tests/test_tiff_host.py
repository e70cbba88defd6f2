"""tests/tiff_model.py against Pillow / libtiff, and what the TIFF entry points decide without a device: the model's files
are Pillow's byte for byte, its reader returns Pillow's raster for every foreign file, its verdict on every damaged file is
Pillow's, the census of LZW edges holds, and arguments and structure are refused on the host (the C parser is the model's)."""
import functools
import struct

import numpy as np
import pytest

import tiff_model as m


@functools.lru_cache(maxsize=None)
def cases():
    return m.raster_cases()


@pytest.mark.parametrize("compression", ["lzw", "deflate"])
@pytest.mark.parametrize("predictor", [1, 2])
def test_model_files_equal_pillows(compression, predictor):
    strips = set()
    for name, a, rpss in cases():
        for rps in rpss:
            f = m.write_file(a, compression, predictor, rps)
            assert m.same_file(f, m.pillow_file(a, compression, predictor, rps)), (name, rps)
            strips.add(len(m.parse(f)["offs"]))
            back = m.read(f, a.shape[0], a.shape[1], 8 * a.dtype.itemsize)
            assert isinstance(back, np.ndarray) and back.dtype == a.dtype and np.array_equal(back, a), (name, rps)
    assert {1, 2, 3} <= strips and max(strips) >= 37  # inline counts, two SHORTs inline, SHORT arrays


def test_byte_counts_are_short_below_6553_strip_bytes():
    by_name = {name: a for name, a, _ in cases()}
    ifd = lambda f: struct.unpack_from("<I", f, 4)[0]
    for name, typ in (("2x6552_u8", 3), ("2x6553_u8", 4), ("smooth_37x50", 3)):
        f = m.write_file(by_name[name], "lzw", 1, 1)
        assert struct.unpack_from("<HH", f, ifd(f) + 2 + 12 * 7) == (279, typ), name
    a = np.random.default_rng(1).integers(0, 65536, (96, 512)).astype(np.uint16)
    a[64:] = 7  # strips of 64 rows: one above 65535 coded bytes, one far below
    f = m.write_file(a, "lzw")
    counts = m.parse(f)["counts"]
    assert max(counts) > 0xFFFF > min(counts)
    assert m.same_file(f, m.pillow_file(a, "lzw"))


def test_model_reads_every_foreign_file_as_pillow_does():
    files = m.foreign_files()
    assert len(files) >= 80
    for name, f, a in files:
        back = m.read(f, a.shape[0], a.shape[1], 8 * a.dtype.itemsize)
        assert isinstance(back, np.ndarray) and np.array_equal(back, a), name
        p = m.pillow_read(f)
        assert isinstance(p, np.ndarray) and np.array_equal(p, a), name


def test_model_verdict_on_damaged_files_is_pillows():
    seen = set()
    for name, f, a in m.damaged_files():
        got, p = m.read(f, a.shape[0], a.shape[1], 8 * a.dtype.itemsize), m.pillow_read(f)
        if isinstance(got, str):
            assert got in ("CCT_E_STREAM", "CCT_E_ZLIB") and isinstance(p, str) and p == "OSError", (name, got)
            seen.add(got)
        else:
            assert isinstance(p, np.ndarray) and np.array_equal(got, p), name
            seen.add("OK" if np.array_equal(got, a) else "other bytes")
    assert seen == {"CCT_E_STREAM", "CCT_E_ZLIB", "OK", "other bytes"}


def test_census_of_lzw_edges():
    edge = m.edge_strips()
    c = m.census([s for _, s in edge])
    assert {254, 766, 1790, 3836} <= c["last_code"]       # EOI at each new width, and behind a Clear
    assert c["eoi_widths"] == {9, 10, 11, 12}
    assert c["eoi_after_clear"] >= 1 and c["one_code_after_clear"] >= 1 and c["clears"] >= 3
    assert c["bit_residues"] == set(range(8)) and c["dword_straddles"] > 1000
    # the raster cases: table-full Clears in the noise strip, long strings in the flat and periodic ones
    by_name = {name: a for name, a, _ in cases()}
    noise = m.census([m.strips_of(by_name["noise_16x512"], 1, 16)[0][0]])
    assert noise["clears"] >= 3 and noise["ratio_clears"] == 0
    assert m.census([m.strips_of(by_name["ratio_48x512_u8"], 1, 48)[0][0]])["ratio_clears"] == 1  # libtiff's compression-ratio Clear
    for name in ("flat_64x512", "periodic_64x512"):
        strip = m.strips_of(by_name[name], 1, None)[0][0]
        assert len(m.lzw_encode(strip)) * 20 < len(strip)
    odd = {len(m.write_file(a, "lzw", 1, rps)) & 1 for name, a, rpss in cases() for rps in rpss}
    pads = {sum(len(s) for s in map(m.lzw_encode, m.strips_of(a, 1, rps)[0])) & 1 for name, a, rpss in cases() for rps in rpss}
    assert odd == {0} and pads == {0, 1}                   # the IFD's pad byte occurred and every file ends even


def test_lzw_decoder_rules_one_by_one():
    s = bytes(range(40)) * 3
    codes = m.lzw_codes(s)
    assert m.lzw_decode(m.pack_codes(codes), len(s)) == ("OK", s)
    assert m.lzw_decode(m.pack_codes(codes[:-1]), len(s)) == ("OK", s)                         # no EOI
    assert m.lzw_decode(m.pack_codes(codes) + b"\xff\xff", len(s)) == ("OK", s)                # trailing bytes
    assert m.lzw_decode(m.pack_codes(codes), len(s) - 1) == ("OK", s[:-1])                     # the last string is cut
    assert m.lzw_decode(m.pack_codes(codes), len(s) + 1)[0] == "CCT_E_STREAM"                  # EOI ends it early
    assert m.lzw_decode(m.pack_codes(codes[:-2]), len(s))[0] == "CCT_E_STREAM"                 # the data ends early
    assert m.lzw_decode(m.pack_codes([(m.CLEAR, 9)] * 4 + codes[1:]), len(s)) == ("OK", s)     # repeated Clears
    assert m.lzw_decode(m.pack_codes(codes[1:]), len(s))[0] == "CCT_E_STREAM"                  # no opening Clear
    assert m.lzw_decode(m.pack_codes([(m.CLEAR, 9), (258, 9)]), 1)[0] == "CCT_E_STREAM"        # not a literal after a Clear
    kwkwk = [(m.CLEAR, 9), (65, 9), (258, 9), (259, 9)]                                        # A, AA, AAA
    assert m.lzw_decode(m.pack_codes(kwkwk), 6) == ("OK", b"AAAAAA")
    assert m.lzw_decode(m.pack_codes([(m.CLEAR, 9), (65, 9), (259, 9)]), 6)[0] == "CCT_E_STREAM"  # beyond the next free entry


def test_parser_of_the_library_is_the_models():
    import cct_hip
    for name, f, a in m.foreign_files() + m.damaged_files():
        assert cct_hip.tiff_info(f) == m.info(f) == (a.shape[0], a.shape[1], 8 * a.dtype.itemsize), name
    for name, a, rpss in cases():
        assert cct_hip.tiff_info(m.write_file(a, "deflate", 2, rpss[-1])) == (a.shape[0], a.shape[1], 8 * a.dtype.itemsize)
    for name, f in m.refused_files():
        assert m.read(f) == "CCT_E_TIFF", name
        with pytest.raises(ValueError):
            cct_hip.tiff_info(f)
    for name, f in m.short_uncompressed_files():
        assert m.read(f) == "CCT_E_STREAM" and cct_hip.tiff_info(f) == m.info(f), name
    with pytest.raises(TypeError):
        cct_hip.tiff_info("text")


def test_arguments_are_refused_before_any_device_call():
    import cct_hip
    a = np.zeros((2, 4, 4), np.uint16)
    enc, rd = cct_hip.tiff_encode_batch, cct_hip.tiff_read_batch
    for kw in (dict(compression="packbits"), dict(compression=5), dict(predictor=3), dict(predictor=0), dict(compression="none", predictor=2),
               dict(rows_per_strip=0), dict(rows_per_strip=-2), dict(compression="deflate", level=3), dict(compression="deflate", level=10),
               dict(compression="deflate", level=0), dict(shape=(2, 4, 4)), dict(dtype=np.uint16)):
        with pytest.raises(ValueError):
            enc(a, **kw)
    for kw in (dict(predictor=1.5), dict(rows_per_strip="7"), dict(level=None), dict(predictor=True)):
        with pytest.raises(TypeError):
            enc(a, **kw)
    for bad in (a.astype(np.int16), a.astype(np.float32), a.astype(np.uint32)):
        with pytest.raises(TypeError):
            enc(bad)
    with pytest.raises(ValueError):
        enc(np.zeros((2, 2, 2, 2), np.uint16))
    with pytest.raises(ValueError):
        enc(np.zeros((1, 1, 65536), np.uint8))
    assert enc(np.zeros((0, 4, 4), np.uint16)) == []
    assert enc(a[:0], compression="lzw", level=99) == []  # level is Deflate's
    good = m.write_file(a[0], "lzw")
    for args in ((0, 4), (4, 0), (65536, 4), (4, 65536)):
        with pytest.raises(ValueError):
            rd([good], *args)
    with pytest.raises(ValueError):
        rd([good], 4, 4, bits=12)
    with pytest.raises(TypeError):
        rd(good, 4, 4)
    with pytest.raises(TypeError):
        rd(["text"], 4, 4)
    with pytest.raises(TypeError):
        rd([good], 4.0, 4)
    with pytest.raises(TypeError):
        rd([good], 4, 4, out_dev=np.zeros(16, np.uint16))
    out = rd([], 4, 4)
    assert out.shape == (0, 4, 4) and out.dtype == np.uint16
    out, status = rd([], 4, 4, bits=8, raise_errors=False)
    assert out.shape == (0, 4, 4) and out.dtype == np.uint8 and status.size == 0


def test_whole_call_refusals_of_the_c_abi_answer_without_a_device():
    from cct_hip import _ffi
    L = _ffi.lib()
    img = np.zeros((2, 4, 4), np.uint16)
    out = np.zeros((2, 4096), np.uint8)
    sizes, status = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    f = m.write_file(img[0], "lzw")
    files = np.frombuffer(f + f, np.uint8)
    offs = np.array([0, len(f), 2 * len(f)], np.uint64)

    def enc(n=2, rows=4, cols=4, bits=16, comp=5, pred=1, rps=0, level=6, stride=4096):
        return L.cct_tiff_encode_batch(img.ctypes.data, 0, n, rows, cols, bits, comp, pred, rps, level, out.ctypes.data, stride, sizes.ctypes.data)

    def dec(n=2, rows=4, cols=4, bits=16, cap=32):
        return L.cct_tiff_read_batch(files.ctypes.data, offs.ctypes.data, n, rows, cols, bits, img.ctypes.data, 0, cap, status.ctypes.data)

    for call in (enc, dec):
        for bits in (0, 1, 12, 32):
            assert call(bits=bits) == _ffi.E_ARG
        assert call(rows=0) == _ffi.E_ARG and call(cols=0) == _ffi.E_ARG and call(rows=65536) == _ffi.E_ARG and call(cols=-1) == _ffi.E_ARG
        assert b"TIFF" in L.cct_last_error()
        assert call(n=-1) == _ffi.E_ARG
    for kw in (dict(comp=2), dict(comp=32773), dict(pred=0), dict(pred=3), dict(comp=1, pred=2), dict(rps=-1), dict(comp=8, level=3),
               dict(comp=8, level=10)):
        assert enc(**kw) == _ffi.E_ARG, kw
    assert enc(stride=L.cct_tiff_bound(4, 4, 16, 5, 0) - 1) == _ffi.E_CAP
    assert dec(cap=31) == _ffi.E_CAP
    assert enc(n=0) == _ffi.OK and dec(n=0) == _ffi.OK
    for args in ((0, 4, 16, 5, 0), (4, 0, 16, 5, 0), (4, 4, 12, 5, 0), (4, 4, 16, 7, 0), (4, 4, 16, 5, -1), (65535, 65535, 16, 1, 0)):
        assert L.cct_tiff_bound(*args) == 0
    assert L.cct_tiff_info(f, len(f), None, None, None) == _ffi.E_ARG
    assert _ffi.E_TIFF == 15


@pytest.mark.parametrize("compression", ["none", "lzw", "deflate"])
def test_bound_covers_the_model_files(compression):
    from cct_hip import _ffi
    L = _ffi.lib()
    r = np.random.default_rng(2)
    for name, a, rpss in cases() + [("noise_u8", r.integers(0, 256, (40, 333)).astype(np.uint8), [None, 1, 3])]:
        for rps in rpss:
            bound = L.cct_tiff_bound(a.shape[0], a.shape[1], 8 * a.dtype.itemsize, m.COMPRESSION[compression], rps or 0)
            assert 0 < len(m.write_file(a, compression, 1, rps)) <= bound, (name, rps)
