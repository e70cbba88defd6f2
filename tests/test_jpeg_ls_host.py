"""tests/jpeg_ls_model.py alone, no device: the worked example of T.87 Annex H.3 byte for byte, the threshold defaults,
round trips over raster_cases and census_cases, and a census of what the coder went through on them."""
import functools

import numpy as np
import pytest

import jpeg_ls_model as m


@functools.lru_cache(maxsize=None)
def coded():
    """[(tag, raster, precision, restart rows, file)] over every case, and the census of encoding them all"""
    census, out = m.new_census(), []
    for rows in m.ROWS:
        for cols in m.COLS:
            for p in m.PRECISIONS:
                for name, x in m.raster_cases(rows, cols, p).items():
                    for rr in m.RESTARTS:
                        out.append(((rows, cols, p, name, rr), x, p, rr, m.encode_frame(x, p, rr, census=census)))
    for name, (x, p) in m.census_cases().items():
        for rr in m.RESTARTS:
            out.append(((name, rr), x, p, rr, m.encode_frame(x, p, rr, census=census)))
    return out, census


def test_annex_h3_byte_for_byte():
    assert m.encode_frame(m.H3_RASTER, 8) == m.H3_FILE
    assert np.array_equal(m.decode_frame(m.H3_FILE, 4, 4, 8), m.H3_RASTER)
    assert m.info(m.H3_FILE) == (4, 4, 8)


def test_default_thresholds():
    assert m.default_thresholds(255) == (3, 7, 21)
    assert m.default_thresholds(4095) == (18, 67, 276)
    assert m.default_thresholds(65535) == (18, 67, 276)
    assert m.default_thresholds(3) == (2, 3, 3)
    p = m.Params(16)
    assert (p.range, p.qbpp, p.limit, p.a0, p.reset) == (65536, 16, 64, 1024, 64)
    p = m.Params(2)
    assert (p.range, p.qbpp, p.limit, p.a0) == (4, 2, 20, 2)


def test_round_trips():
    files, _ = coded()
    for tag, x, p, rr, f in files:
        assert np.array_equal(m.decode_frame(f, *x.shape, 8 if p <= 8 else 16), x), tag
        assert m.info(f) == (*x.shape, p)


def test_census_every_branch_is_reached():
    _, census = coded()
    missing = [k for k in m.CENSUS if census[k] == 0]
    assert not missing, census


def test_restart_intervals_are_independent():
    """an interval's bytes are those of its lines coded as a file of their own"""
    x = m.raster_cases(17, 65, 12)["spikes"]
    f = m.encode_frame(x, 12, 5)
    h = m.parse(f)
    assert h["ri"] == 5 and h["rst"] == [0, 1, 2] and len(h["intervals"]) == 4
    for k, (a, b) in enumerate(h["intervals"]):
        alone = m.encode_frame(x[5 * k:5 * k + 5], 12)
        assert f[a:b] == alone[m.parse(alone)["intervals"][0][0]:-2], k


def test_lse_parameters_round_trip():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 201, (9, 70)).astype(np.uint8)
    x[3:5] = 77
    for lse in (dict(maxval=200), dict(maxval=255, t1=5, t2=9, t3=30), dict(reset=3), dict(maxval=200, t1=1, t2=1, t3=1, reset=255)):
        f = m.encode_frame(x, 8, 2, lse=lse)
        assert f != m.encode_frame(x, 8, 2) and b"\xff\xf8" in f
        assert np.array_equal(m.decode_frame(f, 9, 70, 8), x), lse
    y = rng.integers(0, 1001, (5, 33)).astype(np.uint16)  # RANGE 1001 is no power of two
    f = m.encode_frame(y, 12, lse=dict(maxval=1000))
    assert np.array_equal(m.decode_frame(f, 5, 33), y)


@pytest.mark.parametrize("name,damage,kind", [
    ("no SOI", lambda f: b"\x00" + f[1:], "JPEGLS"),
    ("SOF3 instead", lambda f: f.replace(b"\xff\xf7", b"\xff\xc3", 1), "JPEGLS"),
    ("two components", lambda f: f[:4] + b"\x00\x0e" + f[6:11] + b"\x02\x01\x11\x00\x02\x11\x00" + f[15:], "JPEGLS"),
    ("NEAR 1", lambda f: f[:f.index(b"\xff\xda") + 7] + b"\x01" + f[f.index(b"\xff\xda") + 8:], "JPEGLS"),
    ("ILV 1", lambda f: f[:f.index(b"\xff\xda") + 8] + b"\x01" + f[f.index(b"\xff\xda") + 9:], "JPEGLS"),
    ("LSE id 2", lambda f: f[:15] + b"\xff\xf8\x00\x05\x02\x01\x01" + f[15:], "JPEGLS"),
    ("LSE T1 above T2", lambda f: f[:15] + b"\xff\xf8\x00\x0d\x01\x00\xff\x00\x09\x00\x05\x00\x1e\x00\x40" + f[15:], "JPEGLS"),
    ("no EOI", lambda f: f[:-2], "JPEGLS"),
    ("COM and APP8 ride along", lambda f: f[:2] + b"\xff\xfe\x00\x05abc\xff\xe8\x00\x04\x01\x02" + f[2:], 0),
    ("DRI of 6 bytes", lambda f: f.replace(b"\xff\xdd\x00\x04\x00\x02", b"\xff\xdd\x00\x06\x00\x00\x00\x02"), 0),
    ("bytes behind EOI", lambda f: f + b"\x00\x00", 0),
    ("other shape", lambda f: f[:7] + b"\x00\x08" + f[9:], "MIXED"),
    ("RST renumbered", lambda f: f.replace(b"\xff\xd1", b"\xff\xd2"), "STREAM"),
    ("RST removed", lambda f: f.replace(b"\xff\xd1", b""), "STREAM"),
    ("cut", lambda f: f[:-12] + f[-2:], "STREAM"),
    ("a zero byte left over", lambda f: f[:-2] + b"\x00" + f[-2:], "STREAM"),
])
def test_reader_verdicts(name, damage, kind):
    x = m.raster_cases(5, 63, 8)["spikes"]
    f = damage(m.encode_frame(x, 8, 2))
    if kind == 0:
        assert np.array_equal(m.decode_frame(f, 5, 63, 8), x)
    else:
        with pytest.raises(m.JlsError) as e:
            m.decode_frame(f, 5, 63, 8)
        assert e.value.kind == kind, str(e.value)
