"""tests/jpeg2000_decode_model.py, the CPU statement of the device JPEG 2000 lossless decoder: it inverts the encoder model, it
decodes OpenJPEG's own files to the rasters Pillow returns, it refuses what is out of scope, and it reads the hand-built files."""
import numpy as np
import pytest

import jpeg2000_decode_model as d
import jpeg2000_model as m


def needs_pillow():
    if not d.pillow_has_jpeg2000():
        pytest.skip("this Pillow has no JPEG 2000 codec")


@pytest.mark.parametrize("precision", sorted(m.PRECISIONS))
def test_inverts_the_encoder_model(precision):
    bits = 8 if precision == 8 else 16
    for rows, cols, cb, levels, names, imgs, files in m.matrix(precision):
        for name, x, f in zip(names, imgs, files):
            got = d.decode(f, rows, cols, bits)
            assert not isinstance(got, str) and got.dtype == x.dtype and np.array_equal(got, x), (rows, cols, cb, levels, name, got)


def test_inverts_the_phantoms_shift_and_jp2():
    for img, kw, f in m.phantoms():
        got = d.decode(f, 128, 128, 16, kw.get("shift", 0))
        assert not isinstance(got, str) and np.array_equal(got, img), kw


def test_openjpegs_own_files():
    needs_pillow()
    seen = set()
    for name, f, want in d.foreign_set():
        P = d.walk(f)
        seen.add((P["levels"], P["xcb"], P["ycb"], P["layers"], P["seq"]))
        got = d.decode(f, 70, 130, 8 * want.itemsize)
        assert not isinstance(got, str) and got.dtype == want.dtype and np.array_equal(got, want), (name, got)
    # what the variants were chosen for: three codings, three layers in both packet sequences, one layer resolution-major
    assert {(5, 6, 6, 1, 0), (2, 4, 6, 1, 0), (1, 2, 2, 1, 0), (5, 6, 6, 3, 0), (5, 6, 6, 3, 1), (5, 6, 6, 1, 1)} <= seen
    files = dict((name, f) for name, f, _ in d.foreign_set())
    assert b"\xff\x58" in files["PLT and COM"] and b"hello" in files["PLT and COM"] and files["JP2"][4:8] == b"jP  "


def test_files_out_of_scope_are_refused():
    names = [name for name, _ in d.refused_set()]
    assert "SOP" in names and (not d.pillow_has_jpeg2000() or names == ["precincts", "9/7", "tiles", "RGB", "SOP"])
    for name, f in d.refused_set():
        assert d.decode(f, 70, 130) == "CCT_E_J2K", name
    base = d.handbuilt_set()[0]
    assert d.decode(base[1], 33, 64) == d.decode(base[1], 33, 65, bits=8) == "CCT_E_MIXED"


def test_hand_built_files():
    for name, f, want in d.handbuilt_set():
        got = d.decode(f, 33, 65)
        assert not isinstance(got, str) and np.array_equal(got, want), (name, got)
    files = dict((name, f) for name, f, _ in d.handbuilt_set())
    one = files["one guard bit"]
    at = one.index(b"\xff\x5c")
    assert one[at + 4] == 1 << 5 and one[at + 5] >> 3 == 17  # Kakadu's default: the exponents one higher than with two guard bits
    assert d.walk(one)["mb"] == d.walk(files["Psot 0"])["mb"] == [17, 18, 18, 19, 18, 18, 19]
    assert files["COM in the tile-part header"].index(b"\xff\x64") > files["COM in the tile-part header"].index(b"\xff\x90")
    assert files["Psot 0"][files["Psot 0"].index(b"\xff\x90") + 6:][:4] == bytes(4)
    assert files["no EOC"][-2:] != b"\xff\xd9" and files["Psot 0"][-2:] == b"\xff\xd9"
    if d.pillow_has_jpeg2000():  # OpenJPEG reads them too (but for the missing EOC, which Pillow turns into an error)
        from test_jpeg2000_model import pillow_decode
        for name, f, want in d.handbuilt_set()[:3]:
            assert np.array_equal(pillow_decode(f)[1], want), name


def test_structural_refusals_by_hand():
    img, cases = d.marker_cases()
    seen = set()
    for name, f, want in cases:
        got = d.decode(f, 9, 11)
        seen.add(want)
        assert (isinstance(got, str) and got == want) if want != "OK" else np.array_equal(got, img), (name, got)
    assert seen == {"OK", "CCT_E_J2K", "CCT_E_STREAM"}


def test_damage_is_defined():
    """the rules a damaged file falls under: clamping, modulo arithmetic, 0xFF beyond a segment"""
    assert d._wrap(np.array([2 ** 31, -2 ** 31 - 1, 5])).tolist() == [-2 ** 31, 2 ** 31 - 1, 5]
    mq = d.MQDecoder(b"")
    assert [mq.decode(0) for _ in range(8)] == [mq.decode(0) for _ in range(8)] and mq.bp == 0  # all ones, for ever, no byte consumed
    assert d.t1_decode(b"", 4, 4, 0, 3, 7) == d.t1_decode(b"\xff\xff", 4, 4, 0, 3, 7)
    counts = {}
    for base in sorted({b for b, *_ in d.damaged_set()}):
        for dmg, g, want in d.damaged_expected(base):
            key = want if isinstance(want, str) else "OK"
            counts[key] = counts.get(key, 0) + 1
            if not isinstance(want, str):
                assert want.shape == (33, 65) and want.dtype == np.uint16
    assert counts["CCT_E_J2K"] >= 7 and counts["CCT_E_STREAM"] >= 10 and counts["OK"] >= 10, counts
