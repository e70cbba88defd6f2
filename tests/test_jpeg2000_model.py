"""tests/jpeg2000_model.py, the CPU statement of the device JPEG 2000 lossless encoder, against OpenJPEG through Pillow: its
files decode to the input, they are no larger than OpenJPEG's own, the JP2 container and info(), and one pinned file."""
import functools
import io

import numpy as np
import pytest

import jpeg2000_model as m

# The worst (model - OpenJPEG) / OpenJPEG over the 128 x 128 phantoms (seeds 0 .. 3, code-blocks 32 and 64, 0 / 1 / 5 levels,
# shift 0 and 4) and 8- and 16-bit uniform noise (128 x 128 and 130 x 70), measured with Pillow 12.2.0 / OpenJPEG 2.5.4: the
# model's file was 39 bytes smaller every time, the length of OpenJPEG's COM segment, so the worst case is the largest file,
# 35 295 bytes.  The 0.5 % covers inputs that are not in that set.
WORST_VS_OPENJPEG = -39 / 35295
MARGIN = WORST_VS_OPENJPEG + 0.005


@functools.lru_cache(maxsize=None)
def pillow_has_jpeg2000():
    try:
        from PIL import features
        return bool(features.check_codec("jpg_2000"))
    except Exception:
        return False


def needs_pillow():
    if not pillow_has_jpeg2000():
        pytest.skip("this Pillow has no JPEG 2000 codec")


def pillow_decode(file):
    from PIL import Image
    im = Image.open(io.BytesIO(file))
    im.load()
    return im, np.array(im)


def as_pillow_returns(img, precision, shift=0):
    """Pillow hands precision 9 .. 15 back as value << (16 - precision) in I;16, and precision <= 8 as mode L."""
    v = img.astype(np.int64) << shift
    return v << (16 - precision) if 8 < precision < 16 else v


def pillow_encode(img, levels, codeblock):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG2000", irreversible=False, num_resolutions=levels + 1, codeblock_size=(codeblock, codeblock), no_jp2=True)
    return buf.getvalue()


@pytest.mark.parametrize("precision", sorted(m.PRECISIONS))
def test_pillow_decodes_the_matrix(precision):
    needs_pillow()
    for rows, cols, cb, levels, names, imgs, files in m.matrix(precision):
        for name, x, f in zip(names, imgs, files):
            im, got = pillow_decode(f)
            assert im.mode == ("L" if precision <= 8 else "I;16"), (rows, cols, cb, levels, name)
            assert np.array_equal(got.astype(np.int64), as_pillow_returns(x, precision)), (rows, cols, cb, levels, name)


def test_zero_coefficients_include_no_code_block():
    for precision in sorted(m.PRECISIONS):
        for rows, cols, cb, levels, names, imgs, files in m.matrix(precision):
            f = files[names.index("zero")]
            assert len(m.packet_data(f)) == levels + 1, (rows, cols, cb, levels)  # a packet is its first bit and at most six "not included" bits
            assert len(f) == len(m.main_header(rows, cols, precision, levels, cb)) + 14 + levels + 1 + 2


def test_pillow_decodes_phantoms_shift_and_jp2():
    needs_pillow()
    for img, kw, f in m.phantoms():
        im, got = pillow_decode(f)
        assert np.array_equal(got.astype(np.int64), as_pillow_returns(img, kw["precision"], kw.get("shift", 0))), kw
        assert f[:4] == (b"\x00\x00\x00\x0c" if kw.get("jp2") else b"\xff\x4f\xff\x51")


def test_noise_reaches_the_long_codes_and_the_stuffing():
    img, kw, f = m.phantoms()[4]
    assert kw == dict(precision=16, levels=5, codeblock=64)
    data = m.packet_data(f)
    ff = [k for k in range(len(data) - 1) if data[k] == 0xFF]
    assert len(ff) > 50 and all(data[k + 1] < 0x90 for k in ff) and data[-1] != 0xFF  # no marker code inside the packets
    plane = m.dwt_53(img.astype(np.int64) - 32768, 1)
    # HH of 16-bit noise: 17 of the subband's 19 bit-planes (a 5/3 HH coefficient stays below 2^17), 3 * 17 - 2 = 49 passes, which
    # takes the longest number-of-passes code (37 .. 164)
    assert int(np.abs(plane[64:, 64:]).max()).bit_length() == 17
    # Table B.4; the codes of 36 and more open with 0xFF, so a stuffed 0 bit follows their first eight bits
    for n, bits in ((1, "0"), (2, "10"), (5, "1110"), (6, "111100000"), (35, "111111101"), (36, "11111111" "0" "0"), (37, "11111111" "0" "10000000"),
                    (164, "11111111" "0" "11111111")):
        bw = m.BitWriter()
        m.put_passes(bw, n)
        assert "".join(f"{b:08b}" for b in bw.finish()) == bits + "0" * (-len(bits) % 8), n


def test_size_against_openjpeg():
    needs_pillow()
    worst = -1.0
    for img, kw, f in m.phantoms():
        if kw.get("jp2"):
            continue
        shifted = (img.astype(np.uint32) << kw.get("shift", 0)).astype(np.uint16)
        if kw["precision"] != 16:
            continue  # Pillow writes uint16 arrays at precision 16
        ref = pillow_encode(shifted, kw["levels"], kw["codeblock"])
        worst = max(worst, (len(f) - len(ref)) / len(ref))
        assert len(f) <= len(ref) * (1 + MARGIN), (kw, len(f), len(ref))
    for precision in (8, 16):
        for rows, cols, cb, levels, names, imgs, files in m.matrix(precision):
            if min(rows, cols) < 1 << levels:
                continue  # OpenJPEG's encoder refuses more resolutions than the smaller side has octaves; its decoder took these files above
            for name, x, f in zip(names, imgs, files):
                ref = pillow_encode(x, levels, cb)
                assert len(f) <= len(ref) * (1 + MARGIN), (rows, cols, cb, levels, name, len(f), len(ref))
    print(f"worst (model - OpenJPEG) / OpenJPEG over the phantoms and noise: {worst:+.5f}")


def test_container_and_info():
    img = m.raster_cases(5, 3, 12, np.uint16)["ramp"]
    raw, jp2 = m.encode(img, 12, levels=1), m.encode(img, 12, levels=1, jp2=True)
    assert len(jp2) - len(raw) == 85 and jp2[85:] == raw
    assert jp2[:85] == (bytes.fromhex("0000000c6a5020200d0a870a" "00000014667479706a703220000000006a703220" "0000002d6a703268"
                                      "0000001669686472" "00000005" "00000003" "0001" "0b" "07" "00" "00" "0000000f636f6c72" "01" "00" "00" "00000011")
                        + (8 + len(raw)).to_bytes(4, "big") + b"jp2c")
    assert m.info(raw) == m.info(jp2) == (5, 3, 12)
    at = raw.index(b"\xff\x90")
    assert int.from_bytes(raw[at + 6:at + 10], "big") == len(raw) - at - 2  # Psot: SOT up to EOC
    assert raw[raw.index(b"\xff\x5c"):at] == bytes.fromhex("ff5c0007" "40" "60" "68" "68" "70")
    assert m.encode(img, 12, levels=5)[:2] == b"\xff\x4f" and b"\xff\x64" not in raw  # no COM
    big = m.main_header(2, 2, 16, 1, 64)
    assert big[big.index(b"\xff\x5c"):] == bytes.fromhex("ff5c0007" "4080888890")
    for bad in (b"", raw[:40], raw[:4], b"\x89PNG\r\n\x1a\n" + bytes(64), jp2[:77], jp2[:85].replace(b"jp2c", b"free") + raw, raw[:2] + b"\xff\x52" + raw[4:],
                raw[:41] + b"\x02" + raw[42:], raw[:42] + b"\x8b" + raw[43:]):
        with pytest.raises(ValueError):
            m.info(bad)
    if pillow_has_jpeg2000():
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(np.zeros((9, 14), np.uint8)).save(buf, "JPEG2000", irreversible=False)
        assert m.info(buf.getvalue()) == (9, 14, 8)


def test_known_answer():
    img = np.array([[0, 65535, 0, 32768, 0, 32767, 65535, 1]], dtype=np.uint16)
    want = ("ff4fff5100290000000000080000000100000000000000000000000800000001000000000000000000010f0101ff52000c00000001000004040001"
            "ff5c00044080ff90000a0000000000240001ff93dff8909005884024fcf07e34388ff59232244890c30fffd9")
    assert m.encode(img, 16, 0, 0, 64).hex() == want


def test_overflow_and_arguments():
    with pytest.raises(OverflowError):
        m.encode(np.full((3, 3), 4096, np.uint16), 12)
    with pytest.raises(OverflowError):
        m.encode(np.full((3, 3), 4095, np.uint16), 16, shift=5)
    assert m.encode(np.full((3, 3), 4095, np.uint16), 16, shift=4) == m.encode(np.full((3, 3), 65520, np.uint16), 16)
