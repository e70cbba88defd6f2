"""The stream set of tests/jpeg_lossless_streams.py without a GPU: the conditions that keep it from drifting into triviality,
asserted on the model's verdicts alone; Pillow's libjpeg on the 8-bit placement files (fill bytes included); and the host's
marker walk against the model for every file the model refuses before the entropy-coded data."""
import collections
import io

import numpy as np
import pytest

import jpeg_lossless_model as m
import jpeg_lossless_streams as s

E_MIXED, E_JPEG = 10, 13
NOISE_BASES = ("noise_rr2", "noise_p4", "noise_flat5", "noise_code16")


def test_base_files_round_trip_in_the_model():
    for tag, (img, precision, ss, rr, table, bits) in s.bases().items():
        assert np.array_equal(s.base_rasters()[tag], img), tag
    f = s.base_file("const_flat5")
    assert 8 * (len(f) - 80) > 312 * s.SUB  # a second window of 256 subsequences
    h = m.parse(s.base_file("noise_code16"))
    assert 8 * (h["s1"] - h["s0"]) > 2 * 180 * s.SUB  # two intervals of more than 180


def test_conditions_on_the_set():
    v = s.verdicts()
    base = s.base_rasters()
    for e in s.placement_files():
        assert v[e[0]][0] == 0, e[0]  # every placement file is accepted
    groups = collections.Counter()
    far = 0
    for e in s.damage_files():
        kind, raster = v[e[0]]
        tag = s.base_of(e[0])
        if kind == 0 and not np.array_equal(raster, base[tag]):
            groups[tag, "changed"] += 1
        elif kind == "STREAM":
            groups[tag, "STREAM"] += 1
            far += s.DAMAGE_SUB[e[0]] >= 256
    print(dict(groups), "first fault beyond subsequence 256:", far, "files:", len(s.all_files()))
    assert sum(n for (_, g), n in groups.items() if g == "changed") >= 30
    assert sum(n for (_, g), n in groups.items() if g == "STREAM") >= 30
    for tag in s.bases():
        assert groups[tag, "STREAM"] >= 3, tag
        if tag in NOISE_BASES:  # a constant raster under the flat table has no magnitude bits
            assert groups[tag, "changed"] >= 3, tag
    assert far >= 5
    assert len(s.all_files()) <= 320


def test_placement_files_open_in_pillow():
    if not m.pillow_opens_sof3():
        pytest.skip("this Pillow's libjpeg does not open SOF3")
    from PIL import Image
    v = s.verdicts()
    n = 0
    for name, f, rows, cols, bits in s.placement_files():
        if bits == 8:
            assert np.array_equal(np.array(Image.open(io.BytesIO(f))), v[name][1]), name
            n += 1
    assert n > 100


def test_host_marker_walk_gives_the_models_verdict():
    import cct_hip
    v = s.verdicts()
    walked = 0
    for (rows, cols, bits), entries in s.shapes().items():
        early = [e for e in entries if v[e[0]][0] in ("JPEG", "MIXED")]
        for e in entries:
            if v[e[0]][0] == "JPEG":
                with pytest.raises(ValueError):
                    cct_hip.jpeg_lossless_info(e[1])
            else:
                assert cct_hip.jpeg_lossless_info(e[1]) == m.info(e[1]), e[0]
        if early:  # a batch the marker walk refuses whole needs no device
            _, status = cct_hip.jpeg_lossless_decode_batch([e[1] for e in early], rows, cols, bits=bits, raise_errors=False)
            assert list(status) == [E_JPEG if v[e[0]][0] == "JPEG" else E_MIXED for e in early], [e[0] for e in early]
            walked += len(early)
    assert walked >= 3
    # the files of one shape asked for as another: the model and the host both say MIXED
    some = s.shapes()[(3, s.PCOLS, 8)]
    for e in some:
        with pytest.raises(m.JpegError) as err:
            m.decode_frame(e[1], 2, s.PCOLS, 8)
        assert err.value.kind == "MIXED"
    _, status = cct_hip.jpeg_lossless_decode_batch([e[1] for e in some], 2, s.PCOLS, bits=8, raise_errors=False)
    assert list(status) == [E_MIXED] * len(some)
