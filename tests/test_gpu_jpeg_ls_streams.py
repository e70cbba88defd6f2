"""Device JPEG-LS decoder (cct_jpegls_decode_batch) on the placed and damaged files of tests/jpeg_ls_streams.py: 0xFF data
bytes on chosen offsets, intervals that end in FF 00, LSE segments, and damage of every family.  The status of every file
is the model's verdict, an accepted file decodes to exactly the model's raster, and a refused file disturbs nothing
around it.  The encoder writes the placement rasters as the model does."""
import numpy as np
import pytest

import jpeg_ls_streams as s

pytestmark = pytest.mark.gpu

E_STREAM, E_MIXED, E_JPEGLS = 4, 10, 16
CODE = {0: 0, "JPEGLS": E_JPEGLS, "MIXED": E_MIXED, "STREAM": E_STREAM}
SHAPES = sorted(s.shapes())
DAMAGE_SHAPES = sorted({e[2:] for e in s.damage_files()})  # the shapes that have refused files


def check(entries, status, rasters, tag):
    v = s.verdicts()
    wrong = [(e[0], int(st), v[e[0]][0]) for e, st in zip(entries, status) if st != CODE[v[e[0]][0]]]
    assert not wrong, (tag, wrong)
    other = [e[0] for i, e in enumerate(entries) if v[e[0]][0] == 0 and not np.array_equal(rasters[i], v[e[0]][1])]
    assert not other, (tag, other)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "x".join(map(str, sh)))
def test_one_mixed_batch_per_shape(shape):
    import cct_hip
    rows, cols, bits = shape
    entries = s.shapes()[shape]
    res, status = cct_hip.jpeg_ls_decode_batch([e[1] for e in entries], rows, cols, bits=bits, raise_errors=False)
    check(entries, status, res, shape)


@pytest.mark.parametrize("shape", DAMAGE_SHAPES, ids=lambda sh: "x".join(map(str, sh)))
def test_refused_between_accepted_into_a_sentinel(shape):
    """refused and accepted files alternate as far as both last, good files on both ends, decoded into a device buffer
    that holds a sentinel: a file the host refuses leaves its slot alone, and so does the batch the slot behind it"""
    import cct_hip
    rows, cols, bits = shape
    v = s.verdicts()
    good = [e for e in s.shapes()[shape] if v[e[0]][0] == 0]
    bad = [e for e in s.shapes()[shape] if v[e[0]][0] != 0]
    assert good and bad
    entries = [good[0]]
    for i, b in enumerate(bad):
        entries += [b, good[(i + 1) % len(good)]]
    n = len(entries)
    dt = np.uint8 if bits == 8 else np.uint16
    mark = 0xA5 if bits == 8 else 0xA5A5
    sentinel = np.full((n + 1, rows, cols), mark, dt)
    d = cct_hip.DeviceBuffer.from_numpy(sentinel)
    try:
        got_shape, status = cct_hip.jpeg_ls_decode_batch([e[1] for e in entries], rows, cols, bits=bits, out_dev=d, raise_errors=False)
        got = d.download(dt, sentinel.size).reshape(sentinel.shape)
    finally:
        d.free()
    assert got_shape == (n, rows, cols)
    check(entries, status, got, shape)
    for i, e in enumerate(entries):
        if v[e[0]][0] in ("JPEGLS", "MIXED") or "/rst_" in e[0]:
            assert (got[i] == mark).all(), e[0]  # never sent to the device
    assert (got[n] == mark).all()  # the slot behind the batch


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "x".join(map(str, sh)))
def test_accepted_files_alone_raise_nothing(shape):
    import cct_hip
    rows, cols, bits = shape
    v = s.verdicts()
    good = [e for e in s.shapes()[shape] if v[e[0]][0] == 0]
    res = cct_hip.jpeg_ls_decode_batch([e[1] for e in good], rows, cols, bits=bits)
    assert res.shape == (len(good), rows, cols)
    check(good, [0] * len(good), res, shape)


def test_encoder_writes_the_placement_rasters():
    import cct_hip
    groups = {}
    for name, x, p, rr, f in s.placement_rasters():
        groups.setdefault((x.shape, p, rr), []).append((name, x, f))
    for (shape, p, rr), g in groups.items():
        got = cct_hip.jpeg_ls_encode_batch(np.stack([x for _, x, _ in g]), precision=p, restart_rows=rr)
        assert [name for (name, _, f), h in zip(g, got) if f != h] == []
