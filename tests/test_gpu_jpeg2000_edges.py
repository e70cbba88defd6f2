"""The device JPEG 2000 encoder and decoder on the planted cases of tests/jpeg2000_edges.py: 2 to 8 decomposition levels down to
lengths 2 and 1, precisions 2, 3, 7, 9, 15, tag trees of five levels with excluded leaves, every neighbour pattern and sign key in
every orientation, 1 to 19 bit-planes, segment lengths at every power of two, the adversary's segment.  The encoder's files equal
the model's byte for byte; the decoder is given the model's files, not the device's own.  tests/test_jpeg2000_edges_host.py proves
that the cases reach what they plant; tools/debug/j2k_host_emu and j2k_dec_host_emu ran the set under AddressSanitizer and UBSan
before it ran here."""
import numpy as np
import pytest

import jpeg2000_edges as e
import jpeg2000_model as m

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_STREAM, E_ARG, E_MIXED = 3, 4, 9, 10
GROUPS = ("levels", "precision", "tagtree", "tier1", "mq_t2", "adversary")


def first_difference(a, b):
    return next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))


def encode(cct_hip, rasters, kw, **more):
    return cct_hip.jpeg2000_encode_batch(rasters, precision=kw["precision"], shift=kw.get("shift", 0), levels=kw["levels"], codeblock=kw["codeblock"],
                                         jp2=kw.get("jp2", False), **more)


def test_encode_equals_the_model():
    """One call per (shape, coding) with all its cases, whatever their group, from host memory: every depth from 2 to 8 levels runs with
    three frames at least, so a wrong stride between the frames' planes, slabs, tag trees or files shows in the second frame."""
    import cct_hip
    bound = cct_hip._ffi.lib().cct_j2k_bound
    files, n = e.files(), 0
    for rows, cols, kw, cs in e.batches():
        got = encode(cct_hip, np.stack([c.raster for c in cs]), kw)
        limit = bound(rows, cols, kw["levels"], kw["codeblock"], int(kw.get("jp2", False)))
        for c, g in zip(cs, got):
            want = files[c.name]
            assert g == want, (c.name, "first difference at", first_difference(g, want), len(g), len(want))
            assert len(g) <= limit, (c.name, len(g), limit)
        n += len(cs)
    assert n == len(e.cases())
    assert all(len(cs) >= 3 for _, _, kw, cs in e.batches() if kw["levels"] >= 2 and cs[0].group == "levels")
    assert all(len(cs) >= 3 for _, _, kw, cs in e.batches() if kw["levels"] >= 6)


def test_encode_from_device_memory():
    """The largest batch, and the three-frame batches of 3 x 300 and 300 x 3 at 8 levels as JP2, from a DeviceBuffer."""
    import cct_hip
    files = e.files()
    largest = max(e.batches(), key=lambda b: (len(b[3]), b[0] * b[1]))
    deep = [b for b in e.batches() if b[2]["levels"] == 8 and b[2].get("jp2") and (b[0], b[1]) in ((3, 300), (300, 3))]
    assert len(largest[3]) >= 6 and len(deep) == 2
    for rows, cols, kw, cs in [largest] + deep:
        imgs = np.stack([c.raster for c in cs])
        buf = cct_hip.DeviceBuffer.from_numpy(imgs)
        try:
            got = encode(cct_hip, buf, kw, shape=imgs.shape, dtype=imgs.dtype.type)
        finally:
            buf.free()
        for c, g in zip(cs, got):
            assert g == files[c.name], (c.name, "first difference at", first_difference(g, files[c.name]))


@pytest.mark.parametrize("group", GROUPS)
def test_decode_the_models_files(group):
    """Per shape one call with every coding and precision of the shape mixed (9, 15 and 16 bits share bits=16), forwards into host
    memory and backwards; a shifted file decodes to the shifted samples."""
    import cct_hip
    files = e.files()
    for rows, cols, cs in e.decode_batches():
        cs = [c for c in cs if c.group == group]
        if not cs:
            continue
        for order in (cs, cs[::-1]):
            got = cct_hip.jpeg2000_decode_batch([files[c.name] for c in order], rows, cols)
            assert got.dtype == np.uint16 and got.shape == (len(order), rows, cols)
            for c, g in zip(order, got):
                assert np.array_equal(g, c.raster.astype(np.uint16) << c.kw.get("shift", 0)), c.name


def test_decode_into_a_device_buffer_with_a_guard():
    """Every shape's mixed batch into a sentinel-filled DeviceBuffer, with a file cut in the middle of its packets in a slot of its own in the
    middle of the batch: the verdict on that file is the model's, every other raster is whole, and the samples behind the last raster are the
    sentinel's."""
    import cct_hip
    import jpeg2000_decode_model as d
    files = e.files()
    shapes = {(rows, cols) for rows, cols, _ in e.decode_batches()}
    assert set(e.LEVEL_SHAPES) | {s[:2] for s in e.TREE_SHAPES} | {(97, 97), (64, 64), (33, 65)} <= shapes
    for rows, cols, cs in e.decode_batches():
        whole = max((files[c.name] for c in cs), key=len)
        cut = whole[:len(whole) - max(1, len(m.packet_data(whole)) // 2)]
        verdict = d.decode(cut, rows, cols)
        batch = [files[c.name] for c in cs]
        at = len(batch) // 2
        batch.insert(at, cut)
        n, guard, px = len(batch), 4096, rows * cols
        out = cct_hip.DeviceBuffer((n * px + guard) * 2)
        try:
            out.upload(np.full(n * px + guard, 0xA5C3, np.uint16))
            shape, status = cct_hip.jpeg2000_decode_batch(batch, rows, cols, out_dev=out, raise_errors=False)
            got = out.download(np.uint16, n * px + guard)
        finally:
            out.free()
        assert shape == (n, rows, cols) and np.all(got[n * px:] == 0xA5C3), (rows, cols)
        got = got[:n * px].reshape(n, rows, cols)
        assert isinstance(verdict, str) and verdict == "CCT_E_STREAM" and status[at] == E_STREAM, (rows, cols, verdict, status[at])
        assert not np.any(np.delete(status, at)), (rows, cols, list(status))
        for c, g in zip(cs, np.delete(got, at, axis=0)):
            assert np.array_equal(g, c.raster.astype(np.uint16) << c.kw.get("shift", 0)), c.name


def test_decode_eight_bits_allocated_and_the_shift_on_the_way_back():
    import cct_hip
    files = e.files()
    low = [c for c in e.cases() if c.kw["precision"] <= 8 and c.group == "precision"]
    assert {c.kw["precision"] for c in low} == {2, 3, 7, 8}
    for shape in sorted({c.raster.shape for c in low}):
        cs = [c for c in low if c.raster.shape == shape]
        got = cct_hip.jpeg2000_decode_batch([files[c.name] for c in cs], *shape, bits=8)   # precisions 2, 3, 7 (and 8) in one batch
        assert got.dtype == np.uint8
        for c, g in zip(cs, got):
            assert np.array_equal(g, c.raster << c.kw.get("shift", 0)), c.name
    wide = next(c for c in e.cases() if c.kw["precision"] == 9 and c.raster.shape == (33, 65))
    res, status = cct_hip.jpeg2000_decode_batch([files[low[-1].name], files[wide.name]], 33, 65, bits=8, raise_errors=False)
    assert low[-1].raster.shape == (33, 65) and list(status) == [0, E_MIXED]   # 9 bits of precision do not fit 8 allocated
    shifted = [c for c in e.cases() if c.kw.get("shift")]
    assert {c.kw["precision"] - c.kw["shift"] for c in shifted} == {1, 2} and {c.kw["precision"] for c in shifted} == {2, 8, 9, 16}
    for c in shifted:
        bits = 8 if c.kw["precision"] <= 8 else 16
        got = cct_hip.jpeg2000_decode_batch([files[c.name]], 33, 65, bits=bits, shift=c.kw["shift"])
        assert np.array_equal(got[0], c.raster), c.name


def test_refusals_and_overflow_at_the_edge_precisions():
    import cct_hip
    L = cct_hip._ffi.lib()
    img = np.zeros((1, 8, 8), np.uint16)
    for bad in (dict(levels=9), dict(precision=1)):
        with pytest.raises(ValueError):
            cct_hip.jpeg2000_encode_batch(img, **bad)
    assert L.cct_j2k_bound(8, 8, 9, 64, 0) == 0
    out, sizes, status = np.zeros(4096, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    for levels, precision in ((9, 16), (5, 1)):
        assert L.cct_j2k_encode_batch(img.ctypes.data, 0, 1, 8, 8, 16, precision, 0, levels, 64, 0, out.ctypes.data, 4096, sizes.ctypes.data, status.ctypes.data) == E_ARG
    for precision in (2, 15):   # a sample of 2^precision: that frame alone is refused, its neighbours are whole
        imgs = np.random.default_rng(precision).integers(0, 1 << precision, (4, 5, 33)).astype(np.uint16)
        imgs[1, 4, 32] = imgs[3, 0, 0] = 1 << precision
        stride = L.cct_j2k_bound(5, 33, 2, 32, 0)
        out = np.zeros((4, stride), np.uint8)
        sizes, status = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
        rc = L.cct_j2k_encode_batch(imgs.ctypes.data, 0, 4, 5, 33, 16, precision, 0, 2, 32, 0, out.ctypes.data, stride, sizes.ctypes.data, status.ctypes.data)
        assert rc == E_OVERFLOW and list(status) == [0, E_OVERFLOW, 0, E_OVERFLOW] and sizes[1] == sizes[3] == 0
        for i in (0, 2):
            assert out[i, :sizes[i]].tobytes() == m.encode(imgs[i], precision, 0, 2, 32), (precision, i)
        with pytest.raises(OverflowError):
            cct_hip.jpeg2000_encode_batch(imgs, precision=precision, levels=2, codeblock=32)
