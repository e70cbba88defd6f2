"""Device TIFF writer and reader (cct_hip.tiff_encode_batch / tiff_read_batch) against tests/tiff_model.py and Pillow:
files byte for byte from host arrays and from a DeviceBuffer, Deflate levels per strip against zlib, rasters back from the
device's, the model's, Pillow's and foreign files into host memory and into out_dev, per-file codes of damaged and refused
files in mixed batches with untouched neighbours, and the LZW edges of the census (tests/test_tiff_host.py asserts it)."""
import functools
import zlib

import numpy as np
import pytest

import tiff_model as m

pytestmark = pytest.mark.gpu

CODES = {"CCT_E_ZLIB": 2, "CCT_E_STREAM": 4, "CCT_E_TIFF": 15}


def bits_of(a):
    return 8 * a.dtype.itemsize


@functools.lru_cache(maxsize=None)
def cases():
    return m.raster_cases()


@functools.lru_cache(maxsize=None)
def phantoms():
    from cct_hip.synth import ct_phantom
    return np.stack([ct_phantom(seed, n=128) for seed in range(4)]).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def slices512():
    from cct_hip.synth import ct_phantom
    return np.stack([ct_phantom(seed, n=512) for seed in (11, 12)]).astype(np.uint16)


@pytest.mark.parametrize("compression", ["lzw", "deflate"])
@pytest.mark.parametrize("predictor", [1, 2])
def test_files_equal_the_models_and_pillows(compression, predictor):
    import cct_hip
    for name, a, rpss in cases():
        for rps in rpss:
            got = cct_hip.tiff_encode_batch(np.stack([a, a[::-1]]), compression, predictor, rps)  # two files a call: offsets per file
            for g, x in zip(got, (a, a[::-1])):
                assert g == m.write_file(x, compression, predictor, rps), (name, rps)
                assert m.same_file(g, m.pillow_file(x, compression, predictor, rps)), (name, rps)


def test_uncompressed_files_equal_the_models_and_pillow_reads_them():
    import cct_hip
    for name, a, rpss in cases():
        for rps in rpss:
            (g,) = cct_hip.tiff_encode_batch(a, "none", rows_per_strip=rps)
            assert g == m.write_file(a, "none", 1, rps), (name, rps)
            assert np.array_equal(m.pillow_read(g), a), (name, rps)


def test_lzw_edges_of_the_census():
    import cct_hip
    for name, strip in m.edge_strips():  # EOI at each new width, behind a Clear, one code after a Clear
        a = np.frombuffer(strip, np.uint8).reshape(1, -1)
        (g,) = cct_hip.tiff_encode_batch(a)
        assert g == m.write_file(a, "lzw"), name
        assert np.array_equal(cct_hip.tiff_read_batch([g], 1, a.shape[1], bits=8)[0], a), name


@pytest.mark.parametrize("compression,predictor", [("lzw", 2), ("deflate", 2), ("lzw", 1)])
def test_phantoms_from_host_and_device(compression, predictor):
    import cct_hip
    imgs = phantoms()
    want = [m.pillow_file(x, compression, predictor) for x in imgs]
    got = cct_hip.tiff_encode_batch(imgs, compression, predictor)
    assert all(m.same_file(g, w) for g, w in zip(got, want))
    d = cct_hip.DeviceBuffer.from_numpy(imgs)
    try:
        assert cct_hip.tiff_encode_batch(d, compression, predictor, shape=imgs.shape) == got
        assert cct_hip.tiff_encode_batch(d, compression, predictor, shape=imgs.shape[1:]) == got[:1]
        low = (imgs & 0xFF).astype(np.uint8)
        d.upload(low)
        got8 = cct_hip.tiff_encode_batch(d, compression, predictor, rows_per_strip=50, shape=low.shape, dtype=np.uint8)
        assert got8 == cct_hip.tiff_encode_batch(low, compression, predictor, rows_per_strip=50)
        assert all(m.same_file(g, m.pillow_file(x, compression, predictor, 50)) for g, x in zip(got8, low))
        with pytest.raises(ValueError):
            cct_hip.tiff_encode_batch(d, shape=(5, 128, 128))  # more than the buffer holds
    finally:
        d.free()


@pytest.mark.parametrize("compression", ["lzw", "deflate"])
def test_two_512_slices_at_the_default_strip_height(compression):
    import cct_hip
    imgs = slices512()
    got = cct_hip.tiff_encode_batch(imgs, compression, 2)
    for g, x in zip(got, imgs):
        assert m.same_file(g, m.pillow_file(x, compression, 2))
        assert m.parse(g)["rps"] == 64 and len(m.parse(g)["offs"]) == 8
    assert np.array_equal(cct_hip.tiff_read_batch(got, 512, 512), imgs)


@pytest.mark.parametrize("level", [4, 5, 6, 7, 8, 9, -1])
def test_deflate_levels_per_strip(level):
    import cct_hip
    imgs = phantoms()[:2]
    for pred, rps in ((2, 50), (1, None)):
        got = cct_hip.tiff_encode_batch(imgs, "deflate", pred, rps, level=level)
        for g, x in zip(got, imgs):
            assert g == m.write_file(x, "deflate", pred, rps, level=6 if level == -1 else level)
            d = m.parse(g)
            for (off, cnt), strip in zip(zip(d["offs"], d["counts"]), m.strips_of(x, pred, rps)[0]):
                assert g[off:off + cnt] == zlib.compress(strip, level)


def _read_both_ways(files, rasters):
    """tiff_read_batch into host memory and into out_dev"""
    import cct_hip
    n, rows, cols = rasters.shape
    bits = bits_of(rasters)
    back = cct_hip.tiff_read_batch(files, rows, cols, bits=bits)
    assert back.dtype == rasters.dtype and np.array_equal(back, rasters)
    d = cct_hip.DeviceBuffer(rasters.nbytes + 64)
    try:
        d.zero()
        assert cct_hip.tiff_read_batch(files, rows, cols, bits=bits, out_dev=d) == rasters.shape
        assert np.array_equal(d.download(rasters.dtype, rasters.size).reshape(rasters.shape), rasters)
        assert not d.download(np.uint8, 64, offset=rasters.nbytes).any()  # nothing behind the last raster
    finally:
        d.free()


@pytest.mark.parametrize("source", ["device", "model", "pillow"])
def test_reader_returns_the_rasters(source):
    import cct_hip
    for name, a, rpss in cases():
        files, rasters = [], []
        for comp in ("none", "lzw", "deflate"):  # one mixed batch per raster
            for pred in ((1,) if comp == "none" else (1, 2)):
                for rps in rpss:
                    if source == "device":
                        files += cct_hip.tiff_encode_batch(a, comp, pred, rps)
                    elif source == "model":
                        files.append(m.write_file(a, comp, pred, rps))
                    elif comp != "none":
                        files.append(m.pillow_file(a, comp, pred, rps))
                    else:
                        continue
                    rasters.append(a)
        _read_both_ways(files, np.stack(rasters))


def test_reader_takes_the_foreign_files():
    groups = {}
    for name, f, a in m.foreign_files():
        groups.setdefault((a.shape, a.dtype.str), []).append((f, a))
    assert len(groups) >= 3
    for fa in groups.values():
        _read_both_ways([f for f, _ in fa], np.stack([a for _, a in fa]))


def test_damaged_files_in_a_mixed_batch_give_the_models_codes():
    import cct_hip
    groups = {}
    for name, f, a in m.damaged_files() + [(n, f, (m._fixture_raster() >> 4).astype(np.uint8)) for n, f in m.short_uncompressed_files()]:
        groups.setdefault((a.shape, a.dtype.str), []).append((name, f, a))
    seen = set()
    for items in groups.values():
        a = items[0][2]
        good = [m.write_file(a, "lzw", 2, 7), m.write_file(a, "deflate", 1, 5), m.write_file(a, "none", 1, 3)]
        files, want = [], []
        for k, (name, f, _) in enumerate(items):  # every damaged file between two good ones
            files += [good[k % 3], f]
            want += [a, m.read(f, a.shape[0], a.shape[1], bits_of(a))]
        files.append(good[0]); want.append(a)
        back, status = cct_hip.tiff_read_batch(files, a.shape[0], a.shape[1], bits=bits_of(a), raise_errors=False)
        for i, w in enumerate(want):
            if isinstance(w, str):
                assert status[i] == CODES[w], (items[i // 2][0], status[i], w)
                seen.add(w)
            else:
                assert status[i] == 0 and np.array_equal(back[i], w), i
        # into device memory: the neighbours of a refused file are untouched, a sentinel stays where nothing was decoded
        d = cct_hip.DeviceBuffer(len(files) * a.nbytes)
        try:
            _, status2 = cct_hip.tiff_read_batch(files, a.shape[0], a.shape[1], bits=bits_of(a), out_dev=d, raise_errors=False)
            assert np.array_equal(status2, status)
            dev = d.download(a.dtype, len(files) * a.size).reshape((len(files),) + a.shape)
            for i, w in enumerate(want):
                if not isinstance(w, str):
                    assert np.array_equal(dev[i], w), i
        finally:
            d.free()
        first = next(i for i, w in enumerate(want) if isinstance(w, str))
        with pytest.raises(zlib.error if want[first] == "CCT_E_ZLIB" else ValueError):
            cct_hip.tiff_read_batch(files, a.shape[0], a.shape[1], bits=bits_of(a))
    assert seen == {"CCT_E_STREAM", "CCT_E_ZLIB"}


def test_refused_files_leave_their_neighbours_alone():
    import cct_hip
    a = m._fixture_raster()
    good = m.write_file(a, "lzw", 2, 7)
    other_shape = m.write_file(a[:, :39].copy(), "lzw")
    other_depth = m.write_file((a >> 8).astype(np.uint8), "lzw")
    refused = [f for _, f in m.refused_files()] + [other_shape, other_depth]
    files = [good]
    for f in refused:
        files += [f, good]
    sentinel = np.full((len(files),) + a.shape, 0xABCD, np.uint16)
    d = cct_hip.DeviceBuffer.from_numpy(sentinel)
    try:
        _, status = cct_hip.tiff_read_batch(files, 23, 40, out_dev=d, raise_errors=False)
        dev = d.download(np.uint16, sentinel.size).reshape(sentinel.shape)
    finally:
        d.free()
    assert list(status[0::2]) == [0] * (len(refused) + 1) and list(status[1::2]) == [CODES["CCT_E_TIFF"]] * len(refused)
    assert all(np.array_equal(x, a) for x in dev[0::2]) and (dev[1::2] == 0xABCD).all()  # nothing was written for a refused file
    back, status = cct_hip.tiff_read_batch(files, 23, 40, raise_errors=False)
    assert all(np.array_equal(x, a) for x in back[0::2])
    with pytest.raises(ValueError):
        cct_hip.tiff_read_batch(files, 23, 40)
    assert cct_hip.tiff_info(good) == (23, 40, 16)
