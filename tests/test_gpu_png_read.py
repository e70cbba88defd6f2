"""Device PNG reader (cct_png_read_batch / png_read_batch): the files of tests/png_files.py, which Pillow reads to the same
samples in tests/test_png_read_host.py, the writer's own files, the reference's preview, and the refusals."""
import copy
import hashlib
import json
import os
import threading

import numpy as np
import pytest

import golden_inputs as gi
import png_files as pf
import png_model as pm

pytestmark = pytest.mark.gpu

FIXTURE = json.load(open(os.path.join(gi.GOLDEN, "png.json")))
GUARD = 4096  # samples behind the last raster of a DeviceBuffer that must stay as they were
PATTERN = 0xA5C3


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    cct_hip.device_info()
    return cct_hip


def _guarded(hip, n_px):
    d = hip.DeviceBuffer(2 * (n_px + GUARD))
    d.upload(np.full(n_px + GUARD, PATTERN, np.uint16))
    return d


def _read_dev(hip, files, shift, shape, **kw):
    """png_read_batch into a DeviceBuffer whose capacity is exactly the batch; the guard behind it must stay untouched"""
    n_px = len(files) * shape[0] * shape[1]
    d = _guarded(hip, n_px)
    d.nbytes = 2 * n_px  # what the library may use
    res = hip.png_read_batch(files, shift=shift, out_dev=d, **kw)
    d.nbytes = 2 * (n_px + GUARD)
    got = d.download(np.uint16, n_px + GUARD)
    assert np.all(got[n_px:] == PATTERN), "the reader wrote behind the last raster"
    return res, got[:n_px].reshape((len(files),) + tuple(shape))


def _check(hip, cases, shifts=pf.SHIFTS):
    files = [f for _, f, _ in cases]
    want = np.stack([img for _, _, img in cases])
    for shift in shifts:
        host = hip.png_read_batch(files, shift=shift)
        assert host.dtype == np.uint16 and host.shape == want.shape
        shape, dev = _read_dev(hip, files, shift, want.shape[1:])
        assert shape == want.shape
        for k, (name, _, _) in enumerate(cases):
            assert np.array_equal(host[k], want[k] >> shift), (name, shift, "host")
            assert np.array_equal(dev[k], want[k] >> shift), (name, shift, "out_dev")


@pytest.mark.parametrize("cols", pf.COLS)
@pytest.mark.parametrize("rows", pf.ROWS)
def test_unfilter_edges(hip, rows, cols):
    _check(hip, pf.edge_batch(rows, cols))


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_unfilter_with_every_number_of_waves(hip, waves):
    """bands handed from wave to wave, and from a wave to itself: 129 and 300 rows are 3 and 5 bands"""
    import ctypes as C
    L = hip._ffi.lib()
    old = C.c_int(0)
    assert L.cct_get_option(b"png_unfilter_waves", C.byref(old)) == 0
    assert L.cct_set_option(b"png_unfilter_waves", waves) == 0
    try:
        _check(hip, pf.edge_batch(129, 300), shifts=(0,))
        _check(hip, pf.edge_batch(129, 1), shifts=(4,))
        rng = np.random.default_rng(waves)
        tall = rng.integers(0, 65536, (300, 130), dtype=np.uint16)
        _check(hip, [("tall-paeth", pf.make_png(tall, 16, 4), tall), ("tall-mix", pf.make_png(tall, 16, rng.integers(0, 5, 300)), tall),
                     ("tall-average", pf.make_png(tall, 16, 3), tall)], shifts=(0,))
    finally:
        L.cct_set_option(b"png_unfilter_waves", old.value)


def test_chunk_layer(hip):
    _check(hip, pf.chunk_cases(), shifts=(0, 4))


def test_one_idat_above_64_kib(hip):
    _check(hip, [pf.big_idat_case()], shifts=(0,))


@pytest.mark.parametrize("level", [6, 9])
@pytest.mark.parametrize("name", sorted(pm.cases()))
def test_reads_back_what_the_writer_wrote(hip, name, level):
    img = pm.cases()[name]
    for s in (0, 4):
        x = (img >> s).astype(np.uint16)  # values below 2^(16 - s)
        files = hip.png_encode_batch(np.stack([x, x[::-1]]), level=level, shift=s)
        back = hip.png_read_batch(files, shift=s)
        assert np.array_equal(back[0], x) and np.array_equal(back[1], x[::-1])


def test_mixed_depths_in_one_batch(hip):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (70, 90), dtype=np.uint16)
    b = rng.integers(0, 65536, (70, 90), dtype=np.uint16)
    cases = [("d8", pf.make_png(a, 8, 4), a), ("d16", pf.make_png(b, 16, 3), b), ("d8-again", pf.make_png(a[::-1], 8, 2), a[::-1]),
             ("writer", hip.png_encode_batch(b, level=6)[0], b)]
    _check(hip, cases, shifts=(0, 3))


def test_reference_preview_to_cct_without_the_raster_visiting_the_host(hip):
    fx = FIXTURE["preview"]
    img = gi.load_slice(fx["slice"])
    png = pm.png_bytes(img, fx["level"], fx["shift"])
    assert len(png) == fx["size"] and hashlib.sha256(png).hexdigest() == fx["sha256"]  # the reference's decoded-testing.png
    d = hip.DeviceBuffer(2 * img.size)
    n, w, h = hip.png_read_batch([png], shift=fx["shift"], out_dev=d)
    assert (n, w, h) == (1,) + img.shape
    cfg = copy.deepcopy(hip.default_config())
    cfg["verbose"] = False
    from cct_hip.batch import encode_batch_dev
    out = encode_batch_dev(d, n, w, h, cfg)
    with open(os.path.join(gi.GOLDEN, fx["slice"] + ".cct"), "rb") as f:
        assert out == [f.read()]


def test_refusals(hip):
    cases = pf.damaged_cases()
    files = [f for _, f, _, _ in cases]
    want = np.array([st for _, _, _, st in cases], dtype=np.uint32)
    first_bad = int(want[np.flatnonzero(want)[0]])
    for shift in (0, 4):
        host, st = hip.png_read_batch(files, shift=shift, raise_errors=False)
        assert st.tolist() == want.tolist(), [(c[0], int(s)) for c, s in zip(cases, st) if s != c[3]]
        (shape, st_dev), dev = _read_dev(hip, files, shift, pf.DAMAGED_SHAPE, raise_errors=False)
        assert shape == (len(files),) + pf.DAMAGED_SHAPE and st_dev.tolist() == want.tolist()
        for k, (name, _, img, status) in enumerate(cases):
            if status == 0:
                assert np.array_equal(host[k], img >> shift), name
                assert np.array_equal(dev[k], img >> shift), name
    with pytest.raises(ValueError):
        hip.png_read_batch(files)
    assert first_bad == pf.E_CRC
    # alone, each kind raises what its code maps to
    import zlib
    by_name = {name: f for name, f, _, _ in cases}
    with pytest.raises(zlib.error):
        hip.png_read_batch([by_name["adler-flipped"]])
    with pytest.raises(hip._ffi.CorruptStreamError):
        hip.png_read_batch([by_name["filter-byte-5"]])
    with pytest.raises(ValueError):
        hip.png_read_batch([by_name["good-16"], by_name["other-size"]])
    with pytest.raises(ValueError):
        hip.png_read_batch([by_name["good-16"], by_name["data-byte-flipped"]])


def test_png_read_next_to_encode_in_two_threads(hip):
    cfg = copy.deepcopy(hip.default_config())
    cfg["verbose"] = False
    imgs = np.stack([gi.ct_phantom(i) for i in range(8)])
    files = [pm.png_bytes(im, 6, 4) for im in imgs]
    want_cct = hip.encode_batch(imgs, cfg)
    errors = []

    def run(k):
        try:
            if k == 0:
                assert np.array_equal(hip.png_read_batch(files, shift=4), imgs)
            else:
                assert hip.encode_batch(imgs, cfg) == want_cct
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=run, args=(k,)) for k in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_evaluate_reads_png_slices_on_the_device(hip, tmp_path):
    """tools/evaluate.py --png-input device: the CSV rows of slice0671 and slice3706 from their PNG previews, the same as
    with Pillow on the host and with the sizes of results/encoder-comparisons.csv (tests/test_gpu_parity.py)"""
    import importlib.util
    path = os.path.join(gi.ROOT, "tools", "evaluate.py")
    spec = importlib.util.spec_from_file_location("evaluate", path)
    evaluate = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(evaluate)
    src = tmp_path / "corpus"
    src.mkdir()
    (src / "1-016.png").write_bytes(pm.png_bytes(gi.load_slice("slice0671"), 9, 4))
    (src / "1-55.png").write_bytes(pm.png_bytes(gi.load_slice("slice3706"), 6, 4))
    np.save(src / "2-small.npy", gi.ct_phantom(1)[:64, :128].copy())
    csvs = []
    for where in ("host", "device"):
        out = tmp_path / f"{where}.csv"
        assert evaluate.main([str(src), "--results", str(out), "--png-input", where]) == 0
        csvs.append(out.read_text())
    assert csvs[0] == csvs[1]
    rows = {ln.split(",")[0]: ln.split(",") for ln in csvs[1].splitlines()[1:]}
    a, b = rows["(0000)-1-016.png"], rows["(0001)-1-55.png"]
    assert (a[1], a[2], a[6]) == ("524288", "270969", "207575")
    assert (b[1], b[2], b[6]) == ("524288", "273262", "205179")
