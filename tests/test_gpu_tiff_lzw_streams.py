"""tiff_lzw_decode_kernel and tiff_lzw_encode_kernel on the hand-built streams and planted strips of tests/tiff_lzw_streams.py:
every decoder case in one tiff_read_batch call and again in reverse order, each refused file between accepted ones, into
host memory and into a sentinel-filled out_dev; the cases embedded in ordinary multi-strip files; the strings of 3000 bytes;
the planted strips through tiff_encode_batch, byte for byte the model's and Pillow's.  tests/tiff_model.py gives every
expectation and tests/test_tiff_lzw_streams_host.py pins it to libtiff and asserts what the cases reach."""
import functools

import numpy as np
import pytest

import tiff_lzw_streams as t
import tiff_model as m

pytestmark = pytest.mark.gpu

E_STREAM = 4
SENTINEL = 0xA5


@functools.lru_cache(maxsize=None)
def _expected():
    """{name: the model's raster or "CCT_E_STREAM"}, computed once"""
    return {c.name: t.expected(c) for c in t.cases() + t.long_cases()}


@functools.lru_cache(maxsize=None)
def _items(long=False):
    """[(name, file, expectation)] with every refused file between two accepted ones"""
    exp = _expected()
    cases = t.long_cases() if long else t.cases()
    good = [c for c in cases if c.accept]
    out, k = [], 0
    for c in cases:
        if not c.accept:
            if not out or isinstance(out[-1][2], str):
                out.append((good[k % len(good)].name, t.file_of(good[k % len(good)]), exp[good[k % len(good)].name]))
                k += 1
        out.append((c.name, t.file_of(c), exp[c.name]))
    if isinstance(out[-1][2], str):
        out.append((good[k % len(good)].name, t.file_of(good[k % len(good)]), exp[good[k % len(good)].name]))
    assert all(not (isinstance(a[2], str) and isinstance(b[2], str)) for a, b in zip(out, out[1:]))
    assert not isinstance(out[0][2], str) and not isinstance(out[-1][2], str)
    return tuple(out)


def _wrong(items, rasters, status):
    """[(index, name, status, first differing byte)] of the files that did not come out as the model says"""
    wrong = []
    for k, (name, _, want) in enumerate(items):
        if isinstance(want, str):
            if status[k] != E_STREAM:
                wrong.append((k, name, int(status[k]), "refused by the model"))
        elif status[k] != 0 or not np.array_equal(rasters[k], want):
            diff = np.flatnonzero(np.asarray(rasters[k]).ravel() != want.ravel())
            wrong.append((k, name, int(status[k]), int(diff[0]) if diff.size else None))
    return wrong


def _run(items, rows, cols, bits=8):
    import cct_hip
    back, status = cct_hip.tiff_read_batch([f for _, f, _ in items], rows, cols, bits=bits, raise_errors=False)
    wrong = _wrong(items, back, status)
    assert not wrong, f"{len(wrong)} of {len(items)} files: (index, case, status, first differing byte) {wrong[:12]}"
    return status


def test_every_case_in_one_batch_both_orders():
    items = _items()
    assert len(items) >= len(t.cases()) and sum(isinstance(w, str) for _, _, w in items) >= 50
    _run(items, t.ROWS, t.COLS)
    _run(items[::-1], t.ROWS, t.COLS)   # other neighbours, other places in the uploaded bytes


def test_into_device_memory_neighbours_are_exact_and_nothing_follows():
    import cct_hip
    items = _items()
    n, size = len(items), t.WANT
    d = cct_hip.DeviceBuffer.from_numpy(np.full(n * size + 256, SENTINEL, np.uint8))
    try:
        shape, status = cct_hip.tiff_read_batch([f for _, f, _ in items], t.ROWS, t.COLS, bits=8, out_dev=d, raise_errors=False)
        assert tuple(shape) == (n, t.ROWS, t.COLS)
        dev = d.download(np.uint8, n * size).reshape(n, t.ROWS, t.COLS)
        tail = d.download(np.uint8, 256, offset=n * size)
    finally:
        d.free()
    wrong = _wrong(items, dev, status)
    assert not wrong, f"(index, case, status, first differing byte) {wrong[:12]}"
    assert (tail == SENTINEL).all()     # nothing behind the last raster


def test_raise_errors_names_the_first_refused_file():
    import cct_hip
    items = _items()
    first = next(k for k, (_, _, w) in enumerate(items) if isinstance(w, str))
    with pytest.raises(ValueError):
        cct_hip.tiff_read_batch([f for _, f, _ in items[:first + 2]], t.ROWS, t.COLS, bits=8)
    accepted = [it for it in items[:40] if not isinstance(it[2], str)]
    back = cct_hip.tiff_read_batch([f for _, f, _ in accepted], t.ROWS, t.COLS, bits=8)
    assert all(np.array_equal(b, w) for b, (_, _, w) in zip(back, accepted))


def test_cases_embedded_in_ordinary_files():
    a = m._fixture_raster()
    good = [m.write_file(a, "lzw", 2, 7), m.build_file(a, 8, 2, 7, "MM"), m.write_file(a, "none", 1, 3), m.build_file(a, 5, 1, 5, "MM")]
    items = []
    for k, (name, f, want) in enumerate(t.embedded_files()):
        items += [("good", good[k % len(good)], a), (name, f, want)]
    items.append(("good", good[0], a))
    assert sum(isinstance(w, str) for _, _, w in items) == 2
    _run(items, a.shape[0], a.shape[1], bits=16)
    _run(items[::-1], a.shape[0], a.shape[1], bits=16)


def test_strings_of_3000_bytes():
    items = _items(long=True)
    assert len(items) == len(t.long_cases()) and sum(isinstance(w, str) for _, _, w in items) == 1
    _run(items, t.LONG_ROWS, t.LONG_COLS)


def test_planted_strips_probe_beyond_the_first_window():
    import cct_hip
    strips = dict(t.probe_strips())
    n = max(len(s) for s in strips.values())
    plain = np.random.default_rng(8).integers(0, 7, n).astype(np.uint8)
    for name, strip in strips.items():
        s = np.frombuffer(strip, np.uint8)
        s = np.concatenate([s, s[:n - len(s)]])          # one shape for the call: the shorter strip goes on with its own start
        strips[name] = s
    imgs = np.stack([strips["middle"], plain, strips["end"]])[:, None, :]
    for name in ("middle", "end"):                       # the padded strips still reach what the host test asserts of the planted ones
        c = t.probe_census(strips[name].tobytes())
        assert c["max_rounds"] >= 3 and c["late_inserts"] and c["late_finds"] and (name == "middle" or c["wrapped_late"])
    got = cct_hip.tiff_encode_batch(imgs)
    for g, x, name in zip(got, imgs, ("middle", "plain", "end")):
        assert g == m.write_file(x, "lzw"), name
        assert m.same_file(g, m.pillow_file(x, "lzw")), name
    assert np.array_equal(cct_hip.tiff_read_batch(got, 1, n, bits=8), imgs)
