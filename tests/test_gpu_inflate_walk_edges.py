"""Device INFLATE (walk_segment in inflate_kernels.hip) on the inputs of tests/inflate_walk_inputs.py: 48-bit symbols at every
dword phase and buffer fill, across segment ends, in front of the end of the input, across the wrap of the staged window,
and refused.  CPython's zlib gives every expectation; tests/test_inflate_walk_inputs_host.py asserts the preconditions."""
import functools

import numpy as np
import pytest

import deflate_streams as ds
import golden_inputs as gi
import inflate_walk_inputs as wi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[256, 512], ids=["inflate256", "inflate512"])
def hip(request):
    """both geometries of the INFLATE kernel, as in test_gpu_deflate_streams.py"""
    import cct_hip
    from cct_hip import _ffi
    cct_hip.device_info()
    _ffi.check(_ffi.lib().cct_set_option(b"inflate_lanes", request.param))
    yield cct_hip
    _ffi.check(_ffi.lib().cct_set_option(b"inflate_lanes", 0))


@functools.lru_cache(maxsize=None)
def _expected():
    """{name: zlib's bytes or None}, computed once for both geometries"""
    return {c.name: ds.oracle_verdict(c.stream) for c in wi.cases()}


def _max_out():
    return max(len(o) for o in _expected().values() if o is not None)


def _run(hip, items):
    """one batch of (stream, zlib's verdict): status 0 with zlib's bytes, or CCT_E_ZLIB and nothing"""
    outs, status = hip.zlib_decompress_batch([s for s, _ in items], max_out=_max_out(), raise_errors=False)
    wrong = []
    for k, ((_, want), out, st) in enumerate(zip(items, outs, status)):
        ok = (st == 0 and out == want) if want is not None else (st == ds.E_ZLIB and out is None)
        if not ok:
            wrong.append((k, int(st), None if out is None else len(out), None if want is None else len(want)))
    assert not wrong, f"{len(wrong)} of {len(items)} streams: (index, status, bytes, bytes wanted) {wrong[:8]}"


def _items(groups):
    exp = _expected()
    return [(c.stream, exp[c.name]) for c in wi.cases() if c.group in groups]


def test_every_case_in_one_batch_both_orders(hip):
    exp = _expected()
    assert all((exp[c.name] is not None) == c.accept for c in wi.cases())
    items = _items((1, 2, 3, 4, 5))
    good = _items((4,))
    for k, bad in enumerate(_items((6,))):  # every refusal between accepted neighbours
        items += [bad, good[k % len(good)]]
    _run(hip, items)
    _run(hip, items[::-1])  # other neighbours, other alignments


def test_pair_is_the_last_symbol_before_the_end_of_the_input(hip):
    """group 4 as the last stream of the batch: its trailer ends at the end of the input, one byte and one dword before it (a
    stream of one and of four bytes behind it, which zlib refuses as the device does)"""
    front = _items((2,))
    for tail in (b"", b"\0", b"\0\0\0\0"):
        assert ds.oracle_verdict(tail) is None
        for item in _items((4,)):
            _run(hip, front + [item] + ([(tail, None)] if tail else []))


def test_cct_entrance(hip):
    """a pair at every bit offset in the payload of a real .cct file (a flat image: its payload is one long run)"""
    from oracle import oracle
    flat = np.full((256, 256), 1000, np.uint16)
    raw = oracle.encode(flat, deflate=False)
    assert raw[12] == 0
    stream, check = wi.run_payload_stream(raw[13:])
    check(stream)
    assert ds.oracle_verdict(stream) == raw[13:]
    other = oracle.encode(gi.ct_phantom(3, 256), deflate=True)
    got = hip.decode_batch([other, raw[:12] + b"\x01" + stream, other], hip.default_config())
    assert np.array_equal(got[1], flat) and np.array_equal(got[0], gi.ct_phantom(3, 256)) and np.array_equal(got[2], got[0])
