"""The queues of dfl_match_kernel (positions handed to the heavy and the run matcher) on the inputs of
tests/deflate_match_queue_inputs.py: slices in which almost every position is queued, flushes in mid-loop and on the flush
threshold, slice lengths around a wave, a turn and the grid, batches of 1, 7 and 9 slices.  Every batch goes through one
zlib_compress_batch call per configuration and every stream must equal zlib.compressobj(level, DEFLATED, 15, 8, 0)'s.  That
the inputs do what they claim is checked without a GPU in tests/test_deflate_match_queue_inputs_host.py."""
import ctypes as C
import functools

import pytest

import deflate_match_inputs as dmi
import deflate_match_queue_inputs as qi

pytestmark = pytest.mark.gpu

BATCHES = qi.batches()


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    cct_hip.device_info()
    return cct_hip


@functools.lru_cache(maxsize=None)
def _libz(data, level):
    return dmi.libz(data, level)


class _Option:
    """a library option set for the length of a with block and put back afterwards"""

    def __init__(self, name, value):
        self.name, self.value, self.old = name.encode(), value, C.c_int(0)

    def __enter__(self):
        from cct_hip import _ffi
        _ffi.check(_ffi.lib().cct_get_option(self.name, C.byref(self.old)))
        _ffi.check(_ffi.lib().cct_set_option(self.name, self.value))

    def __exit__(self, *exc):
        from cct_hip import _ffi
        _ffi.check(_ffi.lib().cct_set_option(self.name, self.old.value))


def _check(hip, slices, level):
    got = hip.zlib_compress_batch(slices, level=level)
    assert len(got) == len(slices)
    bad = []
    for k, (d, g) in enumerate(zip(slices, got)):
        want = _libz(d, level)
        if g != want:
            at = next((i for i in range(min(len(g), len(want))) if g[i] != want[i]), min(len(g), len(want)))
            bad.append(f"slice {k} ({len(d)} bytes, level {level}): {len(g)} vs {len(want)} bytes, first differing byte {at}")
    assert not bad, f"{len(bad)} of {len(slices)} streams differ from libz:\n" + "\n".join(bad)


@pytest.mark.parametrize("level", [4, 9])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_compact_records(hip, name, level):
    _check(hip, BATCHES[name], level)


@pytest.mark.parametrize("level", [4, 9])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_wide_records(hip, name, level):
    with _Option("deflate_compact_records", 0):
        _check(hip, BATCHES[name], level)


def test_wide_records_flush_in_mid_loop(hip):
    with _Option("deflate_compact_records", 0):
        _check(hip, qi.wide_long(), 9)


def test_short_slices_after_long_ones(hip):
    """the counts and lists of a slice are those of this call: a batch of short slices after one whose waves flushed many times"""
    _check(hip, BATCHES["long_and_short"], 9)
    _check(hip, BATCHES["short"][::-1], 9)
