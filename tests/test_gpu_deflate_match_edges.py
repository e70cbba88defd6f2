"""The device DEFLATE matcher on the planted inputs of tests/deflate_match_inputs.py: a string on every off-by-one edge of
longest_match / deflate_slow and of the kernels' own seams (light and cooperative walks, compact sort records, run kernels,
dfl_rec_kernel).  Every case of one configuration goes through one zlib_compress_batch call and every stream must equal
zlib.compressobj(level, DEFLATED, 15, mem_level, strategy)'s.  That the inputs reach their edges is checked without a GPU in
tests/test_deflate_match_inputs_host.py."""
import ctypes as C

import pytest

import deflate_match_inputs as dmi

pytestmark = pytest.mark.gpu

CASES = dmi.cases()


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    cct_hip.device_info()
    return cct_hip


def _first_difference(data, got, want):
    try:
        a, b = dmi.Tokens(*dmi.tokens(got, len(data)), len(data)), dmi.Tokens(*dmi.tokens(want, len(data)), len(data))
        return f"first differing token (position, length, distance): device {a.first_difference(b)[0]}, " \
               f"libz {a.first_difference(b)[1]}"
    except Exception as e:  # the device's stream does not even parse
        k = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), None)
        return f"device stream unreadable ({type(e).__name__}), first differing byte {k}"


def _check(hip, level, strategy=0, mem_level=8, cases=CASES):
    got = hip.zlib_compress_batch([c.data for c in cases], level=level, strategy=strategy, mem_level=mem_level)
    bad = []
    for c, g in zip(cases, got):
        want = dmi.libz(c.data, level, strategy, mem_level)
        if g != want:
            bad.append(f"{c.name} (level {level}, strategy {strategy}, memLevel {mem_level}): {len(g)} vs {len(want)} bytes, "
                       + _first_difference(c.data, g, want))
    assert not bad, f"{len(bad)} of {len(cases)} cases differ from libz:\n" + "\n".join(bad[:20])


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


@pytest.mark.parametrize("level", dmi.LEVELS)
def test_every_edge_equals_libz(hip, level):
    _check(hip, level)


@pytest.mark.parametrize("level", [4, 6, 9])
def test_every_edge_under_z_filtered(hip, level):
    _check(hip, level, strategy=dmi.Z_FILTERED)


@pytest.mark.parametrize("level", [4, 6, 9])
def test_every_edge_at_mem_level_9(hip, level):
    _check(hip, level, mem_level=9)


@pytest.mark.parametrize("level", [4, 7, 9])
def test_every_edge_with_wide_sort_records(hip, level):
    with _Option("deflate_compact_records", 0):
        _check(hip, level)


def test_every_edge_without_the_forked_streams(hip):
    with _Option("deflate_fork", 0):
        _check(hip, 9)


def test_reverse_order_of_the_batch(hip):
    """nothing of a slice leaks into the next one through the tagged match records"""
    _check(hip, 6, cases=CASES[::-1])
