"""The encode kernels at the 16-bit value edges and regime boundaries of tests/value_edges.py, against the CPU oracle and the
reference's records (tests/golden/value_edges.json): every implementation of stage (i) that takes the shape -- the streaming
kernel with 4, 2 and 1 tiles per workgroup, the tile kernel, the generic kernel, the run-time block size kernels -- each
proven to have run by last_encode_path.  Payload bytes, sizes, statistics, block roles and, on every case and path, the status
word: the Q7 bit is set exactly when the oracle counts a delta outside [-2047, 2048], and no other bit is.  Bit-exact."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

import value_edges as ve

pytestmark = pytest.mark.gpu

CASES = ve.cases()
TILED = [n for n, c in CASES.items() if ve.is_tile_shape(c["spec"])]
OTHER = [n for n, c in CASES.items() if not ve.is_tile_shape(c["spec"])]
DEFAULTS = {"tile_path": 1, "stream_tpg": 4, "runtime_block_size": 0}
# name -> (options, the implementation last_encode_path must report)
TILED_PATHS = {"stream_tpg4": ({"tile_path": 4, "stream_tpg": 4}, 3), "stream_tpg2": ({"tile_path": 4, "stream_tpg": 2}, 3),
               "stream_tpg1": ({"tile_path": 4, "stream_tpg": 1}, 3), "tile": ({"tile_path": 2}, 2), "generic": ({"tile_path": 0}, 0),
               "run_time": ({"runtime_block_size": 1}, 4)}
# shapes the tile paths do not take, and the other block sizes: the kernel compiled for the size (the run-time one where none is)
# and the run-time kernels forced
OTHER_PATHS = {"compiled": ({}, None), "run_time": ({"runtime_block_size": 1}, 4)}


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    info = cct_hip.device_info()  # raises if the extension or the GPU is missing: no fallback
    assert "gfx950" in info["name"]
    return cct_hip


def _config(hip, bs, deflate=False):
    cfg = hip.default_config()
    cfg["verbose"] = False
    cfg["block_size"] = bs
    cfg["encoder"]["deflate_compression"] = deflate
    return cfg


def _option(name):
    from cct_hip import _ffi
    v = C.c_int(-9)
    _ffi.check(_ffi.lib().cct_get_option(name.encode(), C.byref(v)))
    return v.value


def _set_options(opts):
    from cct_hip import _ffi
    for k, v in opts.items():
        _ffi.check(_ffi.lib().cct_set_option(k.encode(), v))


@functools.lru_cache(maxsize=None)
def _want(name):
    """what the oracle makes of a case: file header, payload, statistics, jump table"""
    from oracle import oracle
    img, exp = ve.built(name)
    bs = CASES[name]["spec"]["bs"]
    out, st = oracle.encode(img, block_size=bs, deflate=False, return_stats=True)
    order = oracle.curve(*img.shape)
    _, jumps = oracle.partition(img.reshape(-1)[order].astype(np.int32), order, bs)
    assert st.q7_violations == exp["q7"]
    return {"header": out[:13], "payload": out[13:], "jumps": sorted(jumps.items()), "q7": st.q7_violations > 0,
            "stats": (st.n_short, st.n_full, st.n_jump, st.n_difficult), "payload_len": st.payload_len}


def _encode(hip, imgs, bs, opts, ran):
    """stage (i) of a batch under the given options -> per slice (payload, status, statistics, roles)"""
    from cct_hip import DeviceBuffer, codec_params, encode_payload_dev
    from cct_hip.batch import payload_stride
    imgs = np.ascontiguousarray(imgs)
    n, w, h = imgs.shape
    nb = w * h // bs
    stride = payload_stride(w, h, bs)
    d_img = DeviceBuffer.from_numpy(imgs)
    d_pay, d_sz, d_st = DeviceBuffer(n * stride), DeviceBuffer(4 * n), DeviceBuffer(4 * n)
    d_stats, d_roles = DeviceBuffer(16 * n), DeviceBuffer(n * nb)
    d_pay.zero()
    _set_options(opts)
    try:
        encode_payload_dev(d_img, n, w, h, codec_params(_config(hip, bs), imgs.dtype), d_pay, d_sz, d_st, d_stats, d_roles)
        path = _option("last_encode_path")
    finally:
        _set_options(DEFAULTS)
    if ran is None:
        ran = 0 if bs in (4, 8, 16, 32, 64) else 4
    assert path == ran, "another implementation ran"
    sizes = d_sz.download(np.uint32, n)
    status = d_st.download(np.uint32, n)
    stats = d_stats.download(np.uint32, 4 * n).reshape(n, 4)
    roles = d_roles.download(np.uint8, n * nb).reshape(n, nb)
    return [(d_pay.download(np.uint8, int(sizes[i]), offset=i * stride).tobytes(), int(status[i]), tuple(int(v) for v in stats[i]), roles[i])
            for i in range(n)]


def _first_difference(a, b):
    m = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:m], np.uint8) != np.frombuffer(b[:m], np.uint8))
    return int(d[0]) if d.size else m


def _check(name, got, where=""):
    from cct_hip import _ffi
    want, rec = _want(name), CASES[name]
    payload, status, stats, roles = got
    print(f"{name} {where}: {len(payload)} bytes (oracle {len(want['payload'])}), status {status:#x} (oracle q7 {want['q7']}), stats {stats}")
    assert bool(status & _ffi.ST_Q7) == want["q7"], "the Q7 bit and the oracle's q7_violations disagree"
    assert not status & ~_ffi.ST_Q7, "an unexpected status bit"
    assert len(payload) == want["payload_len"] == len(want["payload"])
    assert payload == want["payload"], f"first differing payload byte: {_first_difference(payload, want['payload'])}"
    assert stats == want["stats"]
    jumps = [(int(b), int(b) + int(r)) for b, r in enumerate(roles) if 0 < r < 0xFF]
    assert jumps == want["jumps"]
    assert {p for _, p in jumps} == {int(b) for b in np.flatnonzero(roles == 0xFF)}
    if "sha1" in rec:   # what the reference wrote (the 1024x1024 case is held to the oracle alone)
        assert 13 + len(payload) == rec["len"] and hashlib.sha1(want["header"] + payload).hexdigest() == rec["sha1"]
        assert (stats[0], stats[1], stats[2]) == (rec["tokens"]["short"], rec["tokens"]["full"], rec["tokens"]["jump"])
        assert hashlib.sha1(np.array(jumps, dtype=np.int32).tobytes()).hexdigest() == rec["jumps_sha1"]


@pytest.mark.parametrize("path", list(TILED_PATHS))
@pytest.mark.parametrize("name", TILED)
def test_tiled_shapes_every_implementation(hip, name, path):
    img, _ = ve.built(name)
    opts, ran = TILED_PATHS[path]
    _check(name, _encode(hip, img[None], 16, opts, ran)[0], path)


@pytest.mark.parametrize("path", list(OTHER_PATHS))
@pytest.mark.parametrize("name", OTHER)
def test_other_shapes_and_block_sizes(hip, name, path):
    img, _ = ve.built(name)
    opts, ran = OTHER_PATHS[path]
    _check(name, _encode(hip, img[None], CASES[name]["spec"]["bs"], opts, ran)[0], path)


def _mixes():
    """slices of one shape and dtype whose groups are in different regimes, interleaved"""
    def pick(side, dtype, *parts):
        return [n for n in TILED if CASES[n]["spec"]["shape"][0] == side and CASES[n]["dtype"] == dtype and any(p in n for p in parts)]
    return {"u16_256": pick(256, "uint16", "tok_", "q7_256_packed_pair", "q7_256_wide_pair", "one_256_v11_pred", "one_256_v14_pred",
                            "fit_256_top04ea", "fit_256_top3fff", "full_256_u16", "full_256_all_max"),
            "u16_128": pick(128, "uint16", "tok_", "_2049", "_m2047", "fit_128", "full_128_checker"),
            "u16_512": pick(512, "uint16", "tok_", "q7_512", "one_512_v11_pred_pair", "one_512_v14_pred_pair", "full_512_u16"),
            "i16_256": pick(256, "int16", "full_")}


@pytest.mark.parametrize("path", list(TILED_PATHS))
@pytest.mark.parametrize("mix", list(_mixes()))
def test_batch_of_mixed_regimes_in_both_orders(hip, mix, path):
    """one launch over slices in different regimes: a slice must not inherit regime flags, hand-off words or status from its
    neighbours in the batch"""
    names = _mixes()[mix]
    assert len(names) >= 3 and (len({_want(n)["q7"] for n in names}) == 2 or mix == "i16_256")
    opts, ran = TILED_PATHS[path]
    for order in (names, names[::-1]):
        got = _encode(hip, np.stack([ve.built(n)[0] for n in order]), 16, opts, ran)
        for n, g in zip(order, got):
            _check(n, g, f"{path} in batch")


@pytest.mark.parametrize("forced", [0, 1], ids=["default", "run_time"])
@pytest.mark.parametrize("name", [n for n in CASES if "decode" in CASES[n]])
def test_device_decodes_like_oracle_and_reference(hip, name, forced):
    """the oracle's file of every case through the device decoder: the oracle's bytes or the oracle's failure, which is also
    what the reference's Decoder did"""
    from oracle import oracle
    rec = CASES[name]
    bs = rec["spec"]["bs"]
    img, _ = ve.built(name)
    want = _want(name)
    blob = want["header"] + want["payload"]
    cfg = _config(hip, bs)
    _set_options({"runtime_block_size": forced})
    try:
        try:
            raster = oracle.decode(blob, block_size=bs)
        except oracle.OracleError as e:
            assert e.code == oracle.E_OVERFLOW and rec["decode"].get("raises") == "OverflowError"
            with pytest.raises(OverflowError):
                hip.decode_batch([blob], cfg)
        else:
            got = hip.decode_batch([blob], cfg)[0].tobytes()
            assert got == raster
            assert hashlib.sha1(got).hexdigest() == rec["decode"]["sha1"]
            assert (got == img.tobytes()) == rec["decode"]["roundtrip"]
            assert _option("last_decode_path") == (1 if forced or bs not in (4, 8, 16, 32, 64) else 0)
    finally:
        _set_options(DEFAULTS)


@pytest.mark.parametrize("name", [n for n in CASES if "deflate" in CASES[n]])
def test_end_to_end_with_deflate(hip, name):
    """one case per family, uint16 and int16, through encode_batch and Encoder(...).encode() with DEFLATE on: the reference's
    file, the oracle's statistics and Q7 flag, and the reference's decoder outcome through Decoder(...).decode()"""
    from codec.core import Decoder, Encoder
    rec, want = CASES[name], _want(name)
    img, _ = ve.built(name)
    cfg = _config(hip, rec["spec"]["bs"], deflate=True)
    files, info = hip.encode_batch(np.ascontiguousarray(img)[None], cfg, return_info=True)
    st = info[0]
    assert (len(files[0]), hashlib.sha1(files[0]).hexdigest()) == (rec["deflate"]["len"], rec["deflate"]["sha1"])
    assert (st["n_short"], st["n_full"], st["n_jump"], st["n_difficult"]) == want["stats"] and st["payload_len"] == want["payload_len"]
    assert st["q7"] == want["q7"]
    enc = Encoder(cfg, np.ascontiguousarray(img))
    assert enc.encode() == files[0]
    assert (enc.info["delta"], enc.info["full"], enc.block_jumps_count) == (rec["tokens"]["short"], rec["tokens"]["full"], rec["tokens"]["jump"])
    if "raises" in rec["decode"]:
        assert rec["decode"]["raises"] == "OverflowError"
        with pytest.raises(OverflowError):
            Decoder(cfg, files[0]).decode()
    else:
        assert hashlib.sha1(Decoder(cfg, files[0]).decode()).hexdigest() == rec["decode"]["sha1"]
