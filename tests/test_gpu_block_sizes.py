"""Block sizes that are not powers of two on the device: encode_kernel<0> / decode_kernel<0> (a run-time block size)
against the reference-generated fixtures of tests/golden/block_sizes.json and against the CPU oracle, and the same
kernels forced onto the power-of-two sizes (option "runtime_block_size") against the kernels compiled for them."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import block_size_inputs as bsi
import golden_inputs as gi

pytestmark = pytest.mark.gpu

with open(os.path.join(gi.GOLDEN, "block_sizes.json")) as _f:
    CASES = {c["name"]: c for c in json.load(_f)["cases"]}
with open(os.path.join(gi.GOLDEN, "manifest.json")) as _f:
    POW2 = {c["name"]: c for c in json.load(_f)["cases"] if "encode_raises" not in c}


def config(over):
    from cct_hip import default_config
    cfg = default_config()
    cfg["verbose"] = False
    cfg["block_size"] = over.get("block_size", 16)
    cfg["encoder"]["transforms"]["fractal"] = over.get("fractal", True)
    cfg["encoder"]["transforms"]["segmentation"] = over.get("segmentation", True)
    cfg["encoder"]["deflate_compression"] = over.get("deflate", True)
    return cfg


def option(name):
    from cct_hip import _ffi
    v = C.c_int(-9)
    _ffi.check(_ffi.lib().cct_get_option(name.encode(), C.byref(v)))
    return v.value


def set_option(name, value):
    from cct_hip import _ffi
    _ffi.check(_ffi.lib().cct_set_option(name.encode(), value))


@pytest.fixture(scope="module")
def hip():
    import cct_hip
    assert "gfx950" in cct_hip.device_info()["name"]  # raises if the extension or the GPU is missing: no fallback
    return cct_hip


@pytest.fixture
def forced(hip):
    set_option("runtime_block_size", 1)
    try:
        yield
    finally:
        set_option("runtime_block_size", 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_encode_matches_reference(hip, name):
    from codec.core import Encoder
    case = CASES[name]
    img = bsi.build_input(case["input"])
    assert gi.sha1(img.tobytes()) == case["input_sha1"]
    enc = Encoder(config(case["config"]), img)
    out = enc.encode()
    assert option("last_encode_path") == 4
    assert len(out) == case["len"] and hashlib.sha1(out).hexdigest() == case["sha1"]
    if "file" in case:
        with open(os.path.join(gi.GOLDEN, case["file"]), "rb") as f:
            assert out == f.read()
    assert (enc.info["delta"], enc.info["full"]) == (case["tokens"]["short"], case["tokens"]["full"])
    if "jump" in case["tokens"]:
        assert enc.block_jumps_count == case["tokens"]["jump"]
        order, jumps = enc.partition.block_partition()
        assert len(jumps) == case["tokens"]["jump"]
        assert gi.sha1(np.array(sorted(jumps.items()), dtype=np.int32).reshape(-1, 2).tobytes()) == case["jumps_sha1"]
        # PIXEL_ORDER: every pixel once, pairs interleaved
        assert np.array_equal(np.sort(order), np.arange(img.size))


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if "file" in c))
def test_decoder_restores_reference_files(hip, name):
    from codec.core import Decoder
    case = CASES[name]
    with open(os.path.join(gi.GOLDEN, case["file"]), "rb") as f:
        blob = f.read()
    dec = Decoder(config(case["config"]), blob)
    raster = dec.decode()
    assert option("last_decode_path") == 1
    assert hashlib.sha1(raster).hexdigest() == case["decoded_sha1"]
    assert raster == bsi.build_input(case["input"]).tobytes()
    assert len(dec.fulls) == case["tokens"]["full"]


def test_large_batch_bs12_vs_oracle(hip):
    """64 slices of 384^2 at block size 12 (NB = 12288: role and slot tables in LDS, lists spilled to HBM on the noisy
    slices) through encode_batch (packed archive, device DEFLATE) and decode_batch."""
    from oracle import oracle
    cfg = config({"block_size": 12})
    imgs = np.stack([bsi.build_input({"kind": "phantom_noise", "seed": 100 + i, "n": 384, "amp": 90 if i % 2 else 0})
                     for i in range(64)])
    files = hip.encode_batch(imgs, cfg)
    assert option("last_encode_path") == 4
    for i in range(64):
        assert files[i] == oracle.encode(imgs[i], block_size=12), i
    back = hip.decode_batch(files, cfg)
    assert option("last_decode_path") == 1
    assert np.array_equal(np.asarray(back).reshape(imgs.shape), imgs)


def test_small_blocks_hbm_tables(hip):
    """768^2 at block size 3: 196 608 blocks, role table of the encoder and slot table of the decoder in HBM."""
    from oracle import oracle
    cfg = config({"block_size": 3})
    case = CASES["noise768_bs3"]
    img = bsi.build_input(case["input"])
    imgs = np.stack([img, gi.ct_phantom(6, 768)])
    files = hip.encode_batch(imgs, cfg)
    assert hashlib.sha1(files[0]).hexdigest() == case["sha1"]
    assert files[1] == oracle.encode(imgs[1], block_size=3)
    assert np.array_equal(np.asarray(hip.decode_batch(files, cfg)).reshape(imgs.shape), imgs)


@pytest.mark.parametrize("name", sorted(POW2))
def test_forced_run_time_kernels_equal_compiled_ones(hip, name):
    """Every power-of-two fixture of manifest.json: the run-time block size kernels give the bytes and rasters of the
    kernels compiled for the size (and of the tile / streaming paths at block size 16)."""
    from codec.core import Decoder, Encoder
    case = POW2[name]
    img = gi.build_input(case["input"])
    cfg = config(case["config"])
    res = []
    for force in (0, 1):
        set_option("runtime_block_size", force)
        try:
            enc = Encoder(cfg, img)
            out = enc.encode()
            assert (option("last_encode_path") == 4) == bool(force)
            try:
                raster = Decoder(cfg, out).decode()
            except (OverflowError, ValueError) as e:  # the Q7 fixtures: the reference raises too
                raster = type(e).__name__
            assert (option("last_decode_path") == 1) == bool(force)
            res.append((out, dict(enc.info), raster))
        finally:
            set_option("runtime_block_size", 0)
    assert res[0] == res[1]
    assert hashlib.sha1(res[1][0]).hexdigest() == case["sha1"]


def test_forced_run_time_kernels_phantom_batch(hip, forced):
    """8 phantoms of 512^2 at block size 16 through the forced run-time kernels: the oracle's bytes, exact rasters."""
    from oracle import oracle
    cfg = config({})
    imgs = np.stack([gi.ct_phantom(200 + i, 512) for i in range(8)])
    files = hip.encode_batch(imgs, cfg)
    assert option("last_encode_path") == 4
    assert all(files[i] == oracle.encode(imgs[i]) for i in range(8))
    back = hip.decode_batch(files, cfg)
    assert option("last_decode_path") == 1
    assert np.array_equal(np.asarray(back).reshape(imgs.shape), imgs)


def test_options(hip):
    assert option("runtime_block_size") == 0
    set_option("runtime_block_size", 1)
    try:
        assert option("runtime_block_size") == 1
    finally:
        set_option("runtime_block_size", 0)
    cfg = config({})
    f = hip.encode_batch(gi.ct_phantom(1, 128)[None], cfg)
    assert option("last_encode_path") == 3  # 128x128: the streaming kernel
    hip.decode_batch(f, cfg)
    assert option("last_decode_path") == 0


def test_sizes_outside_3_to_64_still_refused(hip):
    img = np.zeros((96, 65), dtype=np.uint16)  # 6240 pixels: divisible by 1, 2, 5, 65 and 96
    for bs in (1, 2, 65, 96):
        with pytest.raises(ValueError, match="block_size"):
            hip.encode_batch(img[None], config({"block_size": bs}))
    f = hip.encode_batch(img[None], config({"block_size": 5}))
    for bs in (1, 2, 65, 96):
        with pytest.raises(ValueError, match="block_size"):
            hip.decode_batch(f, config({"block_size": bs}))
    with pytest.raises(ValueError, match="cannot reshape"):
        hip.encode_batch(img[None], config({"block_size": 7}))
