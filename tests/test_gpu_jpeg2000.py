"""Device JPEG 2000 lossless encoder (cct_j2k_encode_batch) against tests/jpeg2000_model.py: files byte for byte over shapes,
contents, precisions, levels and code-block sizes, host and device inputs, per-frame overflow, refusals before the device,
jpeg2000_info, Pillow's OpenJPEG on the device's files, the two real slices, and the JP2 column of tools/evaluate.py."""
import functools
import importlib.util
import io
import os

import numpy as np
import pytest

import golden_inputs as gi
import jpeg2000_model as m
from test_jpeg2000_model import MARGIN, as_pillow_returns, pillow_decode, pillow_has_jpeg2000

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_CAP, E_ARG, E_J2K = 3, 6, 9, 14


@pytest.mark.parametrize("precision", sorted(m.PRECISIONS))
def test_encode_equals_the_model(precision):
    import cct_hip
    bound = cct_hip._ffi.lib().cct_j2k_bound
    for rows, cols, cb, levels, names, imgs, files in m.matrix(precision):
        got = cct_hip.jpeg2000_encode_batch(imgs, precision=precision, levels=levels, codeblock=cb)  # one mixed batch per shape
        for name, g, want in zip(names, got, files):
            assert g == want, (rows, cols, cb, levels, name)
            assert len(g) <= bound(rows, cols, levels, cb, 0)


def test_encode_phantoms_noise_shift_and_jp2():
    import cct_hip
    for img, kw, want in m.phantoms():
        got = cct_hip.jpeg2000_encode_batch(img, **kw)
        assert got == [want], kw
        assert len(want) <= cct_hip._ffi.lib().cct_j2k_bound(128, 128, kw["levels"], kw["codeblock"], int(kw.get("jp2", False)))
    noise = m.phantoms()[4][2]
    data = m.packet_data(noise)
    assert sum(1 for k in range(len(data) - 1) if data[k] == 0xFF and data[k + 1] < 0x90) > 50  # stuffed sequences


def test_known_answer():
    import cct_hip
    img = np.array([[0, 65535, 0, 32768, 0, 32767, 65535, 1]], dtype=np.uint16)
    want = ("ff4fff5100290000000000080000000100000000000000000000000800000001000000000000000000010f0101ff52000c00000001000004040001"
            "ff5c00044080ff90000a0000000000240001ff93dff8909005884024fcf07e34388ff59232244890c30fffd9")
    assert cct_hip.jpeg2000_encode_batch(img, levels=0)[0].hex() == want


def test_host_and_device_inputs():
    import cct_hip
    imgs = np.stack([p[0] for p in m.phantoms()[:2]])
    want = [m.phantoms()[0][2], m.encode(imgs[1], 16, 0, 5, 64)]
    assert cct_hip.jpeg2000_encode_batch(imgs) == want
    d = cct_hip.DeviceBuffer.from_numpy(imgs)
    try:
        assert cct_hip.jpeg2000_encode_batch(d, shape=imgs.shape) == want
        assert cct_hip.jpeg2000_encode_batch(d, shape=imgs.shape[1:]) == want[:1]
    finally:
        d.free()
    low = np.minimum(imgs[:1] >> 3, 255).astype(np.uint8)
    assert cct_hip.jpeg2000_encode_batch(low, levels=2, codeblock=32) == [m.encode(low[0], 8, 0, 2, 32)]
    assert cct_hip.jpeg2000_encode_batch(np.zeros((0, 4, 4), np.uint16)) == []


def test_overflow_is_per_frame():
    import cct_hip
    L = cct_hip._ffi.lib()
    imgs = np.random.default_rng(2).integers(0, 4096, (4, 6, 70)).astype(np.uint16)
    imgs[1, 5, 69] = 4096
    imgs[3, 0, 0] = 65535
    stride = L.cct_j2k_bound(6, 70, 5, 64, 0)
    out = np.zeros((4, stride), np.uint8)
    sizes, status = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    rc = L.cct_j2k_encode_batch(imgs.ctypes.data, 0, 4, 6, 70, 16, 12, 0, 5, 64, 0, out.ctypes.data, stride, sizes.ctypes.data, status.ctypes.data)
    assert rc == E_OVERFLOW and list(status) == [0, E_OVERFLOW, 0, E_OVERFLOW] and sizes[1] == sizes[3] == 0
    for i in (0, 2):
        assert out[i, :sizes[i]].tobytes() == m.encode(imgs[i], 12)
    with pytest.raises(OverflowError):
        cct_hip.jpeg2000_encode_batch(imgs, precision=12)
    with pytest.raises(OverflowError):
        cct_hip.jpeg2000_encode_batch(imgs[:1], precision=16, shift=5)  # 4095 << 5 needs 17 bits


def test_refusals_before_the_device():
    import cct_hip
    L = cct_hip._ffi.lib()
    img = np.zeros((1, 8, 8), np.uint16)
    stride = L.cct_j2k_bound(8, 8, 5, 64, 0)
    assert stride > 0 and L.cct_j2k_bound(8, 8, 9, 64, 0) == 0 and L.cct_j2k_bound(8, 8, 5, 16, 0) == 0 and L.cct_j2k_bound(0, 8, 5, 64, 0) == 0
    out = np.zeros(stride, np.uint8)
    sizes, status = np.zeros(1, np.uint32), np.zeros(1, np.uint32)

    def call(src_bits=16, precision=16, shift=0, levels=5, codeblock=64, out_stride=stride, rows=8, cols=8):
        return L.cct_j2k_encode_batch(img.ctypes.data, 0, 1, rows, cols, src_bits, precision, shift, levels, codeblock, 0, out.ctypes.data, out_stride,
                                      sizes.ctypes.data, status.ctypes.data)
    assert call() == 0
    for bad in (dict(precision=1), dict(precision=17), dict(src_bits=8, precision=9), dict(src_bits=12), dict(shift=-1), dict(shift=16),
                dict(precision=4, shift=4), dict(levels=-1), dict(levels=9), dict(codeblock=16), dict(codeblock=128), dict(codeblock=48),
                dict(rows=0), dict(cols=65536), dict(rows=65535, cols=65535)):
        assert call(**bad) == E_ARG, bad
    assert call(out_stride=stride - 1) == E_CAP
    for bad in (dict(precision=1), dict(precision=17), dict(shift=16), dict(precision=4, shift=4), dict(levels=9), dict(codeblock=48)):
        with pytest.raises(ValueError):
            cct_hip.jpeg2000_encode_batch(img, **bad)
    with pytest.raises(ValueError):
        cct_hip.jpeg2000_encode_batch(img.astype(np.uint8), precision=9)
    with pytest.raises(TypeError):
        cct_hip.jpeg2000_encode_batch(img.astype(np.int32))


def test_info():
    import cct_hip
    img = m.raster_cases(5, 3, 12, np.uint16)["ramp"]
    raw, jp2 = m.encode(img, 12, levels=1), m.encode(img, 12, levels=1, jp2=True)
    assert cct_hip.jpeg2000_info(raw) == cct_hip.jpeg2000_info(jp2) == (5, 3, 12)
    for bad in (b"", raw[:40], raw[:4], b"\x89PNG\r\n\x1a\n" + bytes(64), jp2[:77], jp2[:85].replace(b"jp2c", b"free") + raw, raw[:2] + b"\xff\x52" + raw[4:],
                raw[:41] + b"\x02" + raw[42:], raw[:42] + b"\x8b" + raw[43:]):
        with pytest.raises(ValueError):
            cct_hip.jpeg2000_info(bad)
        with pytest.raises(ValueError):
            m.info(bad)
    assert cct_hip._ffi.lib().cct_j2k_info(b"", 0, None, None, None) == E_ARG
    if pillow_has_jpeg2000():
        from PIL import Image
        for arr, no_jp2 in ((np.zeros((9, 14), np.uint8), False), (np.zeros((3, 200), np.uint16), True)):
            buf = io.BytesIO()
            Image.fromarray(arr).save(buf, "JPEG2000", irreversible=False, no_jp2=no_jp2)
            assert cct_hip.jpeg2000_info(buf.getvalue()) == m.info(buf.getvalue()) == arr.shape + (8 * arr.itemsize,)


def test_pillow_decodes_the_devices_files():
    if not pillow_has_jpeg2000():
        pytest.skip("this Pillow has no JPEG 2000 codec")
    import cct_hip
    for img, kw, _ in m.phantoms():
        _, got = pillow_decode(cct_hip.jpeg2000_encode_batch(img, **kw)[0])
        assert np.array_equal(got.astype(np.int64), as_pillow_returns(img, kw["precision"], kw.get("shift", 0))), kw
    noise = np.random.default_rng(4).integers(0, 256, (3, 19, 23)).astype(np.uint8)
    for f, x in zip(cct_hip.jpeg2000_encode_batch(noise, levels=2, codeblock=32, jp2=True), noise):
        assert np.array_equal(pillow_decode(f)[1], x)


@functools.lru_cache(maxsize=None)
def real_slices():
    return np.stack([gi.load_slice("slice0671"), gi.load_slice("slice3706")])


def test_real_slices_full_size():
    """512 x 512, where the model is not run: Pillow decodes the files and its own files set the size.  Without Pillow's codec
    the margin-free assertions remain."""
    import cct_hip
    L = cct_hip._ffi.lib()
    imgs = real_slices()
    for shift, jp2 in ((4, True), (0, False)):
        stride = L.cct_j2k_bound(512, 512, 5, 64, int(jp2))
        out = np.zeros((2, stride), np.uint8)
        sizes, status = np.zeros(2, np.uint32), np.ones(2, np.uint32)
        rc = L.cct_j2k_encode_batch(imgs.ctypes.data, 0, 2, 512, 512, 16, 16, shift, 5, 64, int(jp2), out.ctypes.data, stride, sizes.ctypes.data,
                                    status.ctypes.data)
        assert rc == 0 and list(status) == [0, 0]
        files = cct_hip.jpeg2000_encode_batch(imgs, precision=16, shift=shift, jp2=jp2)
        for i, (f, x) in enumerate(zip(files, imgs)):
            assert f == out[i, :sizes[i]].tobytes() and 0 < len(f) <= stride
            assert cct_hip.jpeg2000_info(f) == (512, 512, 16)
            if pillow_has_jpeg2000():
                from PIL import Image
                assert np.array_equal(pillow_decode(f)[1], x.astype(np.uint32) << shift)
                buf = io.BytesIO()
                Image.fromarray((x.astype(np.uint32) << shift).astype(np.uint16)).save(buf, "JPEG2000", irreversible=False, num_resolutions=6,
                                                                                      codeblock_size=(64, 64), no_jp2=not jp2)
                print(f"slice {i} shift {shift}: device {len(f)} B, OpenJPEG {buf.tell()} B")
                assert len(f) <= buf.tell() * (1 + MARGIN)


def test_evaluate_tool_fills_the_jp2_column(tmp_path):
    import cct_hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("evaluate_tool_j2k", os.path.join(root, "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    imgs = real_slices()
    for k, img in enumerate(imgs):
        np.save(tmp_path / f"slice{k}.npy", img)
    out = tmp_path / "out.csv"

    def column(*flags):
        assert tool.main([str(tmp_path), "--results", str(out), *flags]) == 0
        lines = out.read_text().splitlines()
        assert lines[0] == "File,Raw,ZIP,PNG,RLE,JP2,CCT"
        return [ln.split(",")[5] for ln in lines[1:]], [ln.split(",")[:5] + ln.split(",")[6:] for ln in lines[1:]]
    preview, rest = column("--jp2", "device")
    assert [int(v) for v in preview] == [len(f) for f in cct_hip.jpeg2000_encode_batch(imgs, precision=16, shift=4, jp2=True)]
    native, rest_native = column("--jp2", "device-native")
    assert [int(v) for v in native] == [len(f) for f in cct_hip.jpeg2000_encode_batch(imgs, precision=16, shift=0, jp2=True)]
    assert all(int(a) < int(b) for a, b in zip(native, preview))
    plain, rest_plain = column()
    assert plain == ["NA", "NA"] and rest == rest_native == rest_plain  # the other columns are what they were


def test_batches_of_several_passes_equal_single_frames():
    """A frame of 512 x 512 holds 8 bytes a sample of planes, its slabs and its file on the device, 4.78 MB with both at
    cct_j2k_bound's 1.34 MB, so a pass of 512 MiB (csrc/api_jpeg2000.cpp J2K_PASS_BYTES) takes 112 and 120 frames run as 112 + 8."""
    import cct_hip
    bound = cct_hip._ffi.lib().cct_j2k_bound(512, 512, 5, 64, 0)
    assert 100 < (512 << 20) // (8 * 512 * 512 + 2 * bound) < 120
    two = real_slices()
    files = cct_hip.jpeg2000_encode_batch(np.stack([two[i % 2] for i in range(120)]))
    want = cct_hip.jpeg2000_encode_batch(two)
    assert files == [want[i % 2] for i in range(120)]
