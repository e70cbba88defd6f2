"""Argument refusals of the batch entry points, pinned without a device: the exact exception type and message of every
check that cct_hip/batch.py makes "before any device call", the order of those checks (inputs with two faults), the
empty-batch results, and on the C side (return code, cct_last_error()) of the whole-call refusals that answer before the
device is touched.  The expected answers are tests/golden/batch_refusals.json, written by tools/gen_batch_refusals.py from
the case tables below; no case here reaches a device call, so the file is the same with and without a GPU."""
import json
import os
import struct

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_refusals.json")


def dev(nbytes):
    """a DeviceBuffer that owns nothing: the argument checks read its nbytes only"""
    import cct_hip
    d = cct_hip.DeviceBuffer.__new__(cct_hip.DeviceBuffer)
    d.nbytes, d.ptr = nbytes, 0
    return d


def u8(*shape):
    return np.zeros(shape, np.uint8)


def u16(*shape):
    return np.zeros(shape, np.uint16)


def f32(*shape):
    return np.zeros(shape, np.float32)


def huge(dtype, *shape):
    """an array of that shape which owns one element"""
    return np.broadcast_to(np.zeros((), dtype), shape)


def png_head(rows, cols, depth=16):
    """signature and IHDR: all that png_info reads"""
    return b"\x89PNG\r\n\x1a\n" + struct.pack(">I4sIIBBBBB", 13, b"IHDR", cols, rows, depth, 0, 0, 0, 0) + b"\0\0\0\0"


def python_cases():
    """id -> call; each one raises in batch.py or returns an empty batch"""
    import cct_hip as h
    pe, p8, d8, pr, zc = h.png_encode_batch, h.png8_encode_batch, h.decode_png8_batch, h.png_read_batch, h.zlib_compress_batch
    re, rd, je, jd = h.dicom_rle_encode_batch, h.dicom_rle_decode_batch, h.jpeg_lossless_encode_batch, h.jpeg_lossless_decode_batch
    c = {}

    # png_encode_batch
    c["pe.level_float"] = lambda: pe(u16(1, 4, 4), level=6.0)
    c["pe.level_bool"] = lambda: pe(u16(1, 4, 4), level=True)
    c["pe.level_3"] = lambda: pe(u16(1, 4, 4), level=3)
    c["pe.level_10"] = lambda: pe(u16(1, 4, 4), level=10)
    c["pe.shift_str"] = lambda: pe(u16(1, 4, 4), shift="1")
    c["pe.shift_bool"] = lambda: pe(u16(1, 4, 4), shift=False)
    c["pe.shift_16"] = lambda: pe(u16(1, 4, 4), shift=16)
    c["pe.shift_neg"] = lambda: pe(u16(1, 4, 4), shift=-1)
    c["pe.order.level_then_shift"] = lambda: pe(u16(1, 4, 4), level=3, shift=99)
    c["pe.order.shift_then_dtype"] = lambda: pe(f32(4), shift=16)
    c["pe.order.dtype_then_rank"] = lambda: pe(f32(4))
    c["pe.order.dtype_then_shape"] = lambda: pe(f32(1, 0, 4))
    c["pe.order.rank_then_shape"] = lambda: pe(u16(1, 1, 0, 4))
    c["pe.dtype_float"] = lambda: pe(f32(1, 4, 4))
    c["pe.dtype_u8"] = lambda: pe(u8(1, 4, 4))
    c["pe.rank_1"] = lambda: pe(u16(4))
    c["pe.rank_4"] = lambda: pe(u16(1, 1, 4, 4))
    c["pe.rows_0"] = lambda: pe(u16(1, 0, 4))
    c["pe.cols_0_2d"] = lambda: pe(u16(4, 0))
    c["pe.too_many_filtered_bytes"] = lambda: pe(huge(np.uint16, 1, 40000, 40000))
    c["pe.empty"] = lambda: pe(u16(0, 4, 4))
    c["pe.empty_shape_beside_an_array_passes"] = lambda: pe(u16(0, 4, 4), shape=(9, 9, 9))
    c["pe.dev.no_shape"] = lambda: pe(dev(64))
    c["pe.dev.shape_rank_1"] = lambda: pe(dev(64), shape=(4,))
    c["pe.dev.shape_rank_4"] = lambda: pe(dev(64), shape=(1, 2, 3, 4))
    c["pe.dev.negative_n"] = lambda: pe(dev(64), shape=(-1, 4, 4))
    c["pe.dev.too_small_2d"] = lambda: pe(dev(31), shape=(4, 4))
    c["pe.dev.too_small_3d"] = lambda: pe(dev(63), shape=(2, 4, 4))
    c["pe.dev.order.fit_then_shape"] = lambda: pe(dev(0), shape=(1, 40000, 40000))
    c["pe.dev.order.shape_after_fit"] = lambda: pe(dev(64), shape=(1, 0, 4))
    c["pe.dev.order.shape_then_empty"] = lambda: pe(dev(64), shape=(0, 0, 4))
    c["pe.dev.order.level_then_shape_arg"] = lambda: pe(dev(64), level=2)
    c["pe.dev.empty"] = lambda: pe(dev(0), shape=(0, 4, 4))

    # png8_encode_batch
    c["p8.level_float"] = lambda: p8(u8(1, 4, 4), level=6.5)
    c["p8.level_2"] = lambda: p8(u8(1, 4, 4), level=2)
    c["p8.order.level_first"] = lambda: p8("junk", level=2)
    c["p8.arr_with_shape"] = lambda: p8(u8(1, 4, 4), shape=(1, 4, 4))
    c["p8.arr_with_dtype"] = lambda: p8(u8(1, 4, 4), dtype=np.uint8)
    c["p8.rank_1"] = lambda: p8(u8(4))
    c["p8.rank_4"] = lambda: p8(u8(1, 1, 4, 4))
    c["p8.order.rank_then_dtype"] = lambda: p8(f32(4))
    c["p8.u8_with_window"] = lambda: p8(u8(1, 4, 4), window=(0, 255))
    c["p8.u16_without_window"] = lambda: p8(u16(1, 4, 4))
    c["p8.window_str"] = lambda: p8(u16(1, 4, 4), window="ab")
    c["p8.window_int"] = lambda: p8(u16(1, 4, 4), window=5)
    c["p8.window_triple"] = lambda: p8(u16(1, 4, 4), window=(1, 2, 3))
    c["p8.window_float"] = lambda: p8(u16(1, 4, 4), window=(1.0, 2))
    c["p8.window_bool"] = lambda: p8(u16(1, 4, 4), window=(True, 2))
    c["p8.window_equal"] = lambda: p8(u16(1, 4, 4), window=(5, 5))
    c["p8.window_above"] = lambda: p8(u16(1, 4, 4), window=(0, 65536))
    c["p8.window_below"] = lambda: p8(u16(1, 4, 4), window=(-1, 5))
    c["p8.dtype_float"] = lambda: p8(f32(1, 4, 4))
    c["p8.order.dtype_then_shape"] = lambda: p8(f32(1, 0, 4))
    c["p8.order.window_then_shape"] = lambda: p8(u8(1, 0, 4), window=(0, 1))
    c["p8.order.window_value_then_shape"] = lambda: p8(u16(1, 0, 4), window=(5, 5))
    c["p8.rows_0"] = lambda: p8(u8(1, 0, 4))
    c["p8.too_many_filtered_bytes"] = lambda: p8(huge(np.uint8, 1, 40000, 40000))
    c["p8.empty"] = lambda: p8(u8(0, 4, 4))
    c["p8.empty_u16"] = lambda: p8(u16(0, 4, 4), window=(0, 9))
    c["p8.dev.nothing"] = lambda: p8(dev(64))
    c["p8.dev.no_dtype"] = lambda: p8(dev(64), shape=(4, 4))
    c["p8.dev.no_shape"] = lambda: p8(dev(64), dtype=np.uint8)
    c["p8.dev.dtype_nonsense"] = lambda: p8(dev(64), shape=(4, 4), dtype="nonsense")
    c["p8.dev.dtype_float"] = lambda: p8(dev(64), shape=(4, 4), dtype=np.float32)
    c["p8.dev.shape_rank_1"] = lambda: p8(dev(64), shape=(4,), dtype=np.uint8)
    c["p8.dev.u8_too_small"] = lambda: p8(dev(15), shape=(4, 4), dtype=np.uint8)
    c["p8.dev.u16_too_small"] = lambda: p8(dev(31), shape=(4, 4), dtype=np.uint16, window=(0, 100))
    c["p8.dev.negative_n"] = lambda: p8(dev(64), shape=(-1, 4, 4), dtype=np.uint8)
    c["p8.dev.order.shape_then_fit"] = lambda: p8(dev(0), shape=(1, 0, 4), dtype=np.uint8)
    c["p8.dev.order.window_then_fit"] = lambda: p8(dev(0), shape=(1, 4, 4), dtype=np.uint16)
    c["p8.dev.empty"] = lambda: p8(dev(0), shape=(0, 4, 4), dtype=np.uint8)

    # decode_png8_batch
    c["d8.window_str"] = lambda: d8([], "ab")
    c["d8.window_order"] = lambda: d8([], (9, 3))
    c["d8.level_float"] = lambda: d8([], (0, 9), level=1.5)
    c["d8.level_1"] = lambda: d8([], (0, 9), level=1)
    c["d8.files_bytes"] = lambda: d8(b"file", (0, 9))
    c["d8.files_str"] = lambda: d8("file", (0, 9))
    c["d8.file_is_str"] = lambda: d8([b"", "file"], (0, 9))
    c["d8.file_is_int"] = lambda: d8([7], (0, 9))
    c["d8.order.window_then_level"] = lambda: d8(b"file", (9, 3), level=1)
    c["d8.order.level_then_files"] = lambda: d8(b"file", (0, 9), level=1)
    c["d8.empty"] = lambda: d8([], (0, 9))

    # png_read_batch
    c["pr.shift_float"] = lambda: pr([], shift=1.0)
    c["pr.shift_bool"] = lambda: pr([], shift=True)
    c["pr.shift_16"] = lambda: pr([], shift=16)
    c["pr.files_bytes"] = lambda: pr(b"file")
    c["pr.files_str"] = lambda: pr("file")
    c["pr.file_is_str"] = lambda: pr(["file"])
    c["pr.file_is_none"] = lambda: pr([b"", None])
    c["pr.out_dev_type"] = lambda: pr([], out_dev=u16(4))
    c["pr.order.shift_then_files"] = lambda: pr(b"file", shift=16)
    c["pr.order.files_then_out_dev"] = lambda: pr(["file"], out_dev="x")
    c["pr.empty"] = lambda: pr([])
    c["pr.empty_status"] = lambda: pr([], raise_errors=False)
    c["pr.empty_dev"] = lambda: pr([], out_dev=dev(0))
    c["pr.empty_dev_status"] = lambda: pr([], out_dev=dev(0), raise_errors=False)
    c["pr.not_a_png"] = lambda: pr([b"junk"])
    c["pr.not_a_png_status"] = lambda: pr([b"junk"], raise_errors=False)
    c["pr.depth_4"] = lambda: pr([png_head(4, 4, 4)])
    c["pr.too_many_filtered_bytes"] = lambda: pr([png_head(40000, 40000)])
    c["pr.out_dev_too_small"] = lambda: pr([png_head(4, 4)], out_dev=dev(31))
    c["pr.out_dev_too_small_2"] = lambda: pr([png_head(4, 4), b""], out_dev=dev(63))

    # zlib_compress_batch
    c["zc.strategy_bool"] = lambda: zc([b"a"], strategy=True)
    c["zc.strategy_str"] = lambda: zc([b"a"], strategy="0")
    c["zc.strategy_float"] = lambda: zc([b"a"], strategy=1.5)
    c["zc.strategy_5"] = lambda: zc([b"a"], strategy=5)
    c["zc.strategy_neg"] = lambda: zc([b"a"], strategy=-1)
    c["zc.level_3"] = lambda: zc([b"a"], level=3)
    c["zc.level_10"] = lambda: zc([b"a"], level=10)
    c["zc.level_0_huffman"] = lambda: zc([b"a"], level=0, strategy=2)
    c["zc.level_10_rle"] = lambda: zc([b"a"], level=10, strategy=3)
    c["zc.level_true_is_1"] = lambda: zc([b"a"], level=True)
    c["zc.mem_level_7"] = lambda: zc([b"a"], mem_level=7)
    c["zc.mem_level_bool"] = lambda: zc([b"a"], mem_level=True)
    c["zc.mem_level_str"] = lambda: zc([b"a"], mem_level="8")
    c["zc.order.strategy_then_level"] = lambda: zc([b"a"], level=3, strategy=9)
    c["zc.order.level_then_mem_level"] = lambda: zc([b"a"], level=3, mem_level=7)
    c["zc.empty"] = lambda: zc([])
    c["zc.empty_level_minus_1"] = lambda: zc([], level=-1, strategy=4, mem_level=9)

    # the two frame encoders share the shape of their checks
    for k, enc, px_rows, px_cols in (("re", re, 8192, 8193), ("je", je, 8193, 8192)):
        c[k + ".arr_with_shape"] = lambda enc=enc: enc(u16(1, 4, 4), shape=(1, 4, 4))
        c[k + ".arr_with_dtype"] = lambda enc=enc: enc(u16(1, 4, 4), dtype=np.uint16)
        c[k + ".rank_1"] = lambda enc=enc: enc(u16(4))
        c[k + ".rank_4"] = lambda enc=enc: enc(u16(1, 1, 4, 4))
        c[k + ".order.rank_then_dtype"] = lambda enc=enc: enc(f32(4))
        c[k + ".dtype_float"] = lambda enc=enc: enc(f32(1, 4, 4))
        c[k + ".dtype_i16"] = lambda enc=enc: enc(np.zeros((1, 4, 4), np.int16))
        c[k + ".order.dtype_then_empty"] = lambda enc=enc: enc(f32(0, 4, 4))
        c[k + ".order.dtype_then_shape"] = lambda enc=enc: enc(f32(1, 0, 4))
        c[k + ".empty"] = lambda enc=enc: enc(u16(0, 4, 4))
        c[k + ".empty_u8"] = lambda enc=enc: enc(u8(0, 4, 4))
        c[k + ".order.empty_then_shape"] = lambda enc=enc: enc(u16(0, 0, 4))
        c[k + ".rows_0"] = lambda enc=enc: enc(u16(1, 0, 4))
        c[k + ".cols_0_2d"] = lambda enc=enc: enc(u8(4, 0))
        c[k + ".too_many_pixels"] = lambda enc=enc, r=px_rows, q=px_cols: enc(huge(np.uint8, 1, r, q))
        c[k + ".dev.no_shape"] = lambda enc=enc: enc(dev(64))
        c[k + ".dev.no_shape_with_dtype"] = lambda enc=enc: enc(dev(64), dtype=np.uint8)
        c[k + ".dev.shape_rank_1"] = lambda enc=enc: enc(dev(64), shape=(4,))
        c[k + ".dev.shape_rank_4"] = lambda enc=enc: enc(dev(64), shape=(1, 1, 4, 4))
        c[k + ".dev.dtype_float"] = lambda enc=enc: enc(dev(64), shape=(4, 4), dtype=np.float32)
        c[k + ".dev.too_small"] = lambda enc=enc: enc(dev(31), shape=(4, 4))
        c[k + ".dev.too_small_u8"] = lambda enc=enc: enc(dev(31), shape=(2, 4, 4), dtype=np.uint8)
        c[k + ".dev.negative_n"] = lambda enc=enc: enc(dev(64), shape=(-1, 4, 4))
        c[k + ".dev.order.shape_then_fit"] = lambda enc=enc: enc(dev(0), shape=(1, 0, 4))
        c[k + ".dev.empty"] = lambda enc=enc: enc(dev(0), shape=(0, 4, 4))
        c[k + ".dev.order.empty_then_shape"] = lambda enc=enc: enc(dev(0), shape=(0, 0, 0), dtype=np.uint8)

    # jpeg_lossless_encode_batch: precision and restart intervals
    c["je.precision_float"] = lambda: je(u16(1, 4, 4), precision=12.0)
    c["je.precision_bool"] = lambda: je(u16(1, 4, 4), precision=True)
    c["je.restart_rows_float"] = lambda: je(u16(1, 4, 4), restart_rows=1.0)
    c["je.restart_rows_none"] = lambda: je(u16(1, 4, 4), restart_rows=None)
    c["je.precision_1"] = lambda: je(u16(1, 4, 4), precision=1)
    c["je.precision_17"] = lambda: je(u16(1, 4, 4), precision=17)
    c["je.precision_9_of_u8"] = lambda: je(u8(1, 4, 4), precision=9)
    c["je.dev.precision_9_of_u8"] = lambda: je(dev(64), shape=(4, 4), dtype=np.uint8, precision=9)
    c["je.restart_rows_neg"] = lambda: je(u16(1, 4, 4), restart_rows=-1)
    c["je.restart_interval_too_long"] = lambda: je(u16(1, 4, 4), restart_rows=20000)
    c["je.rows_65536"] = lambda: je(huge(np.uint8, 1, 65536, 1))
    c["je.cols_65536"] = lambda: je(huge(np.uint8, 1, 1, 65536))
    c["je.order.dtype_then_precision"] = lambda: je(f32(1, 4, 4), precision=1.0)
    c["je.order.precision_type_then_range"] = lambda: je(u16(1, 4, 4), precision=1, restart_rows=1.0)
    c["je.order.precision_then_restart"] = lambda: je(u16(1, 4, 4), precision=17, restart_rows=-1)
    c["je.order.precision_then_empty"] = lambda: je(u16(0, 4, 4), precision=17)
    c["je.order.restart_then_empty"] = lambda: je(u16(0, 4, 4), restart_rows=-2)
    c["je.order.shape_then_interval"] = lambda: je(u16(1, 0, 4), restart_rows=20000)
    c["je.order.interval_then_fit"] = lambda: je(dev(0), shape=(1, 4, 4), restart_rows=20000)
    c["je.order.empty_then_interval"] = lambda: je(u16(0, 4, 4), restart_rows=20000)

    # the two frame decoders
    for k, dec in (("rd", rd), ("jd", jd)):
        c[k + ".rows_float"] = lambda dec=dec: dec([b""], 4.0, 4)
        c[k + ".cols_bool"] = lambda dec=dec: dec([b""], 4, True)
        c[k + ".bits_str"] = lambda dec=dec: dec([b""], 4, 4, bits="16")
        c[k + ".bits_12"] = lambda dec=dec: dec([b""], 4, 4, bits=12)
        c[k + ".rows_0"] = lambda dec=dec: dec([b""], 0, 4)
        c[k + ".cols_neg"] = lambda dec=dec: dec([b""], 4, -4)
        c[k + ".too_many_pixels"] = lambda dec=dec: dec([b""], 8192, 8193)
        c[k + ".files_bytes"] = lambda dec=dec: dec(b"frame", 4, 4)
        c[k + ".files_str"] = lambda dec=dec: dec("frame", 4, 4)
        c[k + ".file_is_str"] = lambda dec=dec: dec(["frame"], 4, 4)
        c[k + ".file_is_int"] = lambda dec=dec: dec([b"", 3], 4, 4)
        c[k + ".out_dev_type"] = lambda dec=dec: dec([b""], 4, 4, out_dev=u16(16))
        c[k + ".order.type_then_bits"] = lambda dec=dec: dec([b""], 4.0, 4, bits=12)
        c[k + ".order.rows_type_then_cols_type"] = lambda dec=dec: dec([b""], 4.0, 4.0)
        c[k + ".order.bits_then_shape"] = lambda dec=dec: dec([b""], 0, 4, bits=12)
        c[k + ".order.shape_then_files"] = lambda dec=dec: dec(b"frame", 0, 4)
        c[k + ".order.files_then_out_dev"] = lambda dec=dec: dec(["frame"], 4, 4, out_dev="x")
        c[k + ".order.out_dev_type_then_empty"] = lambda dec=dec: dec([], 4, 4, out_dev="x")
        c[k + ".empty"] = lambda dec=dec: dec([], 4, 5)
        c[k + ".empty_8"] = lambda dec=dec: dec([], 4, 5, bits=8)
        c[k + ".empty_status"] = lambda dec=dec: dec([], 4, 5, bits=8, raise_errors=False)
        c[k + ".empty_dev"] = lambda dec=dec: dec([], 4, 5, out_dev=dev(0))
        c[k + ".empty_dev_status"] = lambda dec=dec: dec([], 4, 5, out_dev=dev(0), raise_errors=False)
        c[k + ".out_dev_too_small"] = lambda dec=dec: dec([b""], 4, 4, out_dev=dev(31))
        c[k + ".out_dev_too_small_8"] = lambda dec=dec: dec([b"", b""], 4, 4, bits=8, out_dev=dev(31))
    c["jd.rows_65536"] = lambda: jd([b""], 65536, 1)

    # dicom_encapsulate
    c["en.bytes"] = lambda: h.dicom_encapsulate(b"one frame, not a list")
    c["en.str"] = lambda: h.dicom_encapsulate("text")
    c["en.frame_is_str"] = lambda: h.dicom_encapsulate([b"ab", "cd"])
    c["en.frame_is_int"] = lambda: h.dicom_encapsulate([5])
    c["en.empty"] = lambda: h.dicom_encapsulate([]).hex()
    return c


def c_cases():
    """id -> call of a C entry point that returns before it touches the device"""
    from cct_hip import _ffi
    L = _ffi.lib()
    img = np.zeros((2, 4, 4), np.uint16)
    out = np.zeros((2, 8192), np.uint8)
    sizes, status = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    offs = np.array([0, 70, 140], np.uint64)
    down = np.array([0, 70, 60], np.uint64)
    blob = np.zeros(140, np.uint8)
    rows_o, cols_o, third_o = (np.zeros(1, np.int32) for _ in range(3))
    p = lambda a: a.ctypes.data  # noqa: E731
    keep = (img, out, sizes, status, offs, down, blob, rows_o, cols_o, third_o)

    def png16(n=2, rows=4, cols=4, shift=0, level=6, stride=8192, images=p(img)):
        return L.cct_png_encode_batch(images, 0, n, rows, cols, shift, level, p(out), stride, p(sizes))

    def png8(n=2, rows=4, cols=4, src_bits=16, lo=0, hi=100, level=6, stride=8192, images=p(img)):
        return L.cct_png_encode8_batch(images, 0, n, rows, cols, src_bits, lo, hi, level, p(out), stride, p(sizes))

    def pngr(n=2, rows=4, cols=4, shift=0, cap=32, files=p(blob), o=p(offs)):
        return L.cct_png_read_batch(files, o, n, rows, cols, shift, p(img), 0, cap, p(status))

    def info(fn, data, r=True):
        as_int = lambda a: a.ctypes.data_as(_ffi.C.POINTER(_ffi.C.c_int))  # noqa: E731
        return fn(data, len(data) if data is not None else 0, as_int(rows_o) if r else None, as_int(cols_o), as_int(third_o))

    def zlevel(level):
        return L.cct_zlib_compress_batch_level(p(blob), p(offs), 2, level, p(out), 8192, p(sizes))

    def zparams(n=2, level=9, strategy=0, mem_level=8):
        return L.cct_zlib_compress_batch_params(p(blob), p(offs), n, level, strategy, mem_level, p(out), 8192, p(sizes))

    def unz(n=2, stride=4096):
        return L.cct_zlib_decompress_batch(p(blob), p(offs), n, p(out), stride, p(sizes), p(status))

    def rle_e(n=2, rows=4, cols=4, bits=16, stride=8192, images=p(img)):
        return L.cct_dicom_rle_encode_batch(images, 0, n, rows, cols, bits, p(out), stride, p(sizes))

    def rle_d(n=2, rows=4, cols=4, bits=16, cap=32, o=p(offs), frames=p(blob)):
        return L.cct_dicom_rle_decode_batch(frames, o, n, rows, cols, bits, p(img), 0, cap, p(status))

    def jpl_e(n=2, rows=4, cols=4, src_bits=16, precision=16, rr=0, stride=8192, st=p(status)):
        return L.cct_jpegll_encode_batch(p(img), 0, n, rows, cols, src_bits, precision, rr, p(out), stride, p(sizes), st)

    def jpl_d(n=2, rows=4, cols=4, bits=16, cap=32, o=p(offs), files=p(blob)):
        return L.cct_jpegll_decode_batch(files, o, n, rows, cols, bits, p(img), 0, cap, p(status))

    c = {"_keep": keep}
    c["png16.level_0"] = lambda: png16(level=0)
    c["png16.level_10"] = lambda: png16(level=10)
    c["png16.shift_16"] = lambda: png16(shift=16)
    c["png16.rows_0"] = lambda: png16(rows=0)
    c["png16.too_many_filtered_bytes"] = lambda: png16(rows=40000, cols=40000)
    c["png16.negative_n"] = lambda: png16(n=-1)
    c["png16.no_images"] = lambda: png16(images=None)
    c["png16.stride"] = lambda: png16(stride=L.cct_png_bound(4, 4) - 1)
    c["png16.order.level_then_shift"] = lambda: png16(level=3, shift=16)
    c["png16.order.shape_then_n"] = lambda: png16(rows=0, n=-1)
    c["png8.level_3"] = lambda: png8(level=3)
    c["png8.level_neg"] = lambda: png8(level=-2)
    c["png8.src_bits_12"] = lambda: png8(src_bits=12)
    c["png8.window"] = lambda: png8(lo=5, hi=5)
    c["png8.window_of_u8"] = lambda: png8(src_bits=8, lo=0, hi=100)
    c["png8.cols_0"] = lambda: png8(cols=0)
    c["png8.too_many_filtered_bytes"] = lambda: png8(rows=40000, cols=40000)
    c["png8.negative_n"] = lambda: png8(n=-1)
    c["png8.no_images"] = lambda: png8(images=None)
    c["png8.stride"] = lambda: png8(stride=64)
    c["png8.stride_beyond_the_16_bit_bound"] = lambda: png8(rows=20000, cols=40000, stride=64)
    c["pngr.negative_n"] = lambda: pngr(n=-1)
    c["pngr.shift"] = lambda: pngr(shift=-1)
    c["pngr.rows_0"] = lambda: pngr(rows=0)
    c["pngr.too_many_filtered_bytes"] = lambda: pngr(rows=40000, cols=40000)
    c["pngr.null"] = lambda: pngr(files=None)
    c["pngr.cap"] = lambda: pngr(cap=31)
    c["pngr.empty"] = lambda: pngr(n=0)
    c["png_info.null"] = lambda: info(L.cct_png_info, b"x" * 40, r=False)
    c["png_info.junk"] = lambda: info(L.cct_png_info, b"x" * 40)
    c["zlevel.2"] = lambda: zlevel(2)
    c["zlevel.10"] = lambda: zlevel(10)
    c["zparams.mem_level"] = lambda: zparams(mem_level=7)
    c["zparams.strategy"] = lambda: zparams(strategy=5)
    c["zparams.level_0"] = lambda: zparams(level=0)
    c["zparams.level_11"] = lambda: zparams(level=11)
    c["zparams.level_2_default_strategy"] = lambda: zparams(level=2)
    c["zparams.negative_n"] = lambda: zparams(n=-1)
    c["unz.negative_n"] = lambda: unz(n=-1)
    c["unz.stride_0"] = lambda: unz(stride=0)
    c["unz.stride_odd"] = lambda: unz(stride=100)
    c["rle_e.bits_12"] = lambda: rle_e(bits=12)
    c["rle_e.rows_0"] = lambda: rle_e(rows=0)
    c["rle_e.too_many_pixels"] = lambda: rle_e(rows=8192, cols=8193)
    c["rle_e.negative_n"] = lambda: rle_e(n=-1)
    c["rle_e.stride"] = lambda: rle_e(stride=L.cct_dicom_rle_bound(4, 4, 16) - 1)
    c["rle_e.null"] = lambda: rle_e(images=None)
    c["rle_e.empty"] = lambda: rle_e(n=0)
    c["rle_e.order.bits_then_shape"] = lambda: rle_e(bits=12, rows=0)
    c["rle_d.bits_24"] = lambda: rle_d(bits=24)
    c["rle_d.cols_0"] = lambda: rle_d(cols=0)
    c["rle_d.negative_n"] = lambda: rle_d(n=-1)
    c["rle_d.cap"] = lambda: rle_d(cap=31)
    c["rle_d.cap_8"] = lambda: rle_d(bits=8, cap=0)
    c["rle_d.null"] = lambda: rle_d(frames=None)
    c["rle_d.offsets_decrease"] = lambda: rle_d(o=p(down))
    c["rle_d.empty"] = lambda: rle_d(n=0)
    c["rle_d.order.cap_then_null"] = lambda: rle_d(cap=31, frames=None)
    c["jpl_e.rows_0"] = lambda: jpl_e(rows=0)
    c["jpl_e.cols_65536"] = lambda: jpl_e(rows=1, cols=65536)
    c["jpl_e.negative_n"] = lambda: jpl_e(n=-1)
    c["jpl_e.src_bits_12"] = lambda: jpl_e(src_bits=12)
    c["jpl_e.precision_1"] = lambda: jpl_e(precision=1)
    c["jpl_e.precision_9_of_8"] = lambda: jpl_e(src_bits=8, precision=9)
    c["jpl_e.restart_neg"] = lambda: jpl_e(rr=-1)
    c["jpl_e.restart_interval_too_long"] = lambda: jpl_e(rr=20000)
    c["jpl_e.stride"] = lambda: jpl_e(stride=L.cct_jpegll_bound(4, 4, 0) - 1)
    c["jpl_e.null"] = lambda: jpl_e(st=None)
    c["jpl_e.empty"] = lambda: jpl_e(n=0)
    c["jpl_d.rows_0"] = lambda: jpl_d(rows=0)
    c["jpl_d.negative_n"] = lambda: jpl_d(n=-1)
    c["jpl_d.bits_12"] = lambda: jpl_d(bits=12)
    c["jpl_d.cap"] = lambda: jpl_d(cap=31)
    c["jpl_d.null"] = lambda: jpl_d(files=None)
    c["jpl_d.offsets_decrease"] = lambda: jpl_d(o=p(down))
    c["jpl_d.every_file_refused"] = lambda: jpl_d()
    c["jpl_d.empty"] = lambda: jpl_d(n=0)
    c["jpl_info.null"] = lambda: info(L.cct_jpegll_info, b"x" * 40, r=False)
    c["jpl_info.junk"] = lambda: info(L.cct_jpegll_info, b"x" * 40)
    c["decode.negative_n"] = lambda: L.cct_decode_batch(p(blob), p(offs), -1, 8, b"abcd", p(img), 0, 32, p(status))
    c["decode.empty"] = lambda: L.cct_decode_batch(p(blob), p(offs), 0, 8, b"abcd", p(img), 0, 32, p(status))
    return c


def describe(x):
    """a result as JSON keeps it: shapes and dtypes of arrays, tuples and lists told apart"""
    if isinstance(x, np.ndarray):
        return {"array": list(x.shape), "dtype": str(x.dtype)}
    if isinstance(x, tuple):
        return {"tuple": [describe(v) for v in x]}
    if isinstance(x, list):
        return {"list": [describe(v) for v in x]}
    assert isinstance(x, (int, str)), type(x)
    return x


def run_python(call):
    try:
        return {"returns": describe(call())}
    except Exception as e:  # noqa: BLE001 - the type is what is recorded
        return {"raises": [type(e).__name__, str(e)]}


def run_c(call):
    from cct_hip import _ffi
    rc = call()
    return [rc, _ffi.last_error() if rc else ""]


def record():
    """what tests/golden/batch_refusals.json holds (tools/gen_batch_refusals.py writes it)"""
    c = c_cases()
    return {"python": {k: run_python(f) for k, f in python_cases().items()},
            "c": {k: run_c(f) for k, f in c.items() if k != "_keep"}}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_python_refusals_and_empty_batches(golden):
    cases = python_cases()
    assert sorted(cases) == sorted(golden["python"])
    wrong = {k: (got, golden["python"][k]) for k, got in ((k, run_python(f)) for k, f in cases.items()) if got != golden["python"][k]}
    assert not wrong, wrong


def test_two_faults_fix_the_order(golden):
    """the example the order cases are modelled on, spelled out: a rank-1 float32 array"""
    g = golden["python"]
    assert g["pe.order.dtype_then_rank"]["raises"][0] == "TypeError"
    for k in ("p8", "re", "je"):
        assert g[k + ".order.rank_then_dtype"]["raises"][0] == "ValueError"
    assert sum(".order." in k for k in g) >= 40


def test_no_case_reaches_the_device(golden):
    """every recorded answer is a refusal written in batch.py or the C argument checks, or an empty batch"""
    for k, v in golden["python"].items():
        if "raises" in v:
            assert v["raises"][0] in ("TypeError", "ValueError"), k  # a device call without a device raises DeviceError
    from cct_hip import _ffi
    for k, (rc, msg) in golden["c"].items():
        assert rc != _ffi.E_DEVICE and rc != _ffi.E_NOMEM, k
        assert (rc == 0) == (msg == ""), k


def test_c_whole_call_refusals(golden):
    cases = c_cases()
    assert sorted(k for k in cases if k != "_keep") == sorted(golden["c"])
    wrong = {k: (got, golden["c"][k]) for k, got in ((k, run_c(f)) for k, f in cases.items() if k != "_keep") if got != golden["c"][k]}
    assert not wrong, wrong
