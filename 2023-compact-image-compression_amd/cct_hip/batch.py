"""Batch API over the C ABI: a per-slice Python call cannot feed a TB/s device, so callers
with many slices (scripts/evaluate.py's corpus loop, bench.py) hand whole batches over.
Single-slice use goes through codec.core.Encoder / Decoder, which call into here with n=1.
"""
import ctypes as C
import json
import os

import numpy as np

from . import _ffi

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def default_config():
    """The reference's src/config.json, shipped verbatim as data next to the package."""
    with open(os.path.join(_PKG_ROOT, "config.json")) as f:
        return json.load(f)


def magic_bytes(config):
    """4 header bytes of config['magic'] (core.py:188-196: big-endian write of the low 32 bits)."""
    b = bytes(map(ord, config["magic"]))
    return b[-4:].rjust(4, b"\0")


Z_HUFFMAN_ONLY, Z_RLE = 2, 3  # zlib strategies that run deflate_huff / deflate_rle, which read no level table


def _is_int(x):
    """an integer that is not a bool"""
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _ints(**named):
    """the named arguments as a list of ints; TypeError for the first that is not an integer"""
    for name, x in named.items():
        if not _is_int(x):
            raise TypeError(f"{name} must be an integer, got {x!r}")
    return [int(x) for x in named.values()]


def _check_strategy(strategy):
    """zlib strategy 0 .. 4 (Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED) or ValueError"""
    if not _is_int(strategy):
        raise ValueError(f"deflate strategy must be an integer (zlib's Z_* constants), got {strategy!r}")
    strategy = int(strategy)
    if not 0 <= strategy <= 4:
        raise ValueError(f"deflate strategy {strategy}: zlib strategies are 0 to 4 (Z_DEFAULT_STRATEGY to Z_FIXED)")
    return strategy


def _check_level(level, strategy):
    """zlib level of (level, strategy) on the device: -1 -> 6; 4 .. 9; also 1 .. 3 under Z_HUFFMAN_ONLY / Z_RLE"""
    if not _is_int(level):
        raise ValueError(f"deflate_level must be an integer, got {level!r}")
    level = int(level)
    if level == -1:
        return 6
    if strategy in (Z_HUFFMAN_ONLY, Z_RLE):
        if not 1 <= level <= 9:
            raise ValueError(f"deflate level {level} with strategy {strategy}: supported levels are -1 and 1 to 9 "
                             "(0 is deflate_stored, not on the device)")
    elif not 4 <= level <= 9:
        raise ValueError(f"deflate level {level} with strategy {strategy}: supported levels are -1 and 4 to 9 "
                         "(0 to 3 are deflate_stored / deflate_fast, not on the device)")
    return level


def deflate_strategy(config):
    """config['encoder']['deflate_strategy'] -> zlib strategy of the DEFLATE stage, zlib's integer constants: absent -> 0
    (Z_DEFAULT_STRATEGY, what the reference writes), 1 Z_FILTERED, 2 Z_HUFFMAN_ONLY, 3 Z_RLE, 4 Z_FIXED.  Anything else
    (bool, str and float included): ValueError."""
    strategy = config["encoder"].get("deflate_strategy")
    return 0 if strategy is None else _check_strategy(strategy)


def deflate_level(config):
    """config['encoder']['deflate_level'] -> zlib level of the DEFLATE stage: absent -> 9 (what the reference writes),
    -1 -> 6 (Z_DEFAULT_COMPRESSION), 4 .. 9 as given.  Levels 0 to 3 run deflate_stored / deflate_fast, which the
    device does not implement: ValueError, as for anything else -- except levels 1 to 3 under deflate_strategy 2 or 3
    (deflate_huff / deflate_rle ignore the level)."""
    strategy = deflate_strategy(config)
    level = config["encoder"].get("deflate_level")
    if level is None:
        return 9
    return _check_level(level, strategy)


def codec_params(config, dtype=None):
    """config dict -> (flags, block_size, eof, magic, channels, bytes_per_channel).  An optional
    config['encoder']['deflate_level'] sets the CCT_FLAG_DEFLATE_LEVEL field (absent: field 0 = level 9), an optional
    config['encoder']['deflate_strategy'] the CCT_FLAG_DEFLATE_STRATEGY field (absent: field 0 = Z_DEFAULT_STRATEGY)."""
    enc = config["encoder"]
    tr = enc["transforms"]
    flags = 0
    if tr["fractal"]:
        flags |= _ffi.FLAG_FRACTAL
    if tr["segmentation"]:
        flags |= _ffi.FLAG_SEGMENTATION
    if enc["deflate_compression"]:
        flags |= _ffi.FLAG_DEFLATE
    if dtype is not None and np.dtype(dtype).kind == "i":
        flags |= _ffi.FLAG_SIGNED_SEG
    if enc.get("deflate_level") is not None:
        flags |= _ffi.flag_deflate_level(deflate_level(config))
    if enc.get("deflate_strategy") is not None:
        flags |= _ffi.flag_deflate_strategy(deflate_strategy(config))
    eof = enc.get("end_of_file")
    return (flags, int(config["block_size"]), -1 if eof is None else int(eof) % 256, magic_bytes(config),
            int(enc["channels"]), int(enc["bytes_per_channel"]))


def device_info():
    L = _ffi.lib()
    name = C.create_string_buffer(256)
    cus = C.c_int(0)
    hbm = C.c_uint64(0)
    _ffi.check(L.cct_device_info(name, 256, C.byref(cus), C.byref(hbm)))
    return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}


class DeviceBuffer:
    """Plain HBM allocation owned by the library's device (hipMalloc behind cct_dev_alloc)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p(0)
        _ffi.check(_ffi.lib().cct_dev_alloc(C.byref(p), self.nbytes))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, arr):
        arr = np.ascontiguousarray(arr)
        buf = cls(arr.nbytes)
        buf.upload(arr)
        return buf

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        _ffi.check(_ffi.lib().cct_h2d(self.ptr + offset, arr.ctypes.data, arr.nbytes))

    def download(self, dtype, count, offset=0):
        out = np.empty(count, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes
        _ffi.check(_ffi.lib().cct_d2h(out.ctypes.data, self.ptr + offset, out.nbytes))
        return out

    def zero(self):
        _ffi.check(_ffi.lib().cct_dev_memset(self.ptr, 0, self.nbytes))

    def free(self):
        if self.ptr:
            _ffi.check(_ffi.lib().cct_dev_free(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                _ffi.lib().cct_dev_free(self.ptr)
                self.ptr = None
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class PinnedArray:
    """Page-locked host bytes (cct_host_alloc) seen as a numpy uint8 array: archives kept here move to and from
    the device without a staging copy."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p(0)
        _ffi.check(_ffi.lib().cct_host_alloc(C.byref(p), self.nbytes))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr))

    def free(self):
        if self.ptr:
            self.array = None
            _ffi.check(_ffi.lib().cct_host_free(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                _ffi.lib().cct_host_free(self.ptr)
                self.ptr = None
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class Event:
    """HIP event on the library's stream (bench.py times kernels with these)."""

    def __init__(self):
        p = C.c_void_p(0)
        _ffi.check(_ffi.lib().cct_event_create(C.byref(p)))
        self.ptr = p.value

    def record(self):
        _ffi.check(_ffi.lib().cct_event_record(self.ptr))

    def elapsed_ms_since(self, start):
        ms = C.c_float(0)
        _ffi.check(_ffi.lib().cct_event_elapsed_ms(start.ptr, self.ptr, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                _ffi.lib().cct_event_destroy(self.ptr)
        except Exception:  # noqa: BLE001
            pass


def payload_stride(width, height, block_size):
    return _ffi.lib().cct_payload_stride(width, height, block_size)


def encode_payload_dev(d_images, n, width, height, config_or_params, d_payload, d_sizes, d_status,
                       d_stats=None, d_roles=None, dtype=np.uint16):
    """Stage (i) on device-resident slices; all arguments are DeviceBuffer objects."""
    params = codec_params(config_or_params, dtype) if isinstance(config_or_params, dict) else config_or_params
    flags, bs, eof = params[0], params[1], params[2]
    stride = payload_stride(width, height, bs)
    _ffi.check(_ffi.lib().cct_encode_payload_dev(
        d_images.ptr, n, width, height, bs, flags, eof, d_payload.ptr, stride, d_sizes.ptr, d_status.ptr,
        d_stats.ptr if d_stats is not None else None, d_roles.ptr if d_roles is not None else None))
    return stride


def decode_payload_dev(d_payload, stride, d_sizes, n, width, height, block_size, fractal, d_images, d_status):
    _ffi.check(_ffi.lib().cct_decode_payload_dev(d_payload.ptr, stride, d_sizes.ptr, n, width, height, block_size,
                                                  int(bool(fractal)), d_images.ptr, d_status.ptr))


def partition_roles(image, config=None):
    """Block roles of one slice (the partition of cluster.py:49-199 as the device computes it): uint8[NB], 0 = emitted
    alone, 1..63 = leader of a meshed pair (BLOCK_JUMPS[b] - b), 0xFF = partner."""
    config = config or default_config()
    image = np.ascontiguousarray(image)
    w, h = image.shape
    bs = int(config["block_size"])
    nb = w * h // bs
    d_img = DeviceBuffer.from_numpy(image)
    d_pay, d_sz, d_st, d_roles = DeviceBuffer(payload_stride(w, h, bs)), DeviceBuffer(4), DeviceBuffer(4), DeviceBuffer(max(nb, 1))
    encode_payload_dev(d_img, 1, w, h, codec_params(config, image.dtype), d_pay, d_sz, d_st, None, d_roles)
    return d_roles.download(np.uint8, nb)


# ---- what the batch entry points below share: how they read their arguments and hand buffers to the C ABI --------------

def _raster_batch(images, shape, dtype, fn, noun, dtype_words=""):
    """(source, (n, rows, cols), dtype) of an encoder's rasters: an array of shape (n, rows, cols) or (rows, cols), or a
    DeviceBuffer that shape= (and dtype=, np.uint16 if absent; required where dtype_words names the choice) describe.
    fn and noun ("PNG", "frame") are the caller's words in the messages."""
    if isinstance(images, DeviceBuffer):
        if shape is None or (dtype_words and dtype is None):
            raise ValueError(f"{fn} of a DeviceBuffer needs shape=(n, rows, cols) or (rows, cols)"
                             + (f" and dtype={dtype_words}" if dtype_words else ""))
        dt = np.dtype(np.uint16 if dtype is None else dtype)
        shape = tuple(int(x) for x in shape)
        if len(shape) == 2:
            shape = (1,) + shape
        if len(shape) != 3:
            raise ValueError(f"{noun} batch shape {shape}: (n, rows, cols) or (rows, cols)")
        return images, shape, dt
    if shape is not None or dtype is not None:
        raise ValueError("shape= and dtype= describe a DeviceBuffer; an array carries its own")
    arr = np.asarray(images)
    if arr.ndim == 2:
        arr = arr[None]
    if arr.ndim != 3:
        raise ValueError(f"{noun} batch of shape {arr.shape}: (n, rows, cols) or (rows, cols) expected")
    return arr, arr.shape, arr.dtype


def _raster_ptr(src, shape, dt, what):
    """(ptr, on_device, keep) of a checked _raster_batch: a DeviceBuffer must hold the batch (`what` names it in the
    message), an array is made contiguous; keep is what has to outlive the C call."""
    if isinstance(src, DeviceBuffer):
        n, rows, cols = shape
        if n < 0 or n * rows * cols * dt.itemsize > src.nbytes:
            raise ValueError(f"{what} does not fit the {src.nbytes}-byte DeviceBuffer")
        return src.ptr, 1, src
    arr = np.ascontiguousarray(src)
    return arr.ctypes.data, 0, arr


def _file_list(files, fn, per, what):
    """files as a list of bytes objects, or TypeError: "<fn> takes a list .. one per <per>", "<what> is a bytes object" """
    if isinstance(files, (bytes, bytearray, memoryview, str)):
        raise TypeError(f"{fn} takes a list of bytes objects, one per {per}")
    files = list(files)
    for f in files:
        if not isinstance(f, (bytes, bytearray, memoryview)):
            raise TypeError(f"{what} is a bytes object, got {type(f).__name__}")
    return files


def _archive(files):
    """(blob, offs): the files back to back (one byte where there is none: the C side wants an address) and the n + 1
    offsets of an archive argument"""
    offs = np.zeros(len(files) + 1, dtype=np.uint64)
    np.cumsum([len(f) for f in files], out=offs[1:])
    return b"".join(files) or b"\0", offs


def _files_out(n, out_stride):
    """(out, sizes) for an encoder that writes file i at out[i] and its length to sizes[i]"""
    return np.empty((n, out_stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32)


def _files_of(out, sizes):
    return [out[i, : sizes[i]].tobytes() for i in range(len(sizes))]


def _check_out_dev(out_dev):
    if out_dev is not None and not isinstance(out_dev, DeviceBuffer):
        raise TypeError(f"out_dev must be a DeviceBuffer, got {type(out_dev).__name__}")


def _no_rasters(shape, dt, out_dev, raise_errors):
    """what a raster decoder returns for an empty batch"""
    res = shape if out_dev is not None else np.zeros(shape, dtype=dt)
    return res if raise_errors else (res, np.zeros(0, dtype=np.uint32))


def _decode_rasters(call, n, rows, cols, dt, out_dev, raise_errors, per_file_codes):
    """Run call(images, images_on_device, images_cap_px, status) -> rc into a fresh (n, rows, cols) array or into out_dev.
    Returns the array (the shape with out_dev); with raise_errors=False, (that, status), and the per-file codes pass."""
    if out_dev is not None and n * rows * cols * dt.itemsize > out_dev.nbytes:
        raise ValueError(f"{n} rasters of {rows} x {cols} do not fit the {out_dev.nbytes}-byte DeviceBuffer")
    status = np.zeros(n, dtype=np.uint32)
    if out_dev is not None:
        res = (n, rows, cols)
        rc = call(out_dev.ptr, 1, out_dev.nbytes // dt.itemsize, status.ctypes.data)
    else:
        res = np.empty((n, rows, cols), dtype=dt)
        rc = call(res.ctypes.data, 0, res.size, status.ctypes.data)
    if raise_errors or rc not in per_file_codes:
        _ffi.check(rc)
    return res if raise_errors else (res, status)


def encode_batch(images, config=None, return_info=False):
    """images: (n, W, H) array of a 2-byte dtype (or a DeviceBuffer + shape via encode_batch_dev).
    Returns a list of n `bytes`, each exactly what Encoder(config, images[i]).encode() returns."""
    config = config or default_config()
    images = np.asarray(images)
    if images.ndim != 3:
        raise ValueError("encode_batch expects an array of shape (n, width, height)")
    if images.dtype.itemsize != 2:
        raise TypeError(f"2-byte pixels required (uint16/int16), got {images.dtype}")
    images = np.ascontiguousarray(images)
    n, w, h = images.shape
    return _encode(images.ctypes.data, 0, n, w, h, config, images.dtype, return_info, keep=images)


def encode_batch_dev(d_images, n, width, height, config=None, dtype=np.uint16, return_info=False):
    """Same as encode_batch for slices already resident in HBM (DeviceBuffer)."""
    return _encode(d_images.ptr, 1, n, width, height, config or default_config(), dtype, return_info)


def _encode(ptr, on_device, n, w, h, config, dtype, return_info, keep=None):
    L = _ffi.lib()
    flags, bs, eof, magic, ch, bpc = codec_params(config, dtype)
    if (w * h) % bs != 0:  # numpy's reshape message, core.py:245
        raise ValueError(f"cannot reshape array of size {w * h} into shape ({(w * h) // bs},{bs})")
    defl = bool(flags & _ffi.FLAG_DEFLATE)
    out_stride = L.cct_file_bound(w, h, bs) if defl else 13 + L.cct_payload_stride(w, h, bs)
    out = np.empty((max(n, 1), out_stride), dtype=np.uint8)
    sizes = np.zeros(max(n, 1), dtype=np.uint32)
    status = np.zeros(max(n, 1), dtype=np.uint32)
    psizes = np.zeros(max(n, 1), dtype=np.uint32)
    stats = (_ffi.SliceStats * max(n, 1))()
    dev_defl = C.c_int(0)
    L.cct_get_option(b"device_deflate", C.byref(dev_defl))
    if defl and dev_defl.value and n > 0:
        # archive layout: the files come back to back (one compact copy instead of n * out_stride strided bytes)
        arch = out.reshape(-1)
        offs = np.zeros(n + 1, dtype=np.uint64)
        _ffi.check(L.cct_encode_batch_packed(ptr, on_device, n, w, h, bs, flags, eof, magic, ch, bpc,
                                             arch.ctypes.data, arch.size, offs.ctypes.data, sizes.ctypes.data,
                                             status.ctypes.data, psizes.ctypes.data, C.cast(stats, C.c_void_p)))
        files = [arch[int(offs[i]): int(offs[i + 1])].tobytes() for i in range(n)]
    else:
        _ffi.check(L.cct_encode_batch(ptr, on_device, n, w, h, bs, flags, eof, magic, ch, bpc,
                                      out.ctypes.data, out_stride, sizes.ctypes.data, status.ctypes.data,
                                      psizes.ctypes.data, C.cast(stats, C.c_void_p)))
        files = _files_of(out, sizes[:n])
    if return_info:
        info = [{"payload_len": int(psizes[i]), "n_short": stats[i].n_short, "n_full": stats[i].n_full,
                 "n_jump": stats[i].n_jump, "n_difficult": stats[i].n_difficult,
                 "q7": bool(status[i] & _ffi.ST_Q7)} for i in range(n)]
        return files, info
    return files


def decode_batch(files, config=None, out_dev=None):
    """files: list of .cct byte strings of identical shape/flags.
    Returns an (n, W, H) uint16 array (or fills the DeviceBuffer `out_dev` and returns the shape)."""
    config = config or default_config()
    L = _ffi.lib()
    n = len(files)
    magic = magic_bytes(config)
    bs = int(config["block_size"])
    if n == 0:
        return np.zeros((0, 0, 0), dtype=np.uint16)
    hdr = _ffi.Header()
    _ffi.check(L.cct_read_header(files[0], len(files[0]), magic, C.byref(hdr)))
    w, h = hdr.width, hdr.height
    if (w * h) % bs != 0 or w * h == 0:  # core.py:429
        raise ValueError(f"cannot reshape array of size {w * h} into shape ({(w * h) // bs},{bs})")
    blob, offs = _archive(files)
    status = np.zeros(n, dtype=np.uint32)
    if out_dev is not None:
        rc = L.cct_decode_batch(blob, offs.ctypes.data, n, bs, magic, out_dev.ptr, 1, out_dev.nbytes // 2,
                                status.ctypes.data)
        _ffi.check(rc)
        return (n, w, h)
    out = np.empty((n, w, h), dtype=np.uint16)
    rc = L.cct_decode_batch(blob, offs.ctypes.data, n, bs, magic, out.ctypes.data, 0, out.size, status.ctypes.data)
    _ffi.check(rc)
    return out


def _check_mem_level(mem_level):
    """zlib memLevel on the device: 8 (zlib's default) or 9 (Pillow's PNG writer), or ValueError"""
    if not _is_int(mem_level) or int(mem_level) not in (8, 9):
        raise ValueError(f"zlib mem_level {mem_level!r}: the device runs memLevel 8 and 9")
    return int(mem_level)


def zlib_compress_batch(blobs, level=9, strategy=0, mem_level=8):
    """DEFLATE stage alone on the device: [bytes] -> [zlib streams], each byte-identical to
    zlib.compress(blob, level) -- level 9 by default (what the reference calls at core.py:340), 4 to 8, or
    -1 for zlib's default 6.  Levels 0 to 3 are not on the device (ValueError).  strategy (zlib's Z_* constant, 0 to 4)
    and mem_level (8 or 9): the stream of zlib.compressobj(level, zlib.DEFLATED, 15, mem_level, strategy);
    Z_HUFFMAN_ONLY (2) and Z_RLE (3) also take levels 1 to 3."""
    strategy = _check_strategy(strategy)
    level = _check_level(int(level), strategy)
    mem_level = _check_mem_level(mem_level)
    L = _ffi.lib()
    n = len(blobs)
    if n == 0:
        return []
    data, offs = _archive(blobs)
    longest = max(len(b) for b in blobs)
    in_stride = (longest + 16 + 255) & ~255
    # compressBound at memLevel 8, deflateBound's general bound at 9 (deflate_workspace.h zlib_bound), + slack
    if mem_level == 8:
        bound = in_stride + (in_stride >> 12) + (in_stride >> 14) + (in_stride >> 25) + 13
    else:
        bound = in_stride + ((in_stride + 7) >> 3) + ((in_stride + 63) >> 6) + 11
    out_stride = (bound + 11 + 128 + 63) & ~63
    out, sizes = _files_out(n, out_stride)
    _ffi.check(L.cct_zlib_compress_batch_params(data, offs.ctypes.data, n, level, strategy, mem_level, out.ctypes.data,
                                                out_stride, sizes.ctypes.data))
    return _files_of(out, sizes)


def _png_level(level):
    if not _is_int(level):
        raise TypeError(f"PNG compress_level must be an integer, got {level!r}")
    level = 6 if int(level) == -1 else int(level)
    if not 4 <= level <= 9:
        raise ValueError(f"PNG compress_level {level}: supported levels are -1 and 4 to 9 "
                         "(0 to 3 are deflate_stored / deflate_fast, not on the device)")
    return level


def _png_shift(shift):
    if not _is_int(shift):
        raise TypeError(f"PNG sample shift must be an integer, got {shift!r}")
    if not 0 <= int(shift) <= 15:
        raise ValueError(f"PNG sample shift {int(shift)}: 0 to 15")
    return int(shift)


def _check_png_shape(rows, cols):
    if rows < 1 or cols < 1:
        raise ValueError(f"PNG of {rows} x {cols} samples: rows and cols must be >= 1")
    if rows * (1 + 2 * cols) > (1 << 30) - 512:
        raise ValueError(f"PNG of {rows} x {cols} samples: more filtered bytes than one device DEFLATE pass takes")


def _png_args(images, level, shift, shape):
    """Validated (ptr, on_device, n, rows, cols, level, shift, keep) of png_encode_batch; raises before any device call."""
    level, shift = _png_level(level), _png_shift(shift)
    on_host = not isinstance(images, DeviceBuffer)
    if on_host:
        shape = None  # an array carries its own; this writer has always let a shape= beside it pass
        if np.asarray(images).dtype != np.uint16:  # this writer names the dtype before the rank, the others the rank first
            raise TypeError(f"16-bit PNGs take uint16 samples, got {np.asarray(images).dtype}")
    src, shape, dt = _raster_batch(images, shape, None, "png_encode_batch", "PNG")
    n, rows, cols = shape
    if on_host:
        _check_png_shape(rows, cols)  # before the copy below
    ptr, on_device, keep = _raster_ptr(src, shape, dt, f"PNG batch shape {shape}")
    _check_png_shape(rows, cols)
    return ptr, on_device, n, rows, cols, level, shift, keep


def png_encode_batch(images, level=6, shift=0, shape=None):
    """16-bit grayscale PNGs on the device: a uint16 array of shape (n, rows, cols) or (rows, cols), or a DeviceBuffer
    with shape= given, -> a list of n `bytes`.  File i is byte-identical to what Pillow writes for
    Image.fromarray(((img.astype(uint32) << shift) & 0xFFFF).astype(uint16)).save(f, "PNG", compress_level=level):
    level -1 (= 6, Pillow's default) or 4 to 9.  The row filters are chosen and applied on the device, the zlib stream
    is the device DEFLATE at memLevel 9 / Z_FILTERED (host libz under the device_deflate 0 option), and the chunks and
    CRC-32s are written on the device.  Arguments are checked (TypeError / ValueError) before any device call."""
    ptr, on_device, n, rows, cols, level, shift, keep = _png_args(images, level, shift, shape)
    if n == 0:
        return []
    L = _ffi.lib()
    out_stride = L.cct_png_bound(rows, cols)
    out, sizes = _files_out(n, out_stride)
    _ffi.check(L.cct_png_encode_batch(ptr, on_device, n, rows, cols, shift, level, out.ctypes.data, out_stride,
                                      sizes.ctypes.data))
    del keep
    return _files_of(out, sizes)


def decode_png_batch(files, config=None, level=9):
    """The 16-bit previews of .cct files, the batch form of Decoder(config, bytes, out_path).decode() as the reference
    writes them (imageio -> Pillow at compress_level 9, value << 4: core.py:522-538): files are decoded into HBM and
    turned into PNGs there, without the rasters coming back to the host.  Returns a list of PNG `bytes`."""
    config = config or default_config()
    if not _is_int(level):
        raise TypeError(f"PNG compress_level must be an integer, got {level!r}")
    if not (int(level) == -1 or 4 <= int(level) <= 9):
        raise ValueError(f"PNG compress_level {level}: supported levels are -1 and 4 to 9")
    if not files:
        return []
    n, w, h, d_img = _decode_to_device(files, config)
    return png_encode_batch(d_img, level=level, shift=4, shape=(n, w, h))


def _decode_to_device(files, config):
    """(n, w, h, DeviceBuffer) of .cct files decoded into HBM"""
    hdr = _ffi.Header()
    _ffi.check(_ffi.lib().cct_read_header(files[0], len(files[0]), magic_bytes(config), C.byref(hdr)))
    d_img = DeviceBuffer(max(2 * len(files) * hdr.width * hdr.height, 2))
    return decode_batch(files, config, out_dev=d_img) + (d_img,)


def _png_window(window):
    """(lo, hi) of a window argument, 0 <= lo < hi <= 65535, or TypeError / ValueError"""
    if isinstance(window, (str, bytes)) or not hasattr(window, "__len__") or len(window) != 2:
        raise TypeError(f"PNG window must be a pair (lo, hi), got {window!r}")
    if not all(_is_int(x) for x in window):
        raise TypeError(f"PNG window bounds must be integers, got {window!r}")
    lo, hi = int(window[0]), int(window[1])
    if not 0 <= lo < hi <= 65535:
        raise ValueError(f"PNG window ({lo}, {hi}): 0 <= lo < hi <= 65535")
    return lo, hi


def _png8_args(images, window, level, shape, dtype):
    """Validated (ptr, on_device, n, rows, cols, src_bits, lo, hi, level, keep) of png8_encode_batch; raises before any
    device call."""
    level = _png_level(level)
    if isinstance(images, DeviceBuffer) and shape is not None and dtype is not None:
        try:  # this writer answers for a dtype numpy does not know in its own words
            np.dtype(dtype)
        except TypeError:
            raise TypeError(f"8-bit PNGs take uint8 or uint16 samples, got dtype {dtype!r}") from None
    src, shape, dt = _raster_batch(images, shape, dtype, "png8_encode_batch", "PNG", "np.uint8 or np.uint16")
    n, rows, cols = shape
    if dt == np.uint8:
        if window is not None:
            raise ValueError("uint8 samples are written as they are: window must be None")
        src_bits, lo, hi = 8, 0, 255
    elif dt == np.uint16:
        if window is None:
            raise ValueError("uint16 samples need window=(lo, hi): v <= lo is written as 0 and v >= hi as 255")
        src_bits = 16
        lo, hi = _png_window(window)
    else:
        raise TypeError(f"8-bit PNGs take uint8 or uint16 samples, got {dt}")
    _check_png_shape(rows, cols)  # the 16-bit writer's limit: cct_png_bound, which sizes the output, has no figure beyond it
    ptr, on_device, keep = _raster_ptr(src, shape, dt, f"PNG batch shape {shape} of {dt}")
    return ptr, on_device, n, rows, cols, src_bits, lo, hi, level, keep


def png8_encode_batch(images, window=None, level=6, shape=None, dtype=None):
    """8-bit grayscale PNGs on the device: a uint8 array (window must be None) or a uint16 array with window=(lo, hi), of
    shape (n, rows, cols) or (rows, cols), or a DeviceBuffer with shape= and dtype= (np.uint8 or np.uint16) given, -> a list
    of n `bytes`.  A uint16 value v becomes the byte ((min(max(v, lo), hi) - lo) * 510 + (hi - lo)) // (2 * (hi - lo)):
    round((v - lo) * 255 / (hi - lo)) with halves rounded up, 0 at and below lo, 255 at and above hi; the map runs in
    integers inside the filter kernel.  File i is byte-identical to what Pillow writes for
    Image.fromarray(bytes_i).save(f, "PNG", compress_level=level): level -1 (= 6) or 4 to 9.  Filters, zlib stream and chunks
    as in png_encode_batch, and so is the largest shape (the C entry also takes shapes up to 2^30 - 512 filtered bytes of
    rows * (1 + cols)); png_read_batch reads the files back.  Arguments are checked (TypeError / ValueError) before any
    device call."""
    ptr, on_device, n, rows, cols, src_bits, lo, hi, level, keep = _png8_args(images, window, level, shape, dtype)
    if n == 0:
        return []
    L = _ffi.lib()
    out_stride = L.cct_png_bound(rows, cols)
    out, sizes = _files_out(n, out_stride)
    _ffi.check(L.cct_png_encode8_batch(ptr, on_device, n, rows, cols, src_bits, lo, hi, level, out.ctypes.data, out_stride,
                                       sizes.ctypes.data))
    del keep
    return _files_of(out, sizes)


def decode_png8_batch(files, window, config=None, level=6):
    """Window/level previews of .cct files: each slice is decoded into HBM and written there as an 8-bit PNG through
    window=(lo, hi) (png8_encode_batch), without the rasters coming back to the host.  Returns a list of PNG `bytes`."""
    lo, hi = _png_window(window)
    level = _png_level(level)
    files = _file_list(files, "decode_png8_batch", "file", "a .cct file")
    config = config or default_config()
    if not files:
        return []
    n, w, h, d_img = _decode_to_device(files, config)
    return png8_encode_batch(d_img, window=(lo, hi), level=level, shape=(n, w, h), dtype=np.uint16)


def png_info(file):
    """(rows, cols, bit_depth) of one PNG file (`bytes`), from its signature and IHDR; host only.  ValueError for anything
    png_read_batch does not take: only 8- and 16-bit grayscale without interlace is read."""
    if not isinstance(file, (bytes, bytearray, memoryview)):
        raise TypeError(f"a PNG file is a bytes object, got {type(file).__name__}")
    file = bytes(file)
    rows, cols, depth = C.c_int(0), C.c_int(0), C.c_int(0)
    _ffi.check(_ffi.lib().cct_png_info(file, len(file), C.byref(rows), C.byref(cols), C.byref(depth)))
    return rows.value, cols.value, depth.value


def png_read_batch(files, shift=0, out_dev=None, raise_errors=True):
    """8- and 16-bit grayscale PNG files (a list of `bytes`, all of the shape of the first one; the depths may mix) -> an
    (n, rows, cols) uint16 array of sample >> shift, read on the device: chunk CRC-32s, INFLATE and the row filters.  The
    inverse of png_encode_batch(x, shift=s) for x < 2^(16-s), and with shift=4 of the reference's previews (png_to_array).
    With out_dev it fills that DeviceBuffer and returns the shape, like decode_batch.  With raise_errors=False it returns
    (array or shape, status) with status[i] a CCT_E_* code (include/compact_hip.h lists the refusals); the raster of a
    refused file is unspecified.  Arguments are checked (TypeError / ValueError) before any device call."""
    shift = _png_shift(shift)
    files = _file_list(files, "png_read_batch", "file", "a PNG file")
    _check_out_dev(out_dev)
    n = len(files)
    if n == 0:
        return _no_rasters((0, 0, 0), np.uint16, out_dev, raise_errors)
    rows, cols, _ = png_info(files[0])
    _check_png_shape(rows, cols)
    L = _ffi.lib()
    blob, offs = _archive(files)
    return _decode_rasters(lambda *to: L.cct_png_read_batch(blob, offs.ctypes.data, n, rows, cols, shift, *to), n, rows, cols,
                           np.dtype(np.uint16), out_dev, raise_errors,
                           (_ffi.E_PNG, _ffi.E_MIXED, _ffi.E_CRC, _ffi.E_ZLIB, _ffi.E_STREAM))


def zlib_decompress_batch(streams, max_out, raise_errors=True):
    """INFLATE stage alone on the device: [zlib streams] -> [bytes], what zlib.decompress returns for each
    (the reference calls it at core.py:421).  max_out bounds the inflated size of one stream.  With
    raise_errors=False returns (outputs, status) where status[i] is 0, CCT_E_ZLIB (2) or CCT_E_CAP (6)."""
    L = _ffi.lib()
    n = len(streams)
    if n == 0:
        return [] if raise_errors else ([], np.zeros(0, dtype=np.uint32))
    data, offs = _archive(streams)
    out_stride = (int(max_out) + 15 + 16) & ~15
    out, sizes = _files_out(n, out_stride)
    status = np.zeros(n, dtype=np.uint32)
    rc = L.cct_zlib_decompress_batch(data, offs.ctypes.data, n, out.ctypes.data, out_stride, sizes.ctypes.data,
                                     status.ctypes.data)
    if raise_errors:
        _ffi.check(rc)
    outs = [f if status[i] == 0 else None for i, f in enumerate(_files_of(out, sizes))]
    return outs if raise_errors else (outs, status)


# ---- DICOM RLE Lossless (PS3.5 Annex G): frames on the device, encapsulation on the host ----------------------------

_DICOM_ITEM = b"\xfe\xff\x00\xe0"
_DICOM_SEQ_DELIM = b"\xfe\xff\xdd\xe0\x00\x00\x00\x00"
_RLE_MAX_PIXELS = 1 << 26


def _check_rle_shape(rows, cols):
    if rows < 1 or cols < 1:
        raise ValueError(f"DICOM RLE frame of {rows} x {cols} samples: rows and cols must be >= 1")
    if rows * cols > _RLE_MAX_PIXELS:
        raise ValueError(f"DICOM RLE frame of {rows} x {cols} samples: more than {_RLE_MAX_PIXELS} pixels")


def dicom_rle_encode_batch(images, shape=None, dtype=None):
    """DICOM RLE Lossless frames (transfer syntax 1.2.840.10008.1.2.5) on the device: a uint16 or uint8 array of shape
    (n, rows, cols) or (rows, cols), or a DeviceBuffer with shape= given (dtype= np.uint16 unless np.uint8 is named), -> a
    list of n `bytes`.  Frame i is the 64-byte header and one PackBits segment per byte plane (high byte first), rows coded
    one by one with the rule of pydicom's pure-Python encoder; tests/dicom_rle_model.py states it.  dicom_encapsulate wraps
    frames as PixelData.  Arguments are checked (TypeError / ValueError) before any device call."""
    src, shape, dt = _raster_batch(images, shape, dtype, "dicom_rle_encode_batch", "frame")
    n, rows, cols = shape
    if dt != np.uint8 and dt != np.uint16:
        raise TypeError(f"DICOM RLE frames take uint8 or uint16 samples, got {dt}")
    if n == 0:
        return []
    _check_rle_shape(rows, cols)
    bits = 8 * dt.itemsize
    ptr, on_device, keep = _raster_ptr(src, shape, dt, f"frame batch shape {shape} of {dt}")
    L = _ffi.lib()
    out_stride = L.cct_dicom_rle_bound(rows, cols, bits)
    out, sizes = _files_out(n, out_stride)
    _ffi.check(L.cct_dicom_rle_encode_batch(ptr, on_device, n, rows, cols, bits, out.ctypes.data, out_stride, sizes.ctypes.data))
    del keep
    return _files_of(out, sizes)


def dicom_rle_decode_batch(frames, rows, cols, bits=16, out_dev=None, raise_errors=True):
    """DICOM RLE Lossless frames (a list of `bytes`, one sample per pixel, `bits` = 8 or 16 allocated) -> an (n, rows, cols)
    uint8 / uint16 array, decoded on the device; frames of any conforming encoder are read (packets may cross row ends).
    With out_dev it fills that DeviceBuffer and returns the shape, like decode_batch.  With raise_errors=False it returns
    (array or shape, status) with status[i] 0 or CCT_E_STREAM (a frame shorter than its header, a segment count other than
    bits / 8, offsets that do not start at 64, do not increase or leave the frame, a segment that yields fewer than
    rows * cols bytes); the raster of a refused frame is unspecified.  Arguments are checked before any device call."""
    rows, cols, bits = _ints(rows=rows, cols=cols, bits=bits)
    if bits not in (8, 16):
        raise ValueError(f"DICOM RLE frames of {bits} bits allocated: 8 or 16")
    _check_rle_shape(rows, cols)
    frames = _file_list(frames, "dicom_rle_decode_batch", "frame", "a frame")
    _check_out_dev(out_dev)
    n, dt = len(frames), np.dtype(np.uint8 if bits == 8 else np.uint16)
    if n == 0:
        return _no_rasters((0, rows, cols), dt, out_dev, raise_errors)
    L = _ffi.lib()
    blob, offs = _archive(frames)
    return _decode_rasters(lambda *to: L.cct_dicom_rle_decode_batch(blob, offs.ctypes.data, n, rows, cols, bits, *to), n, rows,
                           cols, dt, out_dev, raise_errors, (_ffi.E_STREAM,))


def dicom_encapsulate(frames):
    """Encapsulated PixelData of a list of frames (PS3.5 A.4): the Basic Offset Table item with one uint32 offset per frame,
    one item per frame (each frame in exactly one fragment, padded to even length), the sequence delimiter.  Host only."""
    items, offsets = bytearray(), []
    for f in _file_list(frames, "dicom_encapsulate", "frame", "a frame"):
        f = bytes(f)
        if len(f) & 1:
            f += b"\0"
        offsets.append(len(items))
        items += _DICOM_ITEM + len(f).to_bytes(4, "little") + f
    bot = b"".join(o.to_bytes(4, "little") for o in offsets)
    return _DICOM_ITEM + len(bot).to_bytes(4, "little") + bot + bytes(items) + _DICOM_SEQ_DELIM


def dicom_fragments(pixel_data):
    """The frames of encapsulated PixelData (one fragment per frame; a fragment keeps its pad byte, which the RLE decoder
    ignores).  ValueError on a malformed item structure: an unknown tag, an item running past the data, no sequence
    delimiter or bytes behind it, no Basic Offset Table item, a table that does not list the fragments.  Host only."""
    if not isinstance(pixel_data, (bytes, bytearray, memoryview)):
        raise TypeError(f"PixelData is a bytes object, got {type(pixel_data).__name__}")
    d = bytes(pixel_data)
    pos, items = 0, []
    while True:
        if pos + 8 > len(d):
            raise ValueError("PixelData ends without a sequence delimiter")
        tag, ln = d[pos:pos + 4], int.from_bytes(d[pos + 4:pos + 8], "little")
        pos += 8
        if tag == _DICOM_SEQ_DELIM[:4]:
            if ln != 0 or pos != len(d):
                raise ValueError("sequence delimiter with a length, or bytes behind it")
            break
        if tag != _DICOM_ITEM:
            raise ValueError(f"tag {tag.hex()} where an item was expected")
        if pos + ln > len(d):
            raise ValueError("item runs past the PixelData")
        items.append(d[pos:pos + ln])
        pos += ln
    if not items:
        raise ValueError("no Basic Offset Table item")
    bot, frames = items[0], items[1:]
    if len(bot) % 4 or (bot and len(bot) != 4 * len(frames)):
        raise ValueError("Basic Offset Table does not list the fragments")
    starts, at = [], 0
    for f in frames:
        starts.append(at)
        at += 8 + len(f)
    if bot and [int.from_bytes(bot[4 * k:4 * k + 4], "little") for k in range(len(frames))] != starts:
        raise ValueError("Basic Offset Table does not list the fragments")
    return frames


# ---- JPEG Lossless, SOF3 (T.81 process 14; DICOM 1.2.840.10008.1.2.4.70): frames on the device ----------------------

_JPL_MAX_PIXELS = 1 << 26


def _check_jpl_shape(rows, cols, what="JPEG Lossless"):
    if not 1 <= rows <= 65535 or not 1 <= cols <= 65535:
        raise ValueError(f"{what} frame of {rows} x {cols} samples: rows and cols are 1 to 65535")
    if rows * cols > _JPL_MAX_PIXELS:
        raise ValueError(f"{what} frame of {rows} x {cols} samples: more than {_JPL_MAX_PIXELS} pixels")


def _check_jpl_predictor(predictor):
    """selection value 1 .. 7, or 0 for "auto" / 0; TypeError for what is neither an integer nor a string, ValueError else"""
    if isinstance(predictor, str):
        if predictor != "auto":
            raise ValueError(f"JPEG Lossless predictor {predictor!r}: 1 to 7, or 'auto'")
        return 0
    predictor, = _ints(predictor=predictor)
    if not 0 <= predictor <= 7:
        raise ValueError(f"JPEG Lossless predictor {predictor}: 1 to 7, or 'auto' (0)")
    return predictor


def jpeg_lossless_encode_batch(images, precision=None, restart_rows=0, shape=None, dtype=None, predictor=1):
    """JPEG Lossless frames on the device, with selection value 1 unless predictor says otherwise (DICOM transfer syntax
    1.2.840.10008.1.2.4.70; any other predictor: 1.2.840.10008.1.2.4.57): a uint16 or
    uint8 array of shape (n, rows, cols) or (rows, cols), or a DeviceBuffer with shape= given (dtype= np.uint16 unless
    np.uint8 is named), -> a list of n `bytes`, each one interchange file: SOI, SOF3, DHT, DRI (with restart_rows > 0: a
    restart interval of that many rows, at most 65535 samples), SOS, entropy-coded segment, EOI.  precision is 2 .. 16 and
    defaults to the sample width; uint8 samples take at most 8.  The Huffman table is the frame's own (T.81 Annex K.2);
    tests/jpeg_lossless_model.py states the file.  A sample >= 2^precision raises OverflowError.  dicom_encapsulate wraps
    the frames as PixelData.  predictor is the selection value 1 .. 7 of T.81 Table H.1 for every frame, or "auto" (0): the
    device builds the seven histograms and tables of each frame and writes the one with the fewest coded bits, its DHT
    counted, ties to the lowest; that estimate leaves out byte stuffing and pad bits, so it is the smallest estimate and not
    provably the smallest file.  Frames of one call may then differ; the Ss is in each file's SOS.
    Arguments are checked (TypeError / ValueError) before any device call.
    Memory: the call reserves cct_jpegll_bound(rows, cols, restart_rows) bytes per frame on the host, the worst case of 31
    bits a sample doubled by byte stuffing, about 7.75 bytes a sample (2 MB for 512 x 512, 520 MB for 256 such frames;
    pages a file does not reach are never touched), and on the device that plus 4 bytes a sample, at most 512 MB at a time:
    split a large batch if the address space matters."""
    src, shape, dt = _raster_batch(images, shape, dtype, "jpeg_lossless_encode_batch", "frame")
    n, rows, cols = shape
    if dt != np.uint8 and dt != np.uint16:
        raise TypeError(f"JPEG Lossless frames take uint8 or uint16 samples, got {dt}")
    src_bits = 8 * dt.itemsize
    precision, restart_rows = _ints(precision=src_bits if precision is None else precision, restart_rows=restart_rows)
    predictor = _check_jpl_predictor(predictor)
    if not 2 <= precision <= 16:
        raise ValueError(f"JPEG Lossless precision {precision}: 2 to 16")
    if precision > src_bits:
        raise ValueError(f"precision {precision} for {dt} samples: at most {src_bits}")
    if restart_rows < 0:
        raise ValueError(f"restart_rows {restart_rows}: 0 (no restart intervals) or a number of rows")
    if n == 0:
        return []
    _check_jpl_shape(rows, cols)
    if restart_rows * cols > 65535:
        raise ValueError(f"a restart interval of {restart_rows} rows of {cols} samples: Ri is at most 65535")
    ptr, on_device, keep = _raster_ptr(src, shape, dt, f"frame batch shape {shape} of {dt}")
    L = _ffi.lib()
    out_stride = L.cct_jpegll_bound(rows, cols, restart_rows)
    out, sizes = _files_out(n, out_stride)
    status = np.zeros(n, dtype=np.uint32)
    _ffi.check(L.cct_jpegll_encode_batch_sv(ptr, on_device, n, rows, cols, src_bits, precision, predictor, restart_rows,
                                            out.ctypes.data, out_stride, sizes.ctypes.data, status.ctypes.data, None))
    del keep
    return _files_of(out, sizes)


def jpeg_lossless_info(file):
    """(rows, cols, precision) of one JPEG Lossless file (`bytes`), from its SOF3 after the whole marker walk; host only.
    ValueError for anything jpeg_lossless_decode_batch refuses by structure (CCT_E_JPEG in include/compact_hip.h)."""
    if not isinstance(file, (bytes, bytearray, memoryview)):
        raise TypeError(f"a JPEG file is a bytes object, got {type(file).__name__}")
    file = bytes(file)
    rows, cols, prec = C.c_int(0), C.c_int(0), C.c_int(0)
    _ffi.check(_ffi.lib().cct_jpegll_info(file, len(file), C.byref(rows), C.byref(cols), C.byref(prec)))
    return rows.value, cols.value, prec.value


def jpeg_lossless_decode_batch(files, rows, cols, bits=16, out_dev=None, raise_errors=True):
    """JPEG Lossless files (a list of `bytes`: SOF3, one component, precision <= `bits` = 8 or 16 allocated) -> an
    (n, rows, cols) uint8 / uint16 array, decoded on the device: any of the seven predictors, a point transform (the sample
    returned is value << Pt), restart intervals of whole rows, any Huffman table over the categories 0 .. 16.  With out_dev
    it fills that DeviceBuffer and returns the shape, like decode_batch.  With raise_errors=False it returns (array or
    shape, status) with status[i] 0, CCT_E_JPEG (13: the structure), CCT_E_MIXED (10: not rows x cols, or a precision above
    bits) or CCT_E_STREAM (4: the entropy-coded data); include/compact_hip.h lists the cases.  The raster of a refused file
    is unspecified.  Arguments are checked before any device call."""
    rows, cols, bits = _ints(rows=rows, cols=cols, bits=bits)
    if bits not in (8, 16):
        raise ValueError(f"JPEG Lossless rasters of {bits} bits allocated: 8 or 16")
    _check_jpl_shape(rows, cols)
    files = _file_list(files, "jpeg_lossless_decode_batch", "file", "a JPEG file")
    _check_out_dev(out_dev)
    n, dt = len(files), np.dtype(np.uint8 if bits == 8 else np.uint16)
    if n == 0:
        return _no_rasters((0, rows, cols), dt, out_dev, raise_errors)
    L = _ffi.lib()
    blob, offs = _archive(files)
    return _decode_rasters(lambda *to: L.cct_jpegll_decode_batch(blob, offs.ctypes.data, n, rows, cols, bits, *to), n, rows,
                           cols, dt, out_dev, raise_errors, (_ffi.E_JPEG, _ffi.E_MIXED, _ffi.E_STREAM))


# ---- JPEG-LS lossless (T.87; DICOM 1.2.840.10008.1.2.4.80): files on the device ------------------------------------------

def jpeg_ls_encode_batch(images, precision=None, restart_rows=0, shape=None, dtype=None):
    """JPEG-LS lossless files (ITU-T T.87 with NEAR = 0, DICOM transfer syntax 1.2.840.10008.1.2.4.80) on the device: a
    uint16 or uint8 array of shape (n, rows, cols) or (rows, cols), or a DeviceBuffer with shape= given (dtype= np.uint16
    unless np.uint8 is named), -> a list of n `bytes`, each one file: SOI, SOF55, DRI (with restart_rows > 0: a restart
    interval of that many lines, at most 65535), SOS, the scan, EOI.  precision is 2 .. 16 and defaults to the sample width;
    uint8 samples take at most 8.  The preset parameters are the defaults of the precision and no LSE segment is written;
    tests/jpeg_ls_model.py states the file.  A sample >= 2^precision raises OverflowError.  dicom_encapsulate wraps the
    files as PixelData.  Arguments are checked (TypeError / ValueError) before any device call.
    A file without restart intervals is coded by one wave, one after the other of its lines: restart_rows trades a few
    bytes an interval for that many waves a frame.
    Memory: the call reserves cct_jpegls_bound(rows, cols, restart_rows) bytes per frame on the host, the worst case of 64
    bits a sample and 7 bits a byte, about 9.2 bytes a sample (2.4 MB for 512 x 512, 613 MB for 256 such frames; pages a
    file does not reach are never touched), and on the device twice that, at most 512 MB at a time: split a large batch
    if the address space matters."""
    src, shape, dt = _raster_batch(images, shape, dtype, "jpeg_ls_encode_batch", "frame")
    n, rows, cols = shape
    if dt != np.uint8 and dt != np.uint16:
        raise TypeError(f"JPEG-LS frames take uint8 or uint16 samples, got {dt}")
    src_bits = 8 * dt.itemsize
    precision, restart_rows = _ints(precision=src_bits if precision is None else precision, restart_rows=restart_rows)
    if not 2 <= precision <= 16:
        raise ValueError(f"JPEG-LS precision {precision}: 2 to 16")
    if precision > src_bits:
        raise ValueError(f"precision {precision} for {dt} samples: at most {src_bits}")
    if not 0 <= restart_rows <= 65535:
        raise ValueError(f"restart_rows {restart_rows}: 0 (no restart intervals) or a number of lines up to 65535")
    if n == 0:
        return []
    _check_jpl_shape(rows, cols, "JPEG-LS")
    ptr, on_device, keep = _raster_ptr(src, shape, dt, f"frame batch shape {shape} of {dt}")
    L = _ffi.lib()
    out_stride = L.cct_jpegls_bound(rows, cols, restart_rows)
    out, sizes = _files_out(n, out_stride)
    status = np.zeros(n, dtype=np.uint32)
    _ffi.check(L.cct_jpegls_encode_batch(ptr, on_device, n, rows, cols, src_bits, precision, restart_rows, out.ctypes.data,
                                         out_stride, sizes.ctypes.data, status.ctypes.data))
    del keep
    return _files_of(out, sizes)


def jpeg_ls_info(file):
    """(rows, cols, precision) of one JPEG-LS file (`bytes`), from its SOF55 after the whole marker walk; host only.
    ValueError for anything jpeg_ls_decode_batch refuses by structure (CCT_E_JPEGLS in include/compact_hip.h)."""
    if not isinstance(file, (bytes, bytearray, memoryview)):
        raise TypeError(f"a JPEG-LS file is a bytes object, got {type(file).__name__}")
    file = bytes(file)
    rows, cols, prec = C.c_int(0), C.c_int(0), C.c_int(0)
    _ffi.check(_ffi.lib().cct_jpegls_info(file, len(file), C.byref(rows), C.byref(cols), C.byref(prec)))
    return rows.value, cols.value, prec.value


def jpeg_ls_decode_batch(files, rows, cols, bits=16, out_dev=None, raise_errors=True):
    """JPEG-LS lossless files (a list of `bytes`: SOF55, one component, NEAR = 0, precision <= `bits` = 8 or 16 allocated)
    -> an (n, rows, cols) uint8 / uint16 array, decoded on the device: restart intervals of whole lines, the default preset
    parameters or those of an LSE segment of id 1.  With out_dev it fills that DeviceBuffer and returns the shape, like
    decode_batch.  With raise_errors=False it returns (array or shape, status) with status[i] 0, CCT_E_JPEGLS (16: the
    structure), CCT_E_MIXED (10: not rows x cols, or a precision above bits) or CCT_E_STREAM (4: the scan data);
    include/compact_hip.h lists the cases.  The raster of a refused file is unspecified.  Arguments are checked before any
    device call."""
    rows, cols, bits = _ints(rows=rows, cols=cols, bits=bits)
    if bits not in (8, 16):
        raise ValueError(f"JPEG-LS rasters of {bits} bits allocated: 8 or 16")
    _check_jpl_shape(rows, cols, "JPEG-LS")
    files = _file_list(files, "jpeg_ls_decode_batch", "file", "a JPEG-LS file")
    _check_out_dev(out_dev)
    n, dt = len(files), np.dtype(np.uint8 if bits == 8 else np.uint16)
    if n == 0:
        return _no_rasters((0, rows, cols), dt, out_dev, raise_errors)
    L = _ffi.lib()
    blob, offs = _archive(files)
    return _decode_rasters(lambda *to: L.cct_jpegls_decode_batch(blob, offs.ctypes.data, n, rows, cols, bits, *to), n, rows,
                           cols, dt, out_dev, raise_errors, (_ffi.E_JPEGLS, _ffi.E_MIXED, _ffi.E_STREAM))


# ---- JPEG 2000 Part-1 lossless (T.800; DICOM 1.2.840.10008.1.2.4.90): files on the device --------------------------------

def jpeg2000_encode_batch(images, precision=None, shift=0, levels=5, codeblock=64, jp2=False, shape=None, dtype=None):
    """JPEG 2000 Part-1 lossless files (DICOM transfer syntax 1.2.840.10008.1.2.4.90) on the device: a uint16 or uint8 array
    of shape (n, rows, cols) or (rows, cols), or a DeviceBuffer with shape= given (dtype= np.uint16 unless np.uint8 is
    named), -> a list of n `bytes`, each one raw codestream (SOC .. EOC) or, with jp2=True, one JP2 file.  precision is
    2 .. 16 and defaults to the sample width; the sample coded is value << shift (shift=4 reproduces the 16-bit PNG preview
    of a 12-bit slice).  levels (0 .. 8) decompositions of the reversible 5/3 transform, code-blocks of codeblock (32 or 64)
    squared, one tile, one layer, LRCP, every coding pass kept; tests/jpeg2000_model.py states the file byte for byte.  A
    sample that does not fit the precision raises OverflowError.  dicom_encapsulate wraps the codestreams as PixelData.
    Arguments are checked (TypeError / ValueError) before any device call.
    Memory: the call reserves cct_j2k_bound(rows, cols, levels, codeblock, jp2) bytes per frame on the host, about 5 bytes
    a sample (1.4 MB for 512 x 512; pages a file does not reach are never touched), and on the device that plus the slabs of
    the same size and 8 bytes a sample, at most 512 MB at a time."""
    src, shape, dt = _raster_batch(images, shape, dtype, "jpeg2000_encode_batch", "frame")
    n, rows, cols = shape
    if dt != np.uint8 and dt != np.uint16:
        raise TypeError(f"JPEG 2000 frames take uint8 or uint16 samples, got {dt}")
    src_bits = 8 * dt.itemsize
    precision, shift, levels, codeblock = _ints(precision=src_bits if precision is None else precision, shift=shift, levels=levels,
                                                codeblock=codeblock)
    if not 2 <= precision <= 16:
        raise ValueError(f"JPEG 2000 precision {precision}: 2 to 16")
    if precision > src_bits:
        raise ValueError(f"precision {precision} for {dt} samples: at most {src_bits}")
    if not 0 <= shift <= 15 or precision - shift < 1:
        raise ValueError(f"shift {shift} at precision {precision}: 0 to 15 and below the precision")
    if not 0 <= levels <= 8:
        raise ValueError(f"{levels} decomposition levels: 0 to 8")
    if codeblock not in (32, 64):
        raise ValueError(f"code-blocks of {codeblock}: 32 or 64")
    if n == 0:
        return []
    if not 1 <= rows <= 65535 or not 1 <= cols <= 65535 or rows * cols > _JPL_MAX_PIXELS:
        raise ValueError(f"JPEG 2000 frame of {rows} x {cols} samples: rows and cols are 1 to 65535, at most {_JPL_MAX_PIXELS} pixels")
    ptr, on_device, keep = _raster_ptr(src, shape, dt, f"frame batch shape {shape} of {dt}")
    L = _ffi.lib()
    out_stride = L.cct_j2k_bound(rows, cols, levels, codeblock, int(bool(jp2)))
    out, sizes = _files_out(n, out_stride)
    status = np.zeros(n, dtype=np.uint32)
    _ffi.check(L.cct_j2k_encode_batch(ptr, on_device, n, rows, cols, src_bits, precision, shift, levels, codeblock, int(bool(jp2)),
                                      out.ctypes.data, out_stride, sizes.ctypes.data, status.ctypes.data))
    del keep
    return _files_of(out, sizes)


def jpeg2000_info(file):
    """(rows, cols, precision) of one JPEG 2000 raw codestream or JP2 file (`bytes`) from its SIZ; host only.  ValueError
    for anything else (CCT_E_J2K in include/compact_hip.h)."""
    if not isinstance(file, (bytes, bytearray, memoryview)):
        raise TypeError(f"a JPEG 2000 file is a bytes object, got {type(file).__name__}")
    file = bytes(file)
    rows, cols, prec = C.c_int(0), C.c_int(0), C.c_int(0)
    _ffi.check(_ffi.lib().cct_j2k_info(file, len(file), C.byref(rows), C.byref(cols), C.byref(prec)))
    return rows.value, cols.value, prec.value


def jpeg2000_decode_batch(files, rows, cols, bits=16, shift=0, out_dev=None, raise_errors=True):
    """JPEG 2000 Part-1 lossless files (a list of `bytes`: raw codestreams or JP2 files of one unsigned component, precision
    <= `bits` = 8 or 16 allocated) -> an (n, rows, cols) uint8 / uint16 array, decoded on the device; the sample returned is
    value >> shift, so jpeg2000_decode_batch(jpeg2000_encode_batch(x, shift=s), ..., shift=s) is x.  Files of any encoder are
    taken within these limits: one tile and one tile-part, origins 0, maximal precincts, no SOP / EPH, any progression order,
    1 to 32 layers, 0 to 8 levels, code-blocks of 4 to 64 by 4 to 64, code-block style 0, the reversible 5/3 transform, no
    quantization, at most 19 magnitude bit-planes a subband; COM, TLM, PLM, PLT and CRG are skipped.  The rest (the 9/7
    transform, precincts, tiles, components, code-block styles, COC / QCC / RGN / POC / PPM / PPT) is refused as CCT_E_J2K: a
    decision about scope, so a caller may fall back on a host decoder for exactly those.  With out_dev it fills that
    DeviceBuffer and returns the shape, like decode_batch.  With raise_errors=False it returns (array or shape, status) with
    status[i] 0, CCT_E_J2K (14: the structure), CCT_E_MIXED (10: not rows x cols, or a precision above bits) or CCT_E_STREAM
    (4: the packets); include/compact_hip.h lists the cases.  The raster of a refused file is unspecified.  Arguments are
    checked before any device call."""
    rows, cols, bits, shift = _ints(rows=rows, cols=cols, bits=bits, shift=shift)
    if bits not in (8, 16):
        raise ValueError(f"JPEG 2000 rasters of {bits} bits allocated: 8 or 16")
    if not 0 <= shift <= 15:
        raise ValueError(f"shift {shift}: 0 to 15")
    if not 1 <= rows <= 65535 or not 1 <= cols <= 65535 or rows * cols > _JPL_MAX_PIXELS:
        raise ValueError(f"JPEG 2000 frame of {rows} x {cols} samples: rows and cols are 1 to 65535, at most {_JPL_MAX_PIXELS} pixels")
    files = _file_list(files, "jpeg2000_decode_batch", "file", "a JPEG 2000 file")
    _check_out_dev(out_dev)
    n, dt = len(files), np.dtype(np.uint8 if bits == 8 else np.uint16)
    if n == 0:
        return _no_rasters((0, rows, cols), dt, out_dev, raise_errors)
    L = _ffi.lib()
    blob, offs = _archive(files)
    return _decode_rasters(lambda *to: L.cct_j2k_decode_batch(blob, offs.ctypes.data, n, rows, cols, bits, shift, *to), n, rows,
                           cols, dt, out_dev, raise_errors, (_ffi.E_J2K, _ffi.E_MIXED, _ffi.E_STREAM))


# ---- strip-organised grayscale TIFF (TIFF 6.0; LZW, Deflate, horizontal predictor): files on the device -----------------

_TIFF_COMPRESSION = {"none": 1, "lzw": 5, "deflate": 8}


def _check_tiff_shape(rows, cols):
    if not 1 <= rows <= 65535 or not 1 <= cols <= 65535:
        raise ValueError(f"TIFF raster of {rows} x {cols} samples: rows and cols are 1 to 65535")


def tiff_encode_batch(images, compression="lzw", predictor=1, rows_per_strip=None, level=6, shape=None, dtype=None):
    """Grayscale TIFF files on the device: a uint16 or uint8 array of shape (n, rows, cols) or (rows, cols), or a DeviceBuffer
    with shape= given (dtype= np.uint16 unless np.uint8 is named), -> a list of n `bytes`.  compression is "lzw", "deflate" or
    "none"; predictor 1 or 2 (horizontal differencing; not with "none"); rows_per_strip None for Pillow's rule (strips of at
    most 64 KiB, one row at least) or a height from 1 up, clamped to rows; level (4 to 9, -1 = 6) is Deflate's.  With "lzw",
    and with "deflate" at level 6, the file is byte for byte what Pillow 12 / libtiff 4.7 write for the raster
    (compression="tiff_lzw" / "tiff_adobe_deflate", tiffinfo={317: 2} for predictor 2, TiffImagePlugin.STRIP_SIZE =
    rows_per_strip * row bytes where one is given); at other levels every strip is zlib.compress(strip, level) in the same
    layout, and "none" uses that layout too.  tests/tiff_model.py states layout and coder.  Arguments are checked (TypeError /
    ValueError) before any device call."""
    src, shape, dt = _raster_batch(images, shape, dtype, "tiff_encode_batch", "raster")
    n, rows, cols = shape
    if dt != np.uint8 and dt != np.uint16:
        raise TypeError(f"TIFF rasters take uint8 or uint16 samples, got {dt}")
    if compression not in _TIFF_COMPRESSION:
        raise ValueError(f"TIFF compression {compression!r}: 'lzw', 'deflate' or 'none'")
    (predictor,) = _ints(predictor=predictor)
    if predictor not in (1, 2):
        raise ValueError(f"TIFF predictor {predictor}: 1 or 2")
    if predictor == 2 and compression == "none":
        raise ValueError("TIFF predictor 2 goes with 'lzw' or 'deflate', not with 'none'")
    if rows_per_strip is None:
        rps = 0
    else:
        (rps,) = _ints(rows_per_strip=rows_per_strip)
        if rps < 1:
            raise ValueError(f"TIFF rows_per_strip {rps}: None or a height from 1 up")
        rps = min(rps, 65535)
    (level,) = _ints(level=level)
    if compression == "deflate":
        if level == -1:
            level = 6
        if not 4 <= level <= 9:
            raise ValueError(f"TIFF Deflate level {level}: -1 and 4 to 9 are on the device")
    if n == 0:
        return []
    _check_tiff_shape(rows, cols)
    bits, comp = 8 * dt.itemsize, _TIFF_COMPRESSION[compression]
    ptr, on_device, keep = _raster_ptr(src, shape, dt, f"raster batch shape {shape} of {dt}")
    L = _ffi.lib()
    out_stride = L.cct_tiff_bound(rows, cols, bits, comp, rps)
    if out_stride == 0:
        raise ValueError(f"TIFF raster of {rows} x {cols} samples: the file could pass 4 GiB")
    out, sizes = _files_out(n, out_stride)
    _ffi.check(L.cct_tiff_encode_batch(ptr, on_device, n, rows, cols, bits, comp, predictor, rps, level, out.ctypes.data, out_stride,
                                       sizes.ctypes.data))
    del keep
    return _files_of(out, sizes)


def tiff_info(file):
    """(rows, cols, bits) of one TIFF file (`bytes`) from its first IFD, after every check of tiff_read_batch's parser; host
    only.  ValueError for anything the reader refuses by structure (CCT_E_TIFF in include/compact_hip.h)."""
    if not isinstance(file, (bytes, bytearray, memoryview)):
        raise TypeError(f"a TIFF file is a bytes object, got {type(file).__name__}")
    file = bytes(file)
    rows, cols, bits = C.c_int(0), C.c_int(0), C.c_int(0)
    _ffi.check(_ffi.lib().cct_tiff_info(file, len(file), C.byref(rows), C.byref(cols), C.byref(bits)))
    return rows.value, cols.value, bits.value


def tiff_read_batch(files, rows, cols, bits=16, out_dev=None, raise_errors=True):
    """Grayscale TIFF files (a list of `bytes`) -> an (n, rows, cols) uint8 / uint16 array, decoded on the device.  Taken:
    classic TIFF of either byte order, the first IFD, one sample per pixel of `bits` = 8 or 16, SampleFormat absent or 1,
    Photometric 1, strips of any RowsPerStrip, StripOffsets / StripByteCounts as SHORT or LONG, compression 1, 5 (LZW) or
    8 / 32946 (Deflate), predictor 1 or 2 (2 with 5 and 8 only), FillOrder absent or 1; unknown tags are ignored.  The rest
    (BigTIFF, tiles, PackBits and other compressions, other photometrics, sample counts or depths, a strip outside the
    file, a shape or depth other than the one asked for) is refused on the host as CCT_E_TIFF (15, ValueError) before
    anything is uploaded.  A strip that does not decode to its rows gives CCT_E_STREAM (4) or, from the INFLATE kernel,
    CCT_E_ZLIB (2).  LZW strips are read by libtiff's rules: decoding stops once the strip's bytes are out, a missing EOI is
    no error, repeated Clears are allowed; a strip that does not open with a Clear is refused.  With out_dev it fills that
    DeviceBuffer and returns the shape; with raise_errors=False it returns (array or shape, status) with the per-file codes,
    and the raster of a refused file is unspecified.  Arguments are checked before any device call."""
    rows, cols, bits = _ints(rows=rows, cols=cols, bits=bits)
    if bits not in (8, 16):
        raise ValueError(f"TIFF rasters of {bits} bits per sample: 8 or 16")
    _check_tiff_shape(rows, cols)
    files = _file_list(files, "tiff_read_batch", "file", "a TIFF file")
    _check_out_dev(out_dev)
    n, dt = len(files), np.dtype(np.uint8 if bits == 8 else np.uint16)
    if n == 0:
        return _no_rasters((0, rows, cols), dt, out_dev, raise_errors)
    L = _ffi.lib()
    blob, offs = _archive(files)
    return _decode_rasters(lambda *to: L.cct_tiff_read_batch(blob, offs.ctypes.data, n, rows, cols, bits, *to), n, rows, cols, dt,
                           out_dev, raise_errors, (_ffi.E_TIFF, _ffi.E_STREAM, _ffi.E_ZLIB))
