"""MI355X-native back end of the CompaCT codec: ctypes binding + batch API (no PyTorch)."""
from . import _ffi  # noqa: F401
from .batch import (DeviceBuffer, Event, PinnedArray, codec_params, decode_batch, decode_payload_dev,  # noqa: F401
                    zlib_compress_batch, zlib_decompress_batch, png_encode_batch, decode_png_batch, png_info, png_read_batch,
                    png8_encode_batch, decode_png8_batch,
                    dicom_rle_encode_batch, dicom_rle_decode_batch, dicom_encapsulate, dicom_fragments,
                    jpeg_lossless_encode_batch, jpeg_lossless_decode_batch, jpeg_lossless_info,
                    jpeg_ls_encode_batch, jpeg_ls_decode_batch, jpeg_ls_info,
                    jpeg2000_decode_batch, jpeg2000_encode_batch, jpeg2000_info,
                    tiff_encode_batch, tiff_info, tiff_read_batch,
                    default_config, device_info, encode_batch, encode_payload_dev)
