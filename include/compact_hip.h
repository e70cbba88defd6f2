/*
 * compact_hip.h -- C ABI of libcompact_hip.so, the MI355X (gfx950) implementation of the
 * CompaCT per-slice encode/decode hot path.
 *
 * The reference (taaha-khan/2023-CompaCT-Image-Compression) is pure Python and has no
 * FFI of its own: its contract is the class surface codec.core.Encoder / Decoder
 * (src/codec/core.py:170-365, 367-543).  The entry points below are what a ctypes
 * binding for that surface needs; each one names the reference code it replaces.
 * The Python mirror that binds them lives in 2023-compact-image-compression_amd/codec/
 * and INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a
 * CCT_E_* code and never throws; buffers are caller-allocated; "d_" pointers are device
 * (HBM) addresses obtained from cct_dev_alloc (or any hipMalloc), "h_" pointers are host
 * addresses.  Threading: calls may come from several host threads.  An encode batch call
 * (cct_encode_batch, cct_encode_batch_packed) takes an internal encode slot -- a HIP stream
 * with its own workspaces; by default there is one, so a second call waits (option
 * "encode_slots" = 2: two batches side by side on the device, which pays on some boxes only,
 * see DESIGN.md); decode calls (cct_decode_batch,
 * cct_zlib_decompress_batch) likewise take one of two decode slots ("decode_slots"), next to
 * the encodes; the size gather (cct_allgather_u32) has its own stream as well.  Everything else
 * shares the main stream (= encode slot 0) under one mutex.  The streams are NOT ordered
 * against each other: every host-facing call is complete when it returns (cct_dev_memset
 * and the h2d/d2h copies included); only cct_encode_payload_dev / cct_decode_payload_dev
 * leave work queued (main / decode stream) -- call cct_sync() before another call reads or
 * overwrites their buffers.  Rare runtime work -- capturing and instantiating a slot's graphs, growing a workspace,
 * creating a stream -- is done with no other call of the library in flight (the other calls finish first; a
 * call that arrives meanwhile waits a few milliseconds): this happens on the first batches of a shape only.
 * The library keeps up to eight HIP streams busy; the runtime spreads a process's streams over GPU_MAX_HW_QUEUES hardware
 * queues (default 4) and two streams on one queue run one after the other, so the first device call sets that variable to 8
 * unless the caller has set it (it is read when the HIP runtime initialises: set it yourself if HIP is up before this library).
 * The library initialises HIP lazily on the first device call.  Processes that fork
 * workers (scripts/evaluate.py:107) must fork BEFORE that call: each child then binds the
 * GPU itself.  A child forked after its parent initialised the GPU gets CCT_E_DEVICE from
 * every device call (ROCm cannot share a runtime across fork).
 *
 * There is NO CPU fallback: every function that computes needs a gfx950 device and fails
 * with CCT_E_DEVICE when none is usable.
 */
#ifndef COMPACT_HIP_H
#define COMPACT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCT_ABI_VERSION 1

/* error codes */
#define CCT_OK 0
#define CCT_E_MAGIC 1     /* header magic mismatch          -> ValueError   (core.py:388-389) */
#define CCT_E_ZLIB 2      /* DEFLATE stream invalid          -> zlib.error   (core.py:421)     */
#define CCT_E_OVERFLOW 3  /* pixel left [0,65535] in decode  -> OverflowError(core.py:506,516) */
#define CCT_E_STREAM 4    /* truncated / malformed token stream (TypeError/IndexError there)  */
#define CCT_E_SHAPE 5     /* width*height % block_size != 0  -> ValueError   (core.py:245,429) */
#define CCT_E_CAP 6       /* caller buffer too small */
#define CCT_E_NOMEM 7
#define CCT_E_DEVICE 8    /* no usable gfx950 device / HIP runtime error */
#define CCT_E_ARG 9       /* unsupported argument (block_size outside 3..64, n<0, ...) */
#define CCT_E_MIXED 10    /* decode batch whose members differ in shape or flags */
#define CCT_E_PNG 11      /* cct_png_read_batch / cct_png_info: not a PNG this reader takes -> ValueError */
#define CCT_E_CRC 12      /* cct_png_read_batch: a chunk's CRC-32 does not match           -> ValueError */
#define CCT_E_JPEG 13     /* cct_jpegll_decode_batch / cct_jpegll_info: not a JPEG this reader takes -> ValueError */
#define CCT_E_J2K 14      /* cct_j2k_info / cct_j2k_decode_batch: not a JPEG 2000 codestream or JP2 file they read -> ValueError */
#define CCT_E_TIFF 15     /* cct_tiff_info / cct_tiff_read_batch: not a TIFF file they read -> ValueError */
#define CCT_E_JPEGLS 16   /* cct_jpegls_decode_batch / cct_jpegls_info: not a JPEG-LS file this reader takes -> ValueError */

/* encoder flags: config['encoder']['transforms'] + deflate_compression (core.py:207-209) */
#define CCT_FLAG_FRACTAL 1u       /* transforms.fractal      (core.py:234) */
#define CCT_FLAG_SEGMENTATION 2u  /* transforms.segmentation (core.py:251) */
#define CCT_FLAG_DEFLATE 4u       /* deflate_compression     (core.py:337) */
#define CCT_FLAG_SIGNED_SEG 8u    /* caller's array dtype is int16: segmentation sees signed
                                     values (core.py:254 image.flatten().tolist()) */
/* zlib level of the DEFLATE stage (config['encoder']['deflate_level'], an extension of the reference):
 * field 0 = level 9 (what the reference writes, and every caller that leaves the field clear),
 * 4 .. 9 = that level; 1 .. 3 and 10 .. 15 are refused with CCT_E_ARG.  The level shows only in the
 * second zlib header byte; the 13-byte .cct header is the same and zlib.decompress reads any level.
 * (Under strategies 2 and 3 below, levels 1 .. 3 are accepted too.) */
#define CCT_FLAG_LEVEL_MASK 0xF00u
#define CCT_FLAG_DEFLATE_LEVEL(l) ((((uint32_t)(l)) & 15u) << 8)
/* zlib strategy of the DEFLATE stage (config['encoder']['deflate_strategy'], an extension of the reference), zlib.h's
 * constants: field 0 = Z_DEFAULT_STRATEGY (every caller that leaves the field clear), 1 = Z_FILTERED,
 * 2 = Z_HUFFMAN_ONLY, 3 = Z_RLE, 4 = Z_FIXED; 5 .. 7 are refused with CCT_E_ARG.  Strategies 0, 1 and 4 take
 * the level field's levels 4 .. 9; 2 and 3 take levels 1 .. 9 (field 0 is still level 9) and write the same
 * bytes at each.  The stream is deflateInit2(level, Z_DEFLATED, 15, 8, strategy)'s; the 13-byte .cct header
 * does not change. */
#define CCT_FLAG_STRATEGY_MASK 0x7000u
#define CCT_FLAG_DEFLATE_STRATEGY(s) ((((uint32_t)(s)) & 7u) << 12)

/* per-slice status bits written by the device kernels (0 = clean) */
#define CCT_ST_Q7 1u         /* encode: a traversal delta outside [-2047,2048] was emitted; the
                                stream is reference-identical but not decodable (SURVEY App.A Q7) */
#define CCT_ST_CAP 2u        /* encode: payload stride too small */
#define CCT_ST_OVERFLOW 4u   /* decode: CCT_E_OVERFLOW condition */
#define CCT_ST_STREAM 8u     /* decode: CCT_E_STREAM condition */
#define CCT_ST_ZLIB 16u      /* decode: CCT_E_ZLIB condition (device INFLATE) */

typedef struct cct_header {  /* the 13-byte .cct header (core.py:193-210 / 385-402) */
	int32_t width;             /* image.shape[0] */
	int32_t height;            /* image.shape[1] */
	int32_t channels;
	int32_t bytes_per_channel;
	int32_t fractal, segmentation, deflate;
} cct_header;

typedef struct cct_slice_stats {  /* Encoder.info / partition statistics of one slice */
	uint32_t n_short;      /* info['delta'], core.py:317 */
	uint32_t n_full;       /* info['full'],  core.py:322 */
	uint32_t n_jump;       /* len(BLOCK_JUMPS), cluster.py:166 */
	uint32_t n_difficult;  /* len(block_deltas), cluster.py:51-59 */
} cct_slice_stats;

/* ---- library / device ------------------------------------------------------------- */
int cct_version(void);                 /* returns CCT_ABI_VERSION */
const char *cct_last_error(void);      /* thread-local text of the last failure */
int cct_init(int device);              /* bind HIP device (default: LOCAL_RANK or 0); idempotent */
int cct_shutdown(void);
int cct_device_info(char *name, size_t name_cap, int *compute_units, uint64_t *hbm_bytes);

int cct_dev_alloc(void **d_ptr, size_t bytes);
int cct_dev_free(void *d_ptr);
/* page-locked host memory: archives / file buffers allocated here are copied to and from the device without a
 * staging pass (the batch entry points detect it); plain malloc'ed buffers keep working */
int cct_host_alloc(void **h_ptr, size_t bytes);
int cct_host_free(void *h_ptr);
int cct_h2d(void *d_dst, const void *h_src, size_t bytes);
int cct_d2h(void *h_dst, const void *d_src, size_t bytes);
int cct_dev_memset(void *d_dst, int value, size_t bytes);
int cct_sync(void);
/* elapsed-time markers on the library's stream (bench.py: HIP events around the kernels) */
int cct_event_create(void **ev);
int cct_event_record(void *ev);
int cct_event_elapsed_ms(void *ev_start, void *ev_stop, float *ms); /* synchronises on ev_stop */
int cct_event_destroy(void *ev);

/* ---- traversal -------------------------------------------------------------------- */
/* Replaces GeneralizedHilbertCurve(width, height, get_index=True).generate_all()
 * (src/codec/curve.py:45-138; call sites core.py:234-237, 423-425).  Host code; shape-only. */
int cct_curve_table(int width, int height, int32_t *h_out);

/* ---- sizes ------------------------------------------------------------------------ */
/* bytes one slice's token stream (+EOF) can need; also the stride between slices in d_payload
 * (a multiple of 256). */
size_t cct_payload_stride(int width, int height, int block_size);
/* bytes one .cct file can need (13-byte header + zlib compressBound of the payload) */
size_t cct_file_bound(int width, int height, int block_size);

/* ---- encode ----------------------------------------------------------------------- */
/* Stage (i), the HBM-bound part: traversal -> segmentation/mesh -> delta -> tag-byte pack
 * (+EOF) for n device-resident slices.  Replaces core.py:234-330 + cluster.py:20-199.
 * d_images: n*width*height uint16 (C order, shape (width,height) each).
 * d_payload: n * payload_stride bytes; d_payload_sizes[n]; d_status[n] (CCT_ST_* bits). */
int cct_encode_payload_dev(const uint16_t *d_images, int n, int width, int height,
                           int block_size, uint32_t flags, int eof_byte /* -1 = none */,
                           uint8_t *d_payload, size_t payload_stride,
                           uint32_t *d_payload_sizes, uint32_t *d_status,
                           cct_slice_stats *d_stats /* may be NULL */,
                           uint8_t *d_roles /* may be NULL; n*NB bytes: the block partition
                              (cluster.py:49-199) as one role per traversal block: 0 = emitted alone,
                              1..63 = leader of a meshed pair (BLOCK_JUMPS[b] - b), 0xFF = partner */);

/* Stages (i)+(ii): whole .cct files (header + DEFLATE(level 9) or raw payload) into host
 * memory.  Replaces Encoder.encode (core.py:212-365) for a batch.  Slice i's file is
 * h_out[i*out_stride .. +h_out_sizes[i]).  images_on_device selects d_/h_ meaning of `images`. */
int cct_encode_batch(const uint16_t *images, int images_on_device, int n, int width, int height,
                     int block_size, uint32_t flags, int eof_byte, const char magic[4],
                     int channels, int bytes_per_channel,
                     uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes,
                     uint32_t *h_status /* CCT_ST_* bits per slice */,
                     uint32_t *h_payload_sizes /* may be NULL */,
                     cct_slice_stats *h_stats /* may be NULL */);

/* Same as cct_encode_batch with the files written back to back ("archive" layout, what a corpus
 * run such as scripts/evaluate.py would store): file i = h_archive[h_offsets[i] .. h_offsets[i+1]),
 * h_offsets has n+1 entries; this is exactly the input layout of cct_decode_batch.  Needs
 * CCT_FLAG_DEFLATE and the device DEFLATE path. */
int cct_encode_batch_packed(const uint16_t *images, int images_on_device, int n, int width, int height,
                            int block_size, uint32_t flags, int eof_byte, const char magic[4],
                            int channels, int bytes_per_channel,
                            uint8_t *h_archive, size_t archive_cap, uint64_t *h_offsets,
                            uint32_t *h_out_sizes, uint32_t *h_status,
                            uint32_t *h_payload_sizes /* may be NULL */,
                            cct_slice_stats *h_stats /* may be NULL */);

/* DEFLATE stage alone, on the device: n byte strings (h_in[h_offsets[i] .. h_offsets[i+1])) ->
 * n zlib streams byte-identical to zlib 1.2.11 compress2(level 9), i.e. CPython's
 * zlib.compress(data, level=9) that the reference calls at core.py:340.  Stream i lands at
 * h_out + i*out_stride; out_stride >= compressBound(longest input rounded up to 256) + 64.
 * Option "device_deflate" (default 1) selects this implementation inside cct_encode_batch;
 * 0 runs libz on the host thread team instead. */
int cct_zlib_compress_batch(const uint8_t *h_in, const uint64_t *h_offsets, int n,
                            uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes);

/* cct_zlib_compress_batch at zlib level 4 .. 9 (compress2(level)), or -1 for 6 (Z_DEFAULT_COMPRESSION,
 * what zlib.compress(data) uses).  Levels 0 to 3 (deflate_stored / deflate_fast) are not on the device:
 * any level outside -1, 4 .. 9 returns CCT_E_ARG before the device is touched. */
int cct_zlib_compress_batch_level(const uint8_t *h_in, const uint64_t *h_offsets, int n, int level,
                                  uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes);

/* cct_zlib_compress_batch at a zlib level and strategy: each stream is byte-identical to
 * deflateInit2(level, Z_DEFLATED, 15, 8, strategy) + deflate(Z_FINISH) (zlib.compressobj(level, zlib.DEFLATED,
 * 15, 8, strategy) in Python).  Strategies 0 (Z_DEFAULT_STRATEGY), 1 (Z_FILTERED) and 4 (Z_FIXED) take levels
 * -1 and 4 .. 9; 2 (Z_HUFFMAN_ONLY) and 3 (Z_RLE) take -1 and 1 .. 9 and need no hash chains (a shorter device
 * pass).  Level 0, levels 1 .. 3 with strategies 0, 1 and 4, and strategies outside 0 .. 4 return CCT_E_ARG
 * before the device is touched.  Strategy 0 returns what cct_zlib_compress_batch_level returns. */
int cct_zlib_compress_batch_strategy(const uint8_t *h_in, const uint64_t *h_offsets, int n, int level, int strategy,
                                     uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes);
/* The same with zlib's memLevel: stream i is byte-identical to zlib.compressobj(level, DEFLATED, 15, mem_level,
 * strategy).  mem_level 8 returns what cct_zlib_compress_batch_strategy returns; 9 hashes into 16 bits and ends a block
 * after 32767 symbols (what Pillow's PNG writer uses).  Any other mem_level returns CCT_E_ARG before the device is
 * touched; (level, strategy) are checked as above. */
int cct_zlib_compress_batch_params(const uint8_t *h_in, const uint64_t *h_offsets, int n, int level, int strategy,
                                   int mem_level, uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes);

/* ---- PNG writer ------------------------------------------------------------------------ */
/* Replaces the reference's 16-bit PNG previews (src/codec/core.py:522-538 through imageio, lib/png.py:25-31 through
 * Pillow): n uint16 rasters of shape (rows, cols), C order, on the host (images_on_device 0) or the device (1).  File i,
 * byte-identical to Pillow's Image.fromarray(((img << shift) & 0xFFFF).astype(uint16)).save(f, "PNG",
 * compress_level=level), lands at h_out + i*out_stride, its size in h_out_sizes[i].  Rows are filtered on the device
 * with Pillow's choice among None, Sub, Up and Paeth; the zlib stream is memLevel 9 / Z_FILTERED at `level` (-1 = 6, or
 * 4 .. 9) on the device, or in host libz with device_deflate 0; IDAT chunks of max(65536, 4*cols) bytes with their
 * CRC-32s are packed on the device.  CCT_E_ARG before the device is touched: levels 0 .. 3 and outside -1 .. 9, shift
 * outside 0 .. 15, rows or cols < 1, more than 2^30 - 512 filtered bytes (rows * (1 + 2*cols)).  out_stride >=
 * cct_png_bound(rows, cols) (CCT_E_CAP otherwise; 0 for a refused shape). */
size_t cct_png_bound(int rows, int cols);
int cct_png_encode_batch(const uint16_t *images, int images_on_device, int n, int rows, int cols, int shift, int level,
                         uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes);

/* The 8-bit writer: grayscale files of bit depth 8, the second kind cct_png_read_batch reads, and the window/level previews
 * of CT slices.  n rasters of shape (rows, cols), C order, on the host or the device, of uint16 (src_bits 16) or uint8
 * (src_bits 8) samples.  A uint16 value v goes through the window 0 <= lo < hi <= 65535 to a byte, in integers only:
 *     w = hi - lo;  c = min(max(v, lo), hi);  y = ((c - lo) * 510 + w) / (2 * w)
 * which is round((c - lo) * 255 / w) with halves rounded up: v <= lo gives 0, v >= hi gives 255.  uint8 samples are written
 * as they are; their window must be (0, 255), the identity.  File i is byte-identical to Pillow's
 * Image.fromarray(y.astype(uint8)).save(f, "PNG", compress_level=level) and lands at h_out + i*out_stride, its size in
 * h_out_sizes[i].  The map is applied as the filter kernel loads a row (no 8-bit raster is written to device memory); filter
 * choice, zlib stream (level -1 = 6, or 4 .. 9; host libz with device_deflate 0), IDAT chunk size and packing are those of
 * cct_png_encode_batch, and the call takes the encode slot like it.  CCT_E_ARG before the device is touched: levels 0 .. 3 and
 * outside -1 .. 9, src_bits not 8 or 16, lo < 0, hi > 65535, lo >= hi, src_bits 8 with another window than (0, 255), rows
 * or cols < 1, n < 0, more than 2^30 - 512 filtered bytes (rows * (1 + cols)).  out_stride >= cct_png_bound(rows, cols)
 * (CCT_E_CAP otherwise): the bound of the 16-bit file is sufficient for the 8-bit file of the same shape, whose rows, zlib
 * stream and chunk count are never larger.  A shape that only the 8-bit file fits (cct_png_bound returns 0 while
 * rows * (1 + cols) is within the limit) needs the same expression on its own filtered bytes; the CCT_E_CAP message names
 * the figure. */
int cct_png_encode8_batch(const void *images, int images_on_device, int n, int rows, int cols,
                          int src_bits /* 8 or 16 */, int lo, int hi, int level,
                          uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes);

/* ---- PNG reader ------------------------------------------------------------------------ */
/* The inverse of the writer and of the reference's png_to_array (lib/png.py:33-38, value >> 4): grayscale PNG files of bit
 * depth 8 or 16 -> uint16 rasters, pixel = sample >> shift (8-bit samples widened first; 16-bit samples are big-endian in
 * the file).  Accepted: colour type 0, depth 8 or 16, compression 0, filter method 0, interlace 0; the five row filter types;
 * any number of IDAT chunks of any length (0 included); ancillary chunks anywhere.
 * cct_png_info: host only, no device: signature + IHDR of one file; CCT_E_PNG for anything the reader does not take.
 * cct_png_read_batch: n files laid out back to back (file i = h_files[h_offsets[i] .. h_offsets[i+1])), all of IHDR height ==
 * rows and width == cols (the two depths may mix), -> n*rows*cols uint16 at `images` (host or device).  The host walks the
 * chunk heads; the chunk CRC-32s are checked, the IDAT data gathered, the streams inflated and the rows unfiltered on the
 * device (a decode slot, see the threading paragraph at the top).  Per-file refusals in h_status[i]; the other files still
 * decode, and the call returns the first non-OK status:
 *   CCT_E_PNG    bad signature; first chunk not a 13-byte IHDR; a chunk length running past the file; no IEND, or an IEND
 *                with data; bytes after IEND; no IDAT; IDAT chunks not consecutive; an unknown critical chunk (upper-case
 *                first letter; PLTE counts); a chunk type that is not four letters; any other colour type, depth, compression,
 *                filter method or interlace
 *   CCT_E_MIXED  IHDR size differs from rows x cols
 *   CCT_E_CRC    CRC-32 mismatch on any chunk, ancillary ones included
 *   CCT_E_ZLIB   whatever the device INFLATE rejects (cct_zlib_decompress_batch)
 *   CCT_E_STREAM the stream inflates to fewer or more than rows * (1 + cols * depth/8) bytes, or a filter byte above 4
 * This is stricter than Pillow in two intended ways: Pillow (12.2) checks no CRC of an ancillary chunk behind the image
 * data, and it opens a stream that carries bytes to spare, or that is a whole row short, without an error.  The raster of a refused file is unspecified; nothing is written outside
 * that file's own rows*cols slot.  Whole-call errors, before the device is touched: CCT_E_ARG for shift outside 0 .. 15, rows
 * or cols < 1, n < 0, more than 2^30 - 512 filtered bytes (rows * (1 + 2*cols), the writer's limit); CCT_E_CAP for
 * images_cap_px < n*rows*cols. */
int cct_png_info(const uint8_t *h_file, size_t len, int *rows, int *cols, int *bit_depth);
int cct_png_read_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int rows, int cols, int shift,
                       uint16_t *images, int images_on_device, size_t images_cap_px, uint32_t *h_status /* CCT_E_* per file */);

/* INFLATE stage alone, on the device: n zlib streams (h_in[h_offsets[i] .. h_offsets[i+1])) -> the bytes
 * zlib.decompress returns for each (what the reference calls at core.py:421).  Output i lands at
 * h_out + i*out_stride (out_stride a multiple of 16); h_status[i] = CCT_OK, CCT_E_ZLIB (anything libz
 * rejects: bad header, invalid code, distance too far back, truncated stream, Adler-32 mismatch) or
 * CCT_E_CAP (the stream inflates to more than out_stride bytes).  Returns the first non-OK status.
 * Option "device_inflate" (default 1) selects this implementation inside cct_decode_batch. */
int cct_zlib_decompress_batch(const uint8_t *h_in, const uint64_t *h_offsets, int n,
                              uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes, uint32_t *h_status);

/* ---- decode ----------------------------------------------------------------------- */
/* Replaces Decoder.read_header (core.py:385-402). */
int cct_read_header(const uint8_t *h_file, size_t len, const char magic[4], cct_header *out);

/* Token stream -> raster for n device-resident payloads of one shape.  Replaces
 * core.py:423-520.  d_payload_sizes[i] counts the trailing EOF byte, which is ignored
 * exactly like ByteReader.padding_len (core.py:136-142). */
int cct_decode_payload_dev(const uint8_t *d_payload, size_t payload_stride,
                           const uint32_t *d_payload_sizes, int n, int width, int height,
                           int block_size, int fractal,
                           uint16_t *d_images, uint32_t *d_status);

/* Whole files -> rasters (Decoder.decode with out_path=None, core.py:404-543) for n files of
 * identical shape/flags laid out back to back: file i = h_files[h_offsets[i] .. h_offsets[i+1]).
 * Output: n*width*height uint16 at `images` (device or host). */
int cct_decode_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int block_size,
                     const char magic[4], uint16_t *images, int images_on_device,
                     size_t images_cap_px, uint32_t *h_status /* CCT_E_* code per file */);

/* ---- multi-GPU: the path's only exchange step ----------------------------------------- */
/* Slices shard over GPUs with no data-path collective (scripts/evaluate.py:107-119 treats them as independent units too);
 * what ranks exchange is the per-slice compressed size, so that every rank knows every file's offset in the archive.
 * One process per GPU.  RCCL (librccl.so, loaded on first use) carries the all-gather over xGMI.  Bootstrap: rank 0 calls
 * cct_comm_unique_id and hands the 128 bytes to the other ranks by whatever channel the launcher has (bench.py: a file
 * next to the rendezvous port); then every rank calls cct_comm_init.  No PyTorch anywhere. */
#define CCT_COMM_ID_BYTES 128
int cct_comm_unique_id(void *id128);                             /* ncclGetUniqueId */
int cct_comm_init(const void *id128, int rank, int world);        /* ncclCommInitRank on the library's device */
int cct_comm_info(int *rank, int *world);                         /* -1, 0 when no communicator exists */
/* every rank passes its n_local values and the same max_local >= every rank's n_local; h_all receives world * max_local
 * values, rank r's at h_all[r * max_local ..] (the caller trims by the counts it gathers the same way).  Without a
 * communicator: a plain copy (single-process use). */
int cct_allgather_u32(const uint32_t *h_local, int n_local, int max_local, uint32_t *h_all);
int cct_comm_destroy(void);

/* ---- PackBits utility -------------------------------------------------------------- */
/* Replaces PackBits(apply_delta_transform).encode / .decode of src/codec/packbits.py:74-163 (dead code in the reference:
 * nothing imports it, the .cct path never runs it) for n byte strings h_in[h_offsets[i] .. h_offsets[i+1]).
 * Output i lands at h_out + i*out_stride.  Encode needs out_stride >= cct_packbits_bound(longest input); decode reports
 * CCT_E_CAP per string when out_stride is too small and CCT_E_STREAM for a run header without its byte. */
size_t cct_packbits_bound(size_t n_bytes);
int cct_packbits_encode_batch(const uint8_t *h_in, const uint64_t *h_offsets, int n, int delta_transform,
                              uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes);
int cct_packbits_decode_batch(const uint8_t *h_in, const uint64_t *h_offsets, int n, int delta_transform,
                              uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes, uint32_t *h_status);

/* ---- DICOM RLE Lossless ------------------------------------------------------------- */
/* The RLE column of the reference's comparison (scripts/evaluate.py:78-85, pydicom's Dataset.compress with
 * RLELossless): frames of transfer syntax 1.2.840.10008.1.2.5 (DICOM PS3.5 Annex G) for one sample per pixel with 8 or 16
 * bits allocated.  A frame is sixteen little-endian uint32 (the segment count, the segments' offsets from the frame start,
 * zeros), then one segment per byte plane, most significant byte first: the plane in raster order, PackBits-coded row by
 * row, padded with one 0x00 to an even length.  This is not the PackBits of cct_packbits_* above (chunks of 127, one string
 * per wave), which stays what it is.
 * cct_dicom_rle_encode_batch: n rasters of shape (rows, cols), C order, uint16 (bits 16) or uint8 (bits 8), on the host
 * (images_on_device 0) or the device (1).  Frame i lands at h_out + i*out_stride, its size in h_out_sizes[i].  Rows are
 * coded with the rule of pydicom's pure-Python encoder: maximal groups of equal bytes; a group of one joins the pending
 * literals; a longer group flushes them and leaves as (129, v) per full 128 bytes and (257 - r, v) for a remainder r >= 2
 * or (0, v) for r = 1; literals leave in chunks of 128; nothing carries across rows (tests/dicom_rle_model.py states the
 * rule in Python).  The call takes the encode slot, like the PNG writer.  out_stride >= cct_dicom_rle_bound(rows, cols,
 * bits) = 64 + bits/8 * 2 * rows * cols (CCT_E_CAP otherwise; 0 for a refused shape).
 * cct_dicom_rle_decode_batch: n frames laid out back to back (frame i = h_frames[h_offsets[i] .. h_offsets[i+1])) ->
 * n*rows*cols uint16 (bits 16) or uint8 (bits 8) at `images` (host or device), images_cap_px counted in pixels.  The host
 * parses the headers, the device decodes the segments (a decode slot, like the PNG reader): header byte h < 128 copies the
 * next h + 1 bytes (what is there, if the segment ends first), h > 128 writes 257 - h copies of the next byte (nothing, if
 * there is none), 128 does nothing; a segment is read until rows*cols bytes are out and whatever follows is ignored (pad,
 * encoder slack); packets may cross row ends.  Per-frame refusals in h_status[i], CCT_E_STREAM: a frame shorter than 64
 * bytes, a segment count other than bits/8, a first offset other than 64, offsets that do not increase or lie past the
 * frame, a segment that yields fewer than rows*cols bytes.  The other frames still decode, nothing is written outside a
 * refused frame's own rows*cols slot, and the call returns the first non-OK status.
 * Whole-call errors of both, before the device is touched: CCT_E_ARG for bits other than 8 or 16, rows or cols < 1, n < 0,
 * rows*cols above 2^26; CCT_E_CAP for out_stride below the bound, or images_cap_px < n*rows*cols.
 * cct_last_timings: [0] the three encode kernels, [4] the three decode kernels, HIP events, summed over the passes. */
size_t cct_dicom_rle_bound(int rows, int cols, int bits);
int cct_dicom_rle_encode_batch(const void *images, int images_on_device, int n, int rows, int cols, int bits /* 8 or 16 */,
                               uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes);
int cct_dicom_rle_decode_batch(const uint8_t *h_frames, const uint64_t *h_offsets, int n, int rows, int cols, int bits,
                               void *images, int images_on_device, size_t images_cap_px, uint32_t *h_status /* CCT_E_* per frame */);

/* ---- JPEG Lossless (SOF3) ------------------------------------------------------------- */
/* JPEG Lossless, Non-Hierarchical, First-Order Prediction (ITU-T T.81 process 14 with selection value 1, DICOM transfer
 * syntax 1.2.840.10008.1.2.4.70) for one sample per pixel; tests/jpeg_lossless_model.py states both directions in Python.
 * cct_jpegll_encode_batch: n rasters of shape (rows, cols), C order, uint16 (src_bits 16) or uint8 (src_bits 8), on the
 * host (images_on_device 0) or the device (1); precision P is 2 .. src_bits.  Frame i lands at h_out + i*out_stride, its
 * size in h_out_sizes[i]: SOI, SOF3, one DHT, DRI (only with restart_rows > 0: Ri = restart_rows * cols <= 65535), SOS
 * (Ss 1, Pt 0), the entropy-coded segment, EOI; no APPn.  The first sample of the image and of every restart interval is
 * predicted by 2^(P-1), the rest of that row by the sample to the left, column 0 of a later row by the sample above.
 * Differences are taken modulo 2^16; the Huffman table is built per frame by Annex K.2 (ties go to the larger symbol, the
 * reserved symbol 256 has frequency 1).  A frame with a sample >= 2^P gets CCT_E_OVERFLOW in h_status[i] and size 0; the
 * other frames are written and the call returns the first non-OK status.  The call takes the encode slot, like the RLE codec.
 * cct_jpegll_encode_batch_sv: the same call with the predictor chosen (process 14 in general, DICOM transfer syntax
 * 1.2.840.10008.1.2.4.57; cct_jpegll_encode_batch is this call with predictor 1).  predictor 1 .. 7 is the selection value Ss
 * of every frame's SOS: Ra, Rb, Rc, Ra + Rb - Rc, Ra + ((Rb - Rc) >> 1), Rb + ((Ra - Rc) >> 1), (Ra + Rb) >> 1 in 32-bit signed
 * arithmetic with an arithmetic shift (Ra left, Rb above, Rc above left); the three rules above for an interval's first
 * sample, its first row and column 0 hold under every Ss (T.81 H.1.2).  predictor 0 lets the device choose per frame: it
 * builds the seven category histograms and Annex K.2 tables and takes the Ss with the smallest
 * sum_s hist[s] * (size[s] + (s < 16 ? s : 0)) + 8 * (number of HUFFVAL bytes) bits, ties to the lowest Ss.  That counts the
 * coded bits before byte stuffing and without the pad bits of the intervals: the smallest estimate, not provably the
 * smallest file.  Frames of one call may differ in Ss.  h_predictors, which may be NULL, receives the Ss written for
 * frame i, also for a frame that fails with CCT_E_OVERFLOW.  A predictor outside 0 .. 7 is CCT_E_ARG.
 * cct_jpegll_bound(rows, cols, restart_rows): a sample costs at most 31 bits (a 16-bit code and 15 extra bits), an interval
 * of s samples at most ceil(31 s / 8) bytes, doubled by byte stuffing, plus 2 for its RST; headers and EOI stay below 72:
 * 72 + intervals * (2 * ceil(31 s / 8) + 2).  0 for a refused shape; out_stride below it is CCT_E_CAP.
 * That is about 7.75 bytes a sample (2 MB for 512 x 512): size h_out for it, the files themselves are a fraction of it
 * and each is copied out at its own length.
 * cct_jpegll_info: (rows, cols, precision) of one file from its SOF3, after the whole marker walk; host only.
 * cct_jpegll_decode_batch: n files laid out back to back -> n*rows*cols uint16 (bits 16) or uint8 (bits 8) at `images`
 * (host or device), images_cap_px counted in pixels; a decode slot.  The host walks the markers and takes: any APPn / COM
 * segment; SOF3 with Nf = 1, P 2 .. 16 (<= bits), Y = rows, X = cols (anything else: CCT_E_MIXED); DHT segments of class 0
 * with ids 0 .. 3, which may hold several tables and redefine one, symbols <= 16, codes not over-subscribed; DRI with Ri a
 * multiple of cols; one SOS with Ns = 1, Ss 1 .. 7, Se = 0, Ah = 0, Al = Pt < P; RST markers in sequence; bytes behind
 * EOI.  The sample written is value << Pt.  CCT_E_JPEG, decided before upload: no SOI, SOF3 or EOI, another SOF type,
 * Nf != 1, Y = 0, DNL, a second scan, a table the scan names but nobody defined, a bad segment length, a DRI that is not
 * whole rows.  CCT_E_STREAM, found on the device: a code that is not in the table, entropy-coded data that ends early or
 * leaves whole bytes over, a wrong, missing or spare RST.  Refused files leave the others decoded, nothing is written
 * outside a refused file's own rows*cols slot, and the call returns the first non-OK status.
 * Whole-call errors, before the device is touched: CCT_E_ARG for rows or cols outside 1 .. 65535, rows*cols above 2^26,
 * n < 0, bits or src_bits other than 8 or 16, a precision outside 2 .. src_bits, Ri above 65535, a predictor outside
 * 0 .. 7 (checked first); CCT_E_CAP as above.
 * cct_last_timings: [0] the five encode kernels (six with predictor 0), [4] the decode kernels, HIP events, summed over the passes. */
size_t cct_jpegll_bound(int rows, int cols, int restart_rows);
int cct_jpegll_encode_batch(const void *images, int images_on_device, int n, int rows, int cols, int src_bits /* 8 or 16 */,
                            int precision, int restart_rows, uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes,
                            uint32_t *h_status /* CCT_E_* per frame */);
int cct_jpegll_encode_batch_sv(const void *images, int images_on_device, int n, int rows, int cols, int src_bits /* 8 or 16 */,
                               int precision, int predictor /* 1 .. 7, 0: the frame's best */, int restart_rows, uint8_t *h_out,
                               size_t out_stride, uint32_t *h_out_sizes, uint32_t *h_status /* CCT_E_* per frame */,
                               uint32_t *h_predictors /* may be NULL: the Ss written per frame */);
int cct_jpegll_info(const uint8_t *h_file, size_t len, int *rows, int *cols, int *precision);
int cct_jpegll_decode_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int rows, int cols, int bits, void *images,
                            int images_on_device, size_t images_cap_px, uint32_t *h_status /* CCT_E_* per file */);

/* ---- JPEG-LS lossless (SOF55) --------------------------------------------------------- */
/* JPEG-LS lossless (ITU-T T.87 with NEAR = 0, DICOM transfer syntax 1.2.840.10008.1.2.4.80) for one sample per pixel;
 * tests/jpeg_ls_model.py states the format and both directions in Python.
 * cct_jpegls_encode_batch: n rasters of shape (rows, cols), C order, uint16 (src_bits 16) or uint8 (src_bits 8), on the
 * host (images_on_device 0) or the device (1); precision P is 2 .. src_bits.  Frame i lands at h_out + i*out_stride, its
 * size in h_out_sizes[i]: SOI, SOF55, DRI (only with restart_rows > 0: Ri = restart_rows, counted in lines), SOS (NEAR 0,
 * ILV 0), the scan, EOI; no LSE segment (the default preset parameters of MAXVAL = 2^P - 1), no APPn.  Every restart
 * interval starts from the initial state with the line above it counted as zeros, and is led by RSTm, m = 0 .. 7 in turn.
 * A frame with a sample >= 2^P gets CCT_E_OVERFLOW in h_status[i] and size 0; the other frames are written and the call
 * returns the first non-OK status.  The call takes the encode slot, like the RLE codec.
 * cct_jpegls_bound(rows, cols, restart_rows): a sample costs at most LIMIT = 64 bits, runs included, and a line one bit
 * more; behind a 0xFF a byte carries 7 bits, so an interval of l lines takes at most ceil((64 l cols + l) / 7) + 2
 * bytes and 2 for its RST; headers and EOI stay below 34: 34 + intervals * (that + 2).  0 for a refused shape; out_stride
 * below it is CCT_E_CAP.  That is about 9.2 bytes a sample (2.4 MB for 512 x 512): size h_out for it, the files themselves
 * are a fraction of it and each is copied out at its own length.
 * cct_jpegls_info: (rows, cols, precision) of one file from its SOF55, after the whole marker walk; host only.
 * cct_jpegls_decode_batch: n files laid out back to back -> n*rows*cols uint16 (bits 16) or uint8 (bits 8) at `images`
 * (host or device), images_cap_px counted in pixels; a decode slot.  The host walks the markers and takes: any APPn / COM
 * segment; SOF55 with Nf = 1, P 2 .. 16 (<= bits), Y = rows, X = cols (anything else: CCT_E_MIXED); DRI of length 4, 5 or
 * 6, Ri in lines; an LSE segment of id 1 whose MAXVAL (<= 2^P - 1), T1 <= T2 <= T3 <= MAXVAL and RESET (3 ..
 * max(255, MAXVAL)) replace the defaults, 0 standing for the default; one SOS with Ns = 1, no mapping table, NEAR = 0,
 * ILV = 0, no point transform; bytes behind EOI.  CCT_E_JPEGLS, decided before upload: no SOI, SOF55, SOS or EOI, another SOF
 * type, Nf != 1, Y = 0, DNL, NEAR != 0, an interleave mode, a mapping table, a point transform, an LSE segment of id 2 .. 4
 * or with illegal values, a bad segment length, a marker other than RSTm or EOI inside the scan (0xFF and a byte >= 0x80).
 * CCT_E_STREAM: a wrong number or sequence of RST markers (the host sees that while it looks for them), and on the device
 * scan data that ends early or leaves whole bytes over, a run that passes the end of its line, a Golomb code longer than
 * LIMIT or with a value above 2^qbpp.  Refused files leave the others decoded, nothing is written outside a refused file's
 * own rows*cols slot, and the call returns the first non-OK status.
 * Whole-call errors, before the device is touched: CCT_E_ARG for rows or cols outside 1 .. 65535, rows*cols above 2^26,
 * n < 0, bits or src_bits other than 8 or 16, a precision outside 2 .. src_bits, restart_rows outside 0 .. 65535; CCT_E_CAP
 * as above.  cct_last_timings: [0] the three encode kernels, [4] the decode kernel, HIP events, summed over the passes. */
size_t cct_jpegls_bound(int rows, int cols, int restart_rows);
int cct_jpegls_encode_batch(const void *images, int images_on_device, int n, int rows, int cols, int src_bits /* 8 or 16 */,
                            int precision, int restart_rows, uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes,
                            uint32_t *h_status /* CCT_E_* per frame */);
int cct_jpegls_info(const uint8_t *h_file, size_t len, int *rows, int *cols, int *precision);
int cct_jpegls_decode_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int rows, int cols, int bits, void *images,
                            int images_on_device, size_t images_cap_px, uint32_t *h_status /* CCT_E_* per file */);

/* ---- JPEG 2000 Part-1 lossless codec (T.800; DICOM transfer syntax 1.2.840.10008.1.2.4.90) ----
 * cct_j2k_encode_batch: n rasters of shape (rows, cols), C order, uint16 (src_bits 16) or uint8 (src_bits 8), on the
 * host or (images_on_device) the device, -> n files at h_out + i*out_stride with their sizes in h_out_sizes[i]; every
 * stage runs on the device (level shift and reversible 5/3 transform, Tier-1, Tier-2).  The sample coded is value << shift
 * (shift 4 reproduces the 16-bit PNG preview) at `precision` bits, unsigned.  The file is fixed, so the output is
 * deterministic (tests/jpeg2000_model.py states it byte for byte): SOC, SIZ (Rsiz 0, one component, one tile), COD (no
 * SOP/EPH, maximal precincts, LRCP, one layer, `levels` decompositions, code-blocks of `codeblock` squared, style 0, 5/3),
 * QCD (no quantization, 2 guard bits), one SOT with Psot, SOD, levels + 1 packets with every coding pass of every
 * code-block, EOC; no COM.  jp2 != 0 puts the minimal JP2 container in front (signature, ftyp, jp2h with ihdr and an
 * enumerated greyscale colr, jp2c: 85 bytes); the default raw codestream is what DICOM encapsulates.
 * Per frame, h_status[i]: CCT_OK; CCT_E_OVERFLOW (a sample << shift >= 2^precision, or a coefficient that needs more
 * bit-planes than the guard bits allow) or CCT_E_CAP (a code-block's bytes beyond its slab, see cct_j2k_bound) with size 0;
 * the other frames are encoded, and the call returns the first status that is not CCT_OK.
 * cct_j2k_bound(rows, cols, levels, codeblock, jp2): a sufficient out_stride: 192 bytes of headers, 512 bytes of packet
 * header per packet and 32 per code-block (their worst case), and per code-block of w x h samples in a subband of mb
 * bit-planes at precision 16 (17 LL, 18 HL / LH, 19 HH) a slab of w h (mb + 2) / 4 + 64 bytes: two bits for every decision
 * of the arithmetic coder, about 5 bytes a sample where uniform noise takes 2.2.  0 for refused arguments.
 * cct_j2k_info: (rows, cols, precision) of a raw codestream or a JP2 file (the boxes are walked to jp2c) from its SIZ;
 * host only; CCT_E_J2K for anything else: no SOC + SIZ, a SIZ that leaves the file, more than one component, signed or
 * deeper than 16 bits, a JP2 without jp2c.
 * Whole-call errors of the encoder, before the device is touched: CCT_E_ARG for rows or cols outside 1 .. 65535, rows*cols
 * above 2^26, n < 0, src_bits other than 8 or 16, precision outside 2 .. 16 or above src_bits, shift outside 0 .. 15 or
 * precision - shift < 1, levels outside 0 .. 8, codeblock other than 32 or 64; CCT_E_CAP for out_stride below the bound. */
size_t cct_j2k_bound(int rows, int cols, int levels, int codeblock, int jp2);
int cct_j2k_encode_batch(const void *images, int images_on_device, int n, int rows, int cols, int src_bits /* 8 or 16 */, int precision,
                         int shift, int levels, int codeblock, int jp2, uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes,
                         uint32_t *h_status /* CCT_E_* per frame */);
int cct_j2k_info(const uint8_t *h_file, size_t len, int *rows, int *cols, int *precision);

/* ---- JPEG 2000 Part-1 lossless decoder ----
 * cct_j2k_decode_batch: n files laid out back to back -> n*rows*cols uint16 (bits 16) or uint8 (bits 8) at `images`
 * (host or device), images_cap_px counted in pixels; a decode slot; every stage on the device (packet parse, Tier-1, inverse
 * 5/3 transform, level shift) in passes of at most 512 MB of device memory.  The sample written is value >> shift, so a
 * file of cct_j2k_encode_batch at the same shift gives the raster back.  tests/jpeg2000_decode_model.py states the decoder.
 * The host walks the boxes and markers and takes a file of any encoder within these limits: a raw codestream or a JP2 file
 * (other boxes are skipped); SIZ with one unsigned component of 2 .. 16 bits, image and tile origins 0, one tile, subsampling
 * 1; one tile-part (TPsot 0, TNsot 0 or 1; Psot 0: to the end of the codestream); COD with maximal precincts, no SOP, no
 * EPH, any of the five progression orders, 1 .. 32 layers, no MCT, 0 .. 8 decomposition levels, code-blocks of 4 .. 64 by
 * 4 .. 64, code-block style 0, the reversible 5/3 transform; QCD without quantization, any guard bits and exponents as long as
 * no subband has more than 19 magnitude bit-planes (Mb = guard bits + exponent - 1; what the Tier-1 word holds: 16-bit data
 * with two guard bits reaches 19 in HH); COM, TLM, PLM, PLT and CRG in either header (skipped); bytes behind EOC, and a
 * missing EOC.  Y = rows, X = cols and a precision <= bits, or the file is CCT_E_MIXED.
 * CCT_E_J2K, decided before upload (scope, not damage: a caller may hand these to a host decoder): the 9/7 transform or
 * quantization style 1 or 2; user-defined precincts, SOP or EPH; a code-block style other than 0; COC, QCC, RGN, POC, PPM or
 * PPT; more than one tile, tile-part or component, a signed component, an origin, subsampling; more than 8 levels or 32
 * layers, a code-block side above 64; a marker segment whose length leaves the file, a marker this list does not name; COD
 * or QCD missing, a QCD with too few exponents for the levels, no SOT or SOD; a subband of more than 19 bit-planes.
 * CCT_E_STREAM, found on the device while it parses the packets: a packet header that runs past the end of the tile data,
 * code-block lengths that sum past it, more zero bit-planes than Mb, more coding passes for a code-block over the layers
 * than 3 (Mb - zero bit-planes) - 2, an Lblock above 32.  Damage inside the MQ-coded bytes cannot be detected by any decoder;
 * the result is defined: 0xFF is read beyond a code-block's last byte, coefficients and lifting are two's complement modulo
 * 2^32, the sample is clamped to 0 .. 2^precision - 1 after the level shift.  Refused files leave the others decoded,
 * nothing is written outside a refused file's own rows*cols slot, and the call returns the first non-OK status.
 * Whole-call errors, before the device is touched: CCT_E_ARG for rows or cols outside 1 .. 65535, rows*cols above 2^26,
 * n < 0, bits other than 8 or 16, shift outside 0 .. 15; CCT_E_CAP for images_cap_px below n*rows*cols.
 * cct_last_timings: [4] the decode kernels, HIP events, summed over the passes. */
int cct_j2k_decode_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int rows, int cols, int bits /* 8 or 16 */, int shift,
                         void *images, int images_on_device, size_t images_cap_px, uint32_t *h_status /* CCT_E_* per file */);

/* ---- strip-organised grayscale TIFF (TIFF 6.0; LZW, Deflate, horizontal predictor) ------------------------------------
 * tests/tiff_model.py states the layout, the LZW coder and decoder, the parser and its refusals; Pillow / libtiff is the oracle.
 *
 * cct_tiff_bound: bytes a file of cct_tiff_encode_batch takes at most (0: an argument it refuses, or a file that could pass
 * 4 GiB).  compression is the TIFF code: 1 none, 5 LZW, 8 Deflate.  rows_per_strip 0: strips of at most 64 KiB, one row at
 * least (Pillow's rule); else the height, clamped to rows. */
size_t cct_tiff_bound(int rows, int cols, int bits /* 8 or 16 */, int compression, int rows_per_strip);

/* cct_tiff_encode_batch: n rasters of rows x cols samples (uint8 / uint16, C order, host or device) -> little-endian TIFF
 * files, file i at h_out + i * out_stride (out_stride >= cct_tiff_bound), its size in h_out_sizes[i].  Layout, as libtiff
 * writes it: header, the strips back to back from offset 8, a zero byte if they end on an odd offset, the IFD (tags 256,
 * 257, 258, 259, 262, 273, 278, 279, 284, and 317 for predictor 2; no SamplesPerPixel), then StripByteCounts and
 * StripOffsets (inline for one strip; the byte counts of several strips are SHORT when a full strip has fewer than 6553
 * bytes -- 65536 uncompressed --, else LONG).  Strips hold little-endian samples, horizontal differences modulo 2^bits for
 * predictor 2 (the first sample of a row as it is).  LZW strips are libtiff's: greedy parse, codes MSB first, a Clear when the
 * next free entry is 4094, and its compression-ratio Clear; Deflate strips are zlib streams of `level` (4 .. 9, -1 = 6),
 * default strategy, memLevel 8, from the device DEFLATE pass.  With LZW, and with Deflate at level 6, the file is byte for
 * byte Pillow 12 / libtiff 4.7's.  Encode slot 0 (one call at a time).
 * CCT_E_ARG, before the device is touched: bits other than 8 or 16, rows or cols outside 1 .. 65535, n < 0, a compression
 * other than 1, 5, 8, a predictor other than 1, 2, predictor 2 with compression 1, rows_per_strip < 0, a level outside
 * -1, 4 .. 9 with compression 8 (ignored otherwise), a file that could pass 4 GiB; CCT_E_CAP for out_stride below the bound.
 * cct_last_timings: [0] the kernels of the call (staging, LZW or DEFLATE, layout), HIP events, summed over the passes. */
int cct_tiff_encode_batch(const void *images, int images_on_device, int n, int rows, int cols, int bits, int compression, int predictor,
                          int rows_per_strip, int level, uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes);

/* cct_tiff_info: (rows, cols, bits) of a file from its first IFD, after every structural check of cct_tiff_read_batch; host
 * only; CCT_E_TIFF for what the reader refuses, CCT_E_ARG for a null argument. */
int cct_tiff_info(const uint8_t *h_file, size_t len, int *rows, int *cols, int *bits);

/* cct_tiff_read_batch: n files laid out back to back (file i = h_files[h_offsets[i] .. h_offsets[i+1])) -> n rasters of
 * rows x cols samples of `bits` in `images` (host or device, images_cap_px samples), decoded on the device; h_status[i] is
 * CCT_OK or the file's code, and the call returns the first code that is not CCT_OK.  A decode slot (two calls at a time).
 * Taken: classic TIFF of either byte order, the first IFD, BitsPerSample 8 or 16 with one sample per pixel, SampleFormat
 * absent or 1, Photometric 1, PlanarConfiguration absent or 1, FillOrder absent or 1, strips of any RowsPerStrip (absent:
 * one strip) with a shorter last strip, StripOffsets and StripByteCounts as SHORT or LONG in any order in the file,
 * Compression 1, 5, 8 or 32946, Predictor absent, 1, or 2 with compression 5 and 8; dimensions as SHORT or LONG; tags this
 * list does not name are ignored.
 * CCT_E_TIFF, decided on the host before anything is uploaded (scope, not damage): no II / MM header, BigTIFF, an IFD or an
 * entry's values outside the file, tiles, any other compression, photometric, sample count, depth, sample format, fill
 * order or planar configuration, predictor 2 on uncompressed strips or a predictor above 2, a missing ImageWidth,
 * ImageLength, BitsPerSample, Photometric, StripOffsets or StripByteCounts, strip tables that do not hold
 * ceil(rows / RowsPerStrip) entries, a strip outside the file, rows, cols or bits other than the ones asked for.
 * A strip that does not yield its rows_in_strip * row_bytes bytes: CCT_E_STREAM for an LZW strip (found on the device), an
 * uncompressed strip with fewer bytes, a coded strip of none (both found on the host), and a Deflate strip that inflates to
 * another size; CCT_E_ZLIB for a Deflate strip the INFLATE kernel refuses (a strip is one whole zlib stream).
 * LZW strips are read by libtiff's rules: decoding stops once the strip's bytes are out and what follows is ignored, a last
 * string longer than what is left is cut, a missing EOI is no error, repeated Clears are allowed, a code equal to the next
 * free entry is the KwKwK case; errors are data or an EOI that ends the strip early, a first code after a Clear that is
 * not a literal, a code beyond the next free entry, more than 4862 codes without a Clear (libtiff's table is full), and --
 * stricter than libtiff -- a strip that does not open with a Clear.  A damaged strip never makes the decoder read outside
 * the strip's bytes or write outside its rows.  Refused files leave the others decoded; nothing is written outside a
 * refused file's own rows * cols slot, and nothing at all for a file refused on the host.
 * Whole-call errors, before the device is touched: CCT_E_ARG for rows or cols outside 1 .. 65535, n < 0, bits other than 8
 * or 16, offsets that decrease; CCT_E_CAP for images_cap_px below n * rows * cols.
 * cct_last_timings: [4] the kernels of the call (LZW decode, gather + INFLATE, predictor), HIP events, summed over the passes. */
int cct_tiff_read_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int rows, int cols, int bits /* 8 or 16 */,
                        void *images, int images_on_device, size_t images_cap_px, uint32_t *h_status /* CCT_E_* per file */);

/* ---- tuning / introspection (bench.py) --------------------------------------------- */
/* Stage times of the CALLING THREAD's most recent cct_encode_batch / cct_decode_batch, milliseconds (kept per
 * thread: an encode and a decode driven from two threads do not overwrite each other; takes no lock):
 * [0] encode kernel (HIP events on the library stream), [1] packed files device -> host, [2] DEFLATE (HIP events
 * on the device path, also after cct_zlib_compress_batch / _level / _strategy; host wall on the libz path), [3] INFLATE
 * (likewise), [4] decode kernel (HIP events),
 * [5] reserved.  After cct_png_read_batch: [3] INFLATE, [4] the unfilter kernel, [5] the unpack kernel (CRC check + IDAT
 * gather), HIP events, summed over the passes of the call. */
int cct_last_timings(float *out6);
/* Options.  cct_set_option refuses an unknown key and a read-only one with CCT_E_ARG ("unknown option <key>"); a value
 * outside a key's set is refused (CCT_E_ARG, the option keeps its value) or clamped, as stated per key:
 * "encode_slots" / "decode_slots": batches on the device at a time, clamped to 1 .. 2.
 * "device_deflate" / "device_inflate": 0 runs that stage on the host thread team, any other value is 1.
 * "zlib_threads": size of that team; below 1 is refused.
 * "png_unfilter_waves": waves per image of the PNG reader's unfilter kernel: 1, 2, 4 or 8, anything else is refused.
 * "inflate_lanes": lanes per stream of the INFLATE kernel: 256, 512, or 0 = 512 unless an encode call is in flight when
 * the decode starts; anything else is refused.  "last_inflate_lanes" (read only) reads back the choice.
 * "tile_path": 0, 1, 2 or 4 (kernel choice); 3 is refused, any other value is 1.  "stream_tpg": 1, 2 or 4, any
 * other value is 4.  "wg_threads": 256, 512 or 1024, anything else is refused.
 * "deflate_graph", "deflate_fork", "deflate_compact_records", "runtime_block_size" (tuning and cross-checks),
 * "decode_yields" / "queue_ahead" (scheduling of pipelined calls; 0 switches them off): 0, any other value is 1.
 * "last_encode_path", "last_decode_path" (read only): which kernel the last call ran.
 * None of these makes an output invalid.  The diagnostic switches that can exist in the tuning build only (csrc/tuning.h;
 * `make -C 2023-compact-image-compression_amd/csrc tuning`): this library has none to set. */
int cct_set_option(const char *key, int value);
int cct_get_option(const char *key, int *value);
/* A further tuning key, "tree_waves": waves per workgroup of the DEFLATE tree kernel, 1 or 16, or 0 = chosen per pass (16 where
 * a batch of 128 slices or more, at most one per CU, has blocks for no more 16-wave workgroups than the device has CUs;
 * DESIGN.md 5); anything else is refused.  The streams are the same at every value (tests/test_gpu_tree_placement.py). */

#ifdef __cplusplus
}
#endif
#endif /* COMPACT_HIP_H */
