// Internal declarations shared by the host side (api.cpp) and the HIP kernels.
// Not part of the C ABI (see include/compact_hip.h).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include <hip/hip_runtime.h>

#include "deflate_workspace.h"
#include "tuning.h"

namespace cct {

// ---- encode kernel geometry ----------------------------------------------------------
constexpr int ENC_CH = 8192;          // pixels per chunk staged in LDS (a multiple of every power-of-two block size; with any other
                                      // size a chunk is the ENC_CH / bs whole blocks that fit, CB * bs <= ENC_CH pixels)
constexpr int ENC_RING = 4;           // chunks resident in the LDS ring (power of two)
constexpr int ENC_LIST_CAP = 1536;    // difficult-block records kept in LDS; the rest spill to HBM
// Token staging for one chunk + carry: two bytes per pixel token, one jump byte per meshed pair, carry and EOF in the 64.
// The jump term: a pair takes two blocks, so a chunk of CB = ENC_CH / bs blocks leads at most CB / 2 pairs, <= ENC_CH / 8
// for bs >= 4.  At bs 3 (CB / 2 = 1365) only block 0 can mesh: a block is difficult when 2 * chg >= 3, so chg = 2 (of at
// most 2 changes), its cur = chg + enter <= 3, and a candidate fits when up + 1 < cur - 2 <= 1, which no up >= 0 meets;
// block 0 is the exception (Q4: every candidate fits), so a bs-3 slice has at most one jump byte.  (Pairs that lead from the
// last 63 blocks of a chunk into the next one add their partners' tokens to this chunk; that slack runs into l_mask, which
// pass 2 of encode_kernel no longer reads.)
constexpr int ENC_STG_BYTES = 2 * ENC_CH + ENC_CH / 8 + 64;
constexpr int ENC_MAX_LDS_ROLE = 48 * 1024;  // role[] lives in LDS when NB <= this

constexpr uint8_t ROLE_PARTNER = 0xFF; // block consumed as the second half of a meshed pair

struct EncArgs {
	const uint16_t *images;   // n * N pixels
	const int32_t *lut;       // traversal order O[N] (device) or nullptr for the identity
	int N, NB;
	int eof;                  // -1: none
	uint32_t flags;           // CCT_FLAG_*
	uint8_t *payload; size_t stride;
	uint32_t *sizes; uint32_t *status;
	uint8_t *ws_role;         // n * NB bytes when role[] does not fit LDS, else nullptr
	uint32_t *ws_lidx;        // n * NB spill: difficult-block index
	uint64_t *ws_lmask;       // n * NB spill: candidate masks
	uint8_t *ws_lcur;         // n * NB spill: cur counts
	uint32_t *stats;          // optional n * 4: short, full, jump tokens, difficult blocks
	uint8_t *roles_out;       // optional n * NB: final role of every block (BLOCK_JUMPS)
	uint32_t dbg_skip;        // tuning build only (tuning.h, option "debug_skip"): phases to skip, results then invalid; 0 in a release build
	int bs;                   // block size, set by launch_encode, read by encode_kernel<0> (run-time block size) only; fills the tail
	                          // padding, so the struct keeps its size and the other kernels their argument layout
};
static_assert(sizeof(EncArgs) == 120, "EncArgs layout: bs must stay in the tail padding");

// tile-staged fast path (block_size 16, traversal made of aligned 64x64 tiles)
constexpr int TILE_MAX_TILES = 1024;
constexpr int TILE_MAX_ORIENT = 4;
struct TileEncArgs {
	EncArgs e;
	const uint32_t *tile_org;    // n_tiles: raster index of each tile's top-left pixel
	const uint8_t *tile_orient;  // n_tiles: which pattern table the tile uses
	const uint16_t *patterns;    // n_orient * 4096: LDS byte offset of every traversal position of a tile
	int n_orient, n_tiles, row_pitch;
};
size_t enc_tiles_lds_bytes(int NB, bool *role_in_lds);
hipError_t launch_encode_tiles(const TileEncArgs &ta, int n, hipStream_t s);

// single streaming pass (encode_stream.hip): one kernel, every pixel read once.  block_size 16, a traversal made of at most 256
// aligned 64x64 tiles with the block structure build_stream_tables (api.cpp) checks
constexpr int STREAM_MAX_NB = 65536;        // blocks per slice
constexpr int STREAM_PAIR_REC = 80;         // bytes per meshed-pair record: jump byte + up to 64 token bytes, padded to 16
constexpr uint32_t CCT_ST_INTERNAL = 0x80000000u;  // the kernels disagree about a size: a bug, never a data property
struct StreamTiles {           // small per-shape tables carried IN the kernel arguments: one scalar load, no pointer to chase
	uint32_t orgo[256];          // raster index of each tile's top-left pixel (< 2^24) | tile orientation << 24: ONE scalar load gives
	                             // both (a byte array indexed by the tile became a vector load the next table lookup had to wait for)
	uint32_t last[TILE_MAX_ORIENT];  // raster offset inside the tile of the tile's last traversal position
	uint32_t qorg[TILE_MAX_ORIENT];  // raster offset inside the tile of the 32x32-pixel quadrant its first 64 traversal blocks cover
};
constexpr int STREAM_TPG = 4;       // default tiles per group = waves per workgroup (1, 2 or 4: option "stream_tpg")
struct StreamArgs {
	EncArgs e;
	StreamTiles tiles;
	const uint32_t *ptab;        // n_orient * 128 entries of 4 dwords, one per block pair of a tile (entry = block row * 8 + block pair):
	                             //   [0] traversal block index | orientation << 8 of the left block, the same << 16 for the right block
	                             //   [1], [2] raster offset inside the tile of the pixel that precedes the left / right block in
	                             //   traversal order (0xFFFFFFFF: the block opens the tile)
	const uint32_t *htab;        // n_orient * 32 entries of 2 dwords: the 32 block pairs (8 rows x 4) of the quadrant a tile's first 64
	                             //   traversal blocks cover (origin: tiles.qorg): [0] as ptab[0], [1] raster offset of the pair inside the tile
	const uint32_t *otab;        // 4 * 16 dwords per block orientation: eight v_perm selectors, quadrant choice bits
	const uint32_t *ttab;        // 16 * 4 dwords: token byte selectors and length for the 16 two-byte masks of a 4-pixel group, kept
	                             //   bits of the low bytes
	int n_tiles, row_pitch, gps, tpg; // gps: groups per slice, tpg: tiles per group
	int dbg;                     // tuning build only (tuning.h, CCT_STREAM_DBG): 1 no carry wait, 2 no look-back (results then invalid), 4 wrong group guess (results valid); 0 in a release build
	uint64_t *hand;              // n * gps * 4 hand-off words, then
	uint32_t *ticket;            // n group tickets (one allocation: zeroed by one memset before every launch)
	uint64_t *spill_mask;        // n * NB: candidate masks beyond the LDS list of a tile
	uint16_t *spill_idx;         // n * NB: their blocks
	uint8_t *pairrec;            // n * (NB / 2) * STREAM_PAIR_REC: meshed pairs beyond one per lane
};
inline size_t stream_ws_bytes(int n, int gps) { return ((size_t)n * gps * 32 + (size_t)n * 4 + 15) & ~(size_t)15; }
hipError_t launch_encode_stream(const StreamArgs &sa, int n, hipStream_t s);

size_t enc_lds_bytes(int NB, bool *role_in_lds);
// Block sizes 4, 8, 16, 32 and 64 have kernels compiled for them; every other size from 3 to 64 runs the run-time block size
// kernels (encode_kernel<0>, decode_kernel<0>), which `force` (option "runtime_block_size") selects for every size.
inline bool bs_run_time(int bs, bool force) { return force || (bs & (bs - 1)) != 0; }

// run_time: encode_kernel<0> (launch_encode sets a.bs) even for a power of two (see bs_run_time)
hipError_t launch_encode(const EncArgs &a, int n, int block_size, int threads, hipStream_t s, bool run_time);

// ---- decode kernel geometry ----------------------------------------------------------
constexpr int DEC_SEG = 16;           // payload bytes parsed per lane per step
constexpr int DEC_JLIST_CAP = 2048;   // jump records kept in LDS; the rest spill to HBM
constexpr int DEC_BLK_ORDERS = 8;     // block path: distinct visiting orders of a 4x4 block that a shape may have
// words of the block tables of a shape with n_orient tile patterns (api.cpp build_block_tables)
constexpr size_t dec_block_words(int n_orient) { return (size_t)n_orient * 256 + DEC_BLK_ORDERS * 2 + DEC_BLK_ORDERS * 8; }
// block path: pass B stages a step's pixel values by ordinal, 16 to a stream slot, before it places them; a slot takes 18
// entries (9 words, an odd count: lanes that work on neighbouring slots use different LDS banks)
constexpr int DEC_STAGE_PITCH = 18;

struct DecArgs {
	const uint8_t *payload; size_t stride; const uint32_t *sizes;
	const int32_t *lut;       // traversal order or nullptr
	int N, NB;
	uint16_t *images; uint32_t *status;
	uint8_t *ws_role;         // n * NB bytes (always in HBM for decode)
	uint32_t *ws_slot;        // n * NB: stream slot -> leader block | kind << 30
	uint32_t *ws_jord;        // n * (NB/2+1) spill: jump ordinals
	uint8_t *ws_jval;         // n * (NB/2+1) spill: jump distances
	// traversal made of aligned 64x64 tiles of 4x4 blocks (tile tables as encode_tiles_kernel's, block tables from
	// build_block_tables): block -> raster rows from LDS
	const uint32_t *tile_org; const uint8_t *tile_orient; const uint32_t *blk_tab;
	int n_tiles, n_orient, width;   // n_tiles == 0: use lut
	uint32_t bs_mul;                // decode_kernel<0> only: ord / bs == __umulhi(ord, bs_mul) >> bs_shift (bs_divider)
	// pass A leaves every lane's view of every parsing step here (pixel ordinal | entry state << 31, value before the
	// segment) so that pass B does not repeat the workgroup scans: n * pcache_steps * threads entries
	uint2 *ws_pcache; int pcache_steps;
	uint16_t bs, bs_shift;          // decode_kernel<0> only (set by launch_decode): the block size and the shift of its divider
	int narrow_stores;              // block path: `images` is not 8-byte aligned, so pixels are stored one by one
};
static_assert(sizeof(DecArgs) == 152, "DecArgs layout");

// Division by a run-time block size d, 3 <= d <= 64, as a multiply-high and a shift: with s = floor(log2(d - 1)) and
// m = ceil(2^(32+s) / d) < 2^32, floor(x * m / 2^(32+s)) == floor(x / d) for every x < 2^31.  (m * d = 2^(32+s) + e with
// 0 <= e < d <= 2^(s+1); the product overshoots x / d by x * e / (d * 2^(32+s)) < 1 / d, less than the distance of x / d to
// the next integer.)  check_shape limits slices to 2^30 pixels.  Mirrored by tests/test_block_size_golden.py.
inline void bs_divider(int d, uint32_t *mul, uint32_t *shift)
{
	uint32_t s = 0;
	while ((2u << s) <= (uint32_t)(d - 1)) s++;
	*shift = s;
	*mul = (uint32_t)((((uint64_t)1 << (32 + s)) + (uint64_t)d - 1) / (uint64_t)d);
}

// run_time: decode_kernel<0> (launch_decode sets a.bs, a.bs_mul, a.bs_shift) even for a power of two (see bs_run_time)
// *block_path: the launch took decode_kernel<16, true, true>
hipError_t launch_decode(const DecArgs &a, int n, int block_size, int threads, hipStream_t s, bool run_time, bool *block_path);

// ---- device DEFLATE (zlib 1.2.11 level 9 restatement, deflate_kernels.hip) ----------------
// BlockMeta, BlockTables, DeflateArgs, the shared constants and the workspace layout: deflate_workspace.h
// a level's fields of DeflateArgs (deflate_kernels.hip); false for levels outside 4 .. 9
bool deflate_level_args(int level, DeflateArgs &a);
// a memLevel's fields of DeflateArgs; false for anything but 8 and 9
bool deflate_mem_level_args(int mem_level, DeflateArgs &a);
// the fields of a (level, strategy) pair: levels 4 .. 9 with strategies 0, 1 and 4 (deflate_slow), levels 1 .. 9 with 2
// and 3 (deflate_huff / deflate_rle, which read no level table); false for anything else
bool deflate_strategy_args(int level, int strategy, DeflateArgs &a);
hipError_t deflate_init_tables();
hipError_t launch_pack(const uint8_t *src, size_t stride, const uint32_t *sizes, int n, uint64_t *offsets, uint8_t *dst,
                       int exact, hipStream_t st);
hipError_t launch_deflate(const DeflateArgs &a, int n, hipStream_t st, hipStream_t side = nullptr,
                          const hipEvent_t *fork_join_events = nullptr);  // side + four events (no timing): independent kernels side by side

// ---- PNG writer (png_kernels.hip) -----------------------------------------------------------------
// n rasters (rows x cols uint16, C order) -> filter byte + filtered big-endian row, rows * (1 + 2 cols) bytes at d_out + i*out_stride
hipError_t launch_png_filter(const uint16_t *d_img, int n, int rows, int cols, int shift, uint8_t *d_out, size_t out_stride,
                             hipStream_t st);
// 8-bit samples: n rasters (rows x cols, uint16 mapped through the window [lo, hi] to 0 .. 255 when src_bits is 16, uint8 with
// the window (0, 255) when it is 8) -> filter byte + filtered row, rows * (1 + cols) bytes at d_out + i*out_stride
hipError_t launch_png_filter8(const void *d_img, int src_bits, int n, int rows, int cols, int lo, int hi, uint8_t *d_out,
                              size_t out_stride, hipStream_t st);
struct PngPackArgs {
	const uint8_t *src; size_t src_stride; uint32_t src_skip;  // zlib stream i = src + i*src_stride + src_skip ..
	const uint32_t *src_sizes;                                 // .. of src_sizes[i] - src_skip bytes (device)
	uint32_t chunk;                                            // IDAT data bytes per chunk: max(65536, 4 cols)
	uint8_t ihdr[25];                                          // IHDR chunk: length, type, data, CRC
	uint8_t *out; size_t out_stride; uint32_t *out_sizes;      // PNG files (device)
};
// grid: max_chunks >= the IDAT chunks of the longest stream
hipError_t launch_png_pack(const PngPackArgs &a, int n, uint32_t max_chunks, hipStream_t st);

// ---- PNG reader (png_read_kernels.hip) ------------------------------------------------------------
// One chunk of one file, as the host's walk over the chunk heads found it (api.cpp png_walk_file).  The bounds argument: the
// device kernels derive every address they touch from this table and from the caller's (rows, cols), never from file content.
// The walk reads a chunk's length only after it has checked that the 8-byte head lies inside the file, and enters the chunk
// only after it has checked length <= file size - position - 12, so [src, src + 4 + len + 4) -- type, data, CRC -- lies inside
// the file and with it inside the uploaded archive.  dst is the running sum of the IDAT lengths entered before it, for the
// batch, so [dst, dst + len) lies inside the gathered buffer, which is allocated for the final sum (plus the INFLATE kernel's
// read-ahead padding), and inside [offsets[file], offsets[file + 1]), the stream the INFLATE kernel is given for that file.
// png_unpack_kernel reads and writes nothing else.  The INFLATE kernel bounds its output by its stride.
// png_unfilter_kernel touches the file's rows_stride bytes of inflated rows and its rows * cols samples of the output, both
// indexed by (row < rows, column < cols) alone; a file is unfiltered only if its stream inflated to exactly
// rows * (1 + cols * bpp) bytes, so every byte it reads was written by this call.  A filter byte selects one of five
// formulas; a value above 4 sets a status bit.
struct PngChunk {
	uint64_t src;   // offset of the chunk's type field in the uploaded files
	uint64_t dst;   // IDAT: offset of its data in the gathered zlib streams
	uint32_t len;   // data bytes (<= 2^31 - 1)
	uint32_t file;  // index of the file in the pass | PNG_CHUNK_IDAT
};
constexpr uint32_t PNG_CHUNK_IDAT = 1u << 31;
// per-file status word of a pass (device): CRC and FILTER are set by the kernels, SKIP by the host for a file its walk refused
constexpr uint32_t PNG_ST_CRC = 1u, PNG_ST_FILTER = 2u, PNG_ST_SKIP = 4u;
struct PngUnpackArgs {
	const uint8_t *files;     // the pass's files as uploaded
	const PngChunk *chunks;
	uint8_t *streams;         // gathered zlib streams
	uint32_t *status;
};
hipError_t launch_png_unpack(const PngUnpackArgs &a, uint32_t n_chunks, hipStream_t st);
struct PngUnfilterArgs {
	uint8_t *rows; size_t rows_stride;              // inflated rows of file i at rows + i * rows_stride; the kernel writes the last row of a band back
	const uint32_t *row_sizes, *zstatus;            // the INFLATE kernel's out_sizes and status
	uint32_t *status;
	const uint8_t *bpp;                             // bytes per sample of every file: 1 or 2
	int nrows, cols, shift;
	uint16_t *images;                               // n * nrows * cols
};
constexpr int PNG_UNFILTER_WAVES = 8;  // waves per image (option "png_unfilter_waves": 1, 2, 4, 8)
hipError_t launch_png_unfilter(const PngUnfilterArgs &a, int n, int waves, hipStream_t st);

// ---- gate between the decode and the encode stream (sched_kernels.hip) ---------------------------
hipError_t launch_gate_bump(uint32_t *word, hipStream_t st);
hipError_t launch_gate_wait(const uint32_t *gate, uint32_t want_pass, uint32_t grace_us, uint32_t timeout_us, hipStream_t st);

// ---- device INFLATE (inflate_kernels.hip) ----------------------------------------------------
struct InflateArgs {
	const uint8_t *in; uint64_t in_total;   // archive bytes on the device (padded to 16), total size
	const uint64_t *offsets; int skip;      // stream i = in[offsets[i] + skip .. offsets[i+1])
	uint8_t *out; size_t out_stride;        // inflated payloads
	uint32_t *out_sizes, *status;           // status: CCT_ST_ZLIB / CCT_ST_STREAM bits
};
// lanes: 256 or 512 per stream (512: faster alone, slower next to an encode batch; inflate_kernels.hip)
hipError_t launch_inflate(const InflateArgs &a, int n, hipStream_t st, int lanes);

// ---- PackBits utility (packbits_kernels.hip) -------------------------------------------------
hipError_t launch_packbits_encode(const uint8_t *d_in, const uint64_t *d_offsets, int n, int delta, uint32_t *d_ws, uint8_t *d_out,
                                  size_t out_stride, uint32_t *d_out_sizes, hipStream_t st);
hipError_t launch_packbits_decode(const uint8_t *d_in, const uint64_t *d_offsets, int n, int delta, uint8_t *d_out, size_t out_stride,
                                  uint32_t *d_out_sizes, uint32_t *d_status, hipStream_t st);

// ---- DICOM RLE Lossless (dicom_rle_kernels.hip) -----------------------------------------------
// Encode: n rasters of rows x cols samples of `planes` bytes (1: uint8, 2: uint16) -> frame i at out + i * out_stride
// (out_stride a multiple of 4, >= 64 + planes * 2 * rows * cols), its size in out_sizes[i].  rowinfo holds
// n * planes * rows words: the size pass leaves each coded row's length there, the scan turns it into the row's offset in
// the frame, the write pass reads it.  Every store of the write pass lies in [offset, offset + length) of its row.
hipError_t launch_dicom_rle_encode(const void *d_images, int n, int rows, int cols, int planes, uint32_t *d_rowinfo, uint8_t *d_out,
                                   size_t out_stride, uint32_t *d_out_sizes, hipStream_t st);
// Decode: the host has parsed the frame headers; what reaches the device is a list of segments.  A segment is cut into
// tiles of RLE_TILE coded bytes (its tiles are tile0 .. tile0 + ceil(len / RLE_TILE) - 1 of the pass, tile0 increasing
// with the segment index).  A packet is at most 129 bytes long, so the first packet head of a tile lies at one of
// RLE_ENTRIES offsets.
constexpr uint32_t RLE_TILE = 2048, RLE_ENTRIES = 129;
struct RleSegment {
	uint64_t src;    // offset of the segment in the uploaded frames
	uint64_t dst;    // byte offset in `images` of the first sample's byte this segment fills
	uint32_t len;    // coded bytes (>= 1)
	uint32_t tile0;
};
struct RleDecodeArgs {
	const uint8_t *frames;       // uploaded frames; readable for 16 bytes past the last one
	const RleSegment *segs;
	uint32_t nseg, ntiles;
	uint32_t want;               // rows * cols: bytes every segment has to yield
	uint32_t step;               // bytes per sample in `images`: decoded byte k lands at dst + k * step
	uint32_t *table;             // ntiles * RLE_ENTRIES words: (exit offset | bytes produced << 12) per entry offset
	uint2 *tinfo;                // ntiles: the tile's true entry offset and the output index it starts at (clipped to want)
	uint32_t *short_seg;         // nseg: 1 for a segment that yields fewer than `want` bytes
	uint8_t *images;
};
hipError_t launch_dicom_rle_decode(const RleDecodeArgs &a, hipStream_t st);

// ---- TIFF strips: predictor, LZW, file layout (tiff_kernels.hip) ---------------------------------
// LZW numbering (TIFF 6.0 section 13, as libtiff writes it): after a Clear the codes, Clear and EOI included, are counted from
// 1; code j has 9 bits for j <= 254, 10 for j <= 766, 11 for j <= 1790 and 12 beyond, and code j >= 2 defines table entry
// 256 + j.  An encoder writes its Clear as code 3837; a decoder follows a stream that does not up to code TIFF_LZW_MAX_J,
// where libtiff's table (5119 entries) is full.
constexpr uint32_t TIFF_LZW_SLOTS = 8192;   // encoder: dictionary slots in LDS (3836 entries at most: load below 47 %)
constexpr uint32_t TIFF_LZW_TAB = 3904;     // decoder: codes whose (length, destination) are kept: entry 4095 is code 3839
constexpr uint32_t TIFF_LZW_MAX_J = 4862;   // code 4862 defines entry 5118, the last of libtiff's table
// bytes an LZW strip of L bytes takes at most: 12 bits a byte, a Clear per 3836 codes, the opening Clear, EOI, the fill,
// rounded up to the words the encoder stores
inline size_t tiff_lzw_bound(size_t L) { return ((L + L / 3836 + 4) * 3 / 2 + 8 + 3) & ~(size_t)3; }
// Encode staging: raster i, rows [s * rps, ..) -> strip (i * spf + s) at strips + that * strip_stride as little-endian
// samples, horizontal differences when predictor is 2; its byte count in strip_sizes
hipError_t launch_tiff_stage(const void *d_images, int n, int rows, int cols, int bps, int predictor, int rps, int spf, uint8_t *d_strips,
                             size_t strip_stride, uint32_t *d_strip_sizes, hipStream_t st);
// one wave per strip: strip k of in_sizes[k] bytes -> LZW stream at out + k * out_stride (>= tiff_lzw_bound, a multiple of 4)
hipError_t launch_tiff_lzw_encode(const uint8_t *d_strips, size_t strip_stride, const uint32_t *d_in_sizes, int nstrips, uint8_t *d_out,
                                  size_t out_stride, uint32_t *d_out_sizes, hipStream_t st);
struct TiffPackArgs {
	const uint8_t *src; size_t src_stride; uint32_t src_skip;  // coded strip k = src + k * src_stride + src_skip ..
	const uint32_t *src_sizes;                                 // .. of src_sizes[k] - src_skip bytes
	uint32_t spf, rows, cols, bits, compression, predictor, rps;
	uint32_t *strip_off;                                       // n * spf words: where each strip starts in its file
	uint8_t *out; size_t out_stride; uint32_t *out_sizes;      // the files
};
// header, strips from offset 8, pad byte, IFD, StripByteCounts, StripOffsets: the layout of tests/tiff_model.py write_file
hipError_t launch_tiff_pack(const TiffPackArgs &a, int n, hipStream_t st);
// Read side.  The host has parsed every IFD (api_tiff.cpp); the device gets a list of strips whose [src, src + len) lies inside
// the uploaded files and whose [dst, dst + want) lies inside the decoded-strip buffer, by the host's checks.
struct TiffStrip {
	uint64_t src;    // offset of the coded strip in the uploaded files
	uint64_t dst;    // offset of its rows in the decoded-strip buffer
	uint32_t len;    // coded bytes
	uint32_t want;   // rows_in_strip * row_bytes
	uint32_t file;   // file of the pass
	uint32_t row0;   // its first row
	uint32_t nrows;
	uint32_t flags;  // TIFF_F_*
};
constexpr uint32_t TIFF_F_BIG_ENDIAN = 1u, TIFF_F_PREDICTOR = 2u, TIFF_F_FROM_FILE = 4u;  // FROM_FILE: uncompressed, the rows are at src
// dst[offsets[k] ..] = files[src .. src + len) of strip k: Deflate strips back to back, as the INFLATE kernel takes them
hipError_t launch_tiff_gather(const uint8_t *d_files, const TiffStrip *d_strips, uint32_t nstrips, const uint64_t *d_offsets, uint8_t *d_dst,
                              hipStream_t st);
// one wave per strip; status[k] = 1 for a strip that does not yield `want` bytes.  Nothing outside [dst, dst + want) is written.
hipError_t launch_tiff_lzw_decode(const uint8_t *d_files, const TiffStrip *d_strips, uint32_t nstrips, uint8_t *d_decoded,
                                  uint32_t *d_status, hipStream_t st);
// rows of every strip (at dst of the decoded strips, or at src of the files) -> raster: byte swap for big-endian files,
// inclusive sum along the row modulo 2^bits for predictor 2
hipError_t launch_tiff_unpredict(const uint8_t *d_files, const uint8_t *d_decoded, const TiffStrip *d_strips, uint32_t nstrips, int rows,
                                 int cols, int bps, void *d_images, hipStream_t st);

// ---- JPEG Lossless, SOF3 (jpeg_lossless_kernels.hip) --------------------------------------------
constexpr uint32_t JPL_HDR_MAX = 72;     // SOI 2, SOF3 13, DHT 4 + 1 + 16 + 17, DRI 6, SOS 10 = 69 bytes at most, rounded up
constexpr uint32_t JPL_CHUNK = 1024;     // samples per step of the emit kernel: 4 per lane
constexpr uint32_t JPL_SUB = 1024;       // bits per subsequence of the Huffman decoder (a coded sample has 31 at most)
constexpr uint32_t JPL_ST_OVERFLOW = 1u; // encode: a sample >= 2^precision
constexpr uint32_t JPL_ST_STREAM = 1u;   // decode: RST sequence, a code outside the table, data that ends early or is left over
constexpr uint32_t JPL_ST_INTERVALS = 2u; // decode, set by jpl_unstuff_kernel only: the frame's interval starts are not valid, nothing of it is decoded
struct JplCode {             // one frame's Huffman table as its DHT states it, and the code of every category (size 0: none)
	uint8_t bits[16], huffval[17], nval;
	uint8_t size[17];
	uint16_t code[17];
};
// Encode.  Interval k of a frame holds rows [k * rpi, min(rows, (k + 1) * rpi)); n_int = ceil(rows / rpi).  bitbuf gives every
// sample one word: interval k's unstuffed bytes start at word k * rpi * cols, 31 bits a sample fit.  The bytes of word w
// are taken from its top down.  out_stride >= jpl_bound(): the layout kernel derives every offset from ibytes + iff, which
// count bytes that exist in bitbuf, so no store leaves [0, bound).
// predictor 1 .. 7 is the selection value of every frame and ncand is 1.  predictor 0 lets every frame take the cheapest of
// the seven: ncand is 7, candidate k (selection value k + 1) of frame f has its histogram at hist[(f * 7 + k) * 17] and its
// table at codes[f * 7 + k]; the pick kernel copies the winner's table over candidate 0.  Either way the frame's table is
// codes[f * ncand] and its selection value sel[f] from the table / pick kernel on.
constexpr uint32_t JPL_NCAND = 7;
struct JplEncArgs {
	const void *images;        // n * rows * cols samples of src_bits (8 or 16)
	uint32_t src_bits, n, rows, cols, precision, rpi, n_int, restart;  // restart: a DRI segment and RST markers are written
	uint32_t predictor, ncand; // 1 .. 7 and 1, or 0 and JPL_NCAND
	uint32_t *hist;            // n * ncand * 17, zero on entry
	uint32_t *status;          // n, zero on entry: JPL_ST_OVERFLOW
	uint32_t *sel;             // n: the selection value written into the frame's SOS
	JplCode *codes;            // n * ncand
	uint32_t *bitbuf;          // n * rows * cols words
	uint32_t *ibytes, *iff;    // n * n_int: unstuffed bytes of an interval, and how many of them are 0xFF
	uint32_t *ioff;            // n * n_int: offset in the file of the interval's first byte
	uint8_t *out; size_t out_stride; uint32_t *out_sizes;  // a frame with a status gets size 0
};
hipError_t launch_jpl_encode(const JplEncArgs &a, hipStream_t st);
// Decode.  The host has walked the markers (api_jpeg_lossless.cpp); a frame reaches the device as the byte range of its
// entropy-coded segment, its decoding table and its scan parameters.
struct JplFrame {
	uint64_t src;              // offset of the entropy-coded segment in the upload; the unstuffed bytes go to the same offset of ubuf
	uint32_t len;              // its bytes, RST markers included; the two bytes behind it (the next marker) are readable
	uint32_t slot;             // the raster this frame fills: images + slot * rows * cols
	uint32_t ss, pt, init;     // predictor, point transform, 2^(P - Pt - 1)
	uint32_t rpi, n_int;       // rows per interval, intervals
	uint32_t int0;             // index of its interval 0 among the pass's intervals; its n_int + 1 interval starts sit at istart[int0 + frame index ..]
	uint32_t sub0;             // its first entry of the subsequence tables
	int32_t maxcode[17];       // [l]: the largest code of length l, -1 where there is none
	int32_t delta[17];         // [l]: index into huffval of the first code of length l, minus that code
	uint8_t huffval[20];
};
struct JplDecArgs {
	const uint8_t *files;      // the upload
	const JplFrame *frames; uint32_t nframes;
	const uint32_t *int_frame; uint32_t total_int;  // frame index of every interval of the pass
	uint32_t rows, cols, out_bits;                  // out_bits 8 or 16: the sample type of images
	uint8_t *ubuf;             // unstuffed entropy-coded bytes
	uint32_t *istart;          // total_int + nframes: byte offset of every interval inside its frame's unstuffed data, and the end
	uint32_t *sub_start, *sub_land, *sub_cnt;       // per subsequence: entry bit, landing bit, samples that start inside
	uint16_t *diff;            // nslots * rows * cols: the differences, modulo 2^16
	uint32_t *status;          // nframes, zero on entry: JPL_ST_STREAM
	void *images;
	uint32_t any_generic;      // some frame has a predictor other than 1
};
hipError_t launch_jpl_decode(const JplDecArgs &a, hipStream_t st);

// ---- JPEG-LS lossless, SOF55 (jpeg_ls_kernels.hip) ---------------------------------------------------
constexpr uint32_t JLS_HDR_MAX = 32;      // SOI 2, SOF55 13, DRI 6, SOS 10 = 31 bytes at most, rounded up
constexpr uint32_t JLS_LIMIT_MAX = 64;    // LIMIT = 2 * (bpp + max(8, bpp)) at bpp = 16: the longest code
constexpr uint32_t JLS_STEP_WORDS = 260;  // LDS words of the encoder's bit buffer: a carry below a byte and 64 lanes of up to 128 bits, 257 words, and the two a put may touch behind
constexpr uint32_t JLS_DEC_LANES = 8;     // intervals per workgroup of the decoder: a context table of 367 * 12 bytes each in LDS
constexpr uint32_t JLS_ST_OVERFLOW = 1u;  // encode: a sample >= 2^precision
constexpr uint32_t JLS_ST_BOUND = 2u;     // encode: an interval or a file would leave its bound (a defect of the bound, never seen)
constexpr uint32_t JLS_ST_STREAM = 1u;    // decode: data that ends early or is left over, a run past the line end, a value outside the range
// The bytes of a restart interval of `lines` lines, at most.  A sample in regular mode costs LIMIT bits at most.  A run of L
// samples and its interruption sample cost at most L ones, a zero, J bits and LIMIT - J - 1 bits: LIMIT + L for L + 1 samples.
// A run to the end of a line costs L + 1 bits for L samples.  LIMIT >= 20 > 2, so LIMIT bits a sample cover every case and one
// bit a line is spare.  Behind a 0xFF a byte carries 7 bits: ceil(bits / 7) bytes, and one 0x00 if the last byte is 0xFF.
inline size_t jls_interval_bound(size_t lines, size_t cols) { return (JLS_LIMIT_MAX * lines * cols + lines + 6) / 7 + 2; }
struct JlsParams {  // T.87 C.2.4.1.1: the defaults of a precision (api_jpeg_ls.cpp jls_params), or what an LSE segment of id 1 states
	uint32_t maxval, range, qbpp, limit, a0, reset;
	int32_t t1, t2, t3;
};
// Encode.  Interval k of a frame holds lines [k * rpi, min(rows, (k + 1) * rpi)); n_int = ceil(rows / rpi).  Its stuffed bytes go
// to stage + (frame * n_int + k) * istride, istride >= jls_interval_bound(rpi, cols); every store there is checked against
// istride, and the layout kernel checks the sum against out_stride.
struct JlsEncArgs {
	const void *images;        // n * rows * cols samples of src_bits (8 or 16)
	uint32_t src_bits, n, rows, cols, precision, rpi, n_int, restart;  // restart: Ri of the DRI segment, in lines; 0: none is written
	JlsParams par;
	uint32_t *status;          // n, zero on entry: JLS_ST_OVERFLOW, JLS_ST_BOUND
	uint8_t *stage; size_t istride;
	uint32_t *ibytes;          // n * n_int: bytes of an interval
	uint32_t *ioff;            // n * n_int: offset in the file of the interval's first byte
	uint8_t *out; size_t out_stride; uint32_t *out_sizes;  // a frame with a status gets size 0
};
hipError_t launch_jls_encode(const JlsEncArgs &a, hipStream_t st);
// Decode.  The host has walked the headers and found the markers of the scan (api_jpeg_ls.cpp): the device gets every interval
// as a byte range [src, src + len) of the upload that holds no marker, and the lines it fills.
struct JlsFrame { uint32_t slot; JlsParams par; };  // slot: the raster this frame fills, images + slot * rows * cols
struct JlsInterval { uint64_t src; uint32_t len, frame, row0, nrows; };
struct JlsDecArgs {
	const uint8_t *files;      // the upload
	const JlsFrame *frames; uint32_t nframes;
	const JlsInterval *intervals; uint32_t total_int;
	uint32_t rows, cols, out_bits;  // out_bits 8 or 16: the sample type of images
	uint32_t *status;          // nframes, zero on entry: JLS_ST_STREAM
	void *images;
};
hipError_t launch_jls_decode(const JlsDecArgs &a, hipStream_t st);

// ---- JPEG 2000 Part-1: what the layouts of the encoder and the decoder share -----------------------
// The coefficients of all subbands share one rows x cols int32 plane in the Mallat arrangement (after a stage the LL band is
// the top left corner), every code-block is a rectangle of it, the subbands are listed in packet order.  Device side: jpeg2000_device.h.
struct J2kSizes { uint32_t w[10], h[10]; };  // [d]: the LL band after d decompositions, d <= levels <= 8
inline J2kSizes j2k_level_sizes(uint32_t rows, uint32_t cols, uint32_t levels)
{
	J2kSizes z; z.w[0] = cols; z.h[0] = rows;
	for (uint32_t d = 1; d <= levels; d++) { z.w[d] = (z.w[d - 1] + 1) / 2; z.h[d] = (z.h[d - 1] + 1) / 2; }
	return z;
}
// band(orient, x0, y0, w, h) for every subband in packet order (tests/jpeg2000_model.py resolutions()): LL, then HL, LH, HH
// of every resolution from the coarsest; orient 0 LL, 1 HL, 2 LH, 3 HH; a band may be empty (w or h 0)
template <class F>
inline void j2k_for_each_band(uint32_t rows, uint32_t cols, uint32_t levels, F &&band)
{
	const J2kSizes z = j2k_level_sizes(rows, cols, levels);
	band(0u, 0u, 0u, z.w[levels], z.h[levels]);
	for (uint32_t r = 1; r <= levels; r++) {
		const uint32_t d = levels - r + 1, pw = z.w[d - 1], ph = z.h[d - 1], wl = z.w[d], hl = z.h[d];
		band(1u, wl, 0u, pw - wl, hl);
		band(2u, 0u, hl, wl, ph - hl);
		band(3u, wl, hl, pw - wl, ph - hl);
	}
}
// nodes of the tag tree (B.10.2) over ncw x nch >= 1 x 1 code-blocks
inline uint32_t j2k_tt_nodes(uint32_t ncw, uint32_t nch)
{
	uint32_t nodes = 0;
	for (uint32_t pw = ncw, ph = nch;; pw = (pw + 1) / 2, ph = (ph + 1) / 2) { nodes += pw * ph; if (pw == 1 && ph == 1) return nodes; }
}

// ---- JPEG 2000 Part-1 lossless encoder (jpeg2000_kernels.hip) -------------------------------------
// tests/jpeg2000_model.py states the file.  The host lays the image out once per call (j2k_layout): on top of the band walk
// above, the Mb of every subband from its gain, the square code-blocks, and a slab of the workspace for each.
constexpr uint32_t J2K_ST_OVERFLOW = 1u;  // a sample >= 2^precision after the shift (the convert kernel sets it)
constexpr uint32_t J2K_ST_CAP = 2u;       // a code-block's bytes or a packet header would leave its space
constexpr uint32_t J2K_ST_GUARD = 4u;     // a coefficient needs more bit-planes than the guard bits allow (Tier-1 sets it)
constexpr uint32_t J2K_HDR_MAX = 192;     // JP2 boxes 85, SOC 2, SIZ 43, COD 14, QCD 5 + 25, SOT 12, SOD 2 = 188 at 8 levels
constexpr uint32_t J2K_GUARD_BITS = 2;
constexpr uint32_t J2K_PKT_BYTES = 512;   // packet header bytes granted per packet ..
constexpr uint32_t J2K_CB_HDR_BYTES = 32; // .. and per code-block (cct_j2k_bound derives both)
constexpr uint32_t J2K_TT_LEVELS = 13;    // tag tree levels: at most 65535 / 32 + 1 = 2048 code-blocks a side, 2^11 -> 12 levels
struct J2kBlock {          // one code-block: where it lies in the plane, and its slab in the workspace of a frame
	uint16_t x0, y0, w, h;   // w, h <= 64
	uint32_t orient;         // 0 LL, 1 HL, 2 LH, 3 HH
	uint32_t mb;             // magnitude bit-planes of its subband: guard bits + exponent - 1 = precision + gain + 1
	uint32_t slab_off, slab_cap;
};
struct J2kBand { uint32_t cb0, ncw, nch, mb; };  // a subband in packet order: its first code-block, the grid (0 x 0: empty)
struct J2kBlockOut { uint32_t passes, bytes, zero_planes, dst; };  // Tier-1's result; dst: Tier-2's offset of the bytes in the file
struct J2kArgs {
	const void *images;        // n * rows * cols samples of src_bits (8 or 16)
	uint32_t src_bits, n, rows, cols, precision, shift, levels, codeblock;
	uint32_t stages;           // 7: all, always in a release build; a tuning build (tuning.h, CCT_J2K_STAGES) stops early: 1 convert and transform, 2 Tier-1, 4 Tier-2
	int32_t *plane_a, *plane_b;  // n * rows * cols each: the coefficients end up in plane_a
	const J2kBlock *blocks; uint32_t nblocks;
	const J2kBand *bands; uint32_t nbands;  // 1 + 3 * levels: LL, then HL, LH, HH of every resolution
	uint8_t *slabs; size_t slab_stride;     // a frame's code-block bytes: block b at slabs + frame * slab_stride + slab_off
	J2kBlockOut *cbout;        // n * nblocks
	uint8_t *tt; uint32_t tt_nodes;  // tag tree nodes: per frame 2 trees of 3 byte arrays (value, low, known) of tt_nodes
	uint32_t *status;          // n, zero on entry: J2K_ST_*
	uint32_t hdr_len, psot_at, jp2c_at;  // bytes of hdr; where Psot and (0: raw codestream) the jp2c box length are patched
	uint8_t hdr[J2K_HDR_MAX];  // everything up to and including SOD
	uint8_t *out; size_t out_stride; uint32_t *out_sizes;  // a frame with a status gets size 0
};
hipError_t launch_j2k_encode(const J2kArgs &a, hipStream_t st);

// The slab rule.  A sample takes part in at most mb magnitude decisions (one per bit-plane, in one of the three passes), one
// sign decision, and the run-length decisions of the cleanup pass, which replace the zero-coding decisions of the samples they
// cover or add two position bits to one of four samples: at most mb + 2 decisions a sample.  The MQ coder's estimates adapt,
// so a run of decisions against the estimate drives the state to Qe ~ 0.5, where a decision costs about one bit; the rule
// grants two bits a decision, (mb + 2) / 4 bytes a sample (5.25 for HH at precision 16, where uniform noise, the costliest
// content there is in practice, takes about 2.2), plus 64 bytes for the flush.  It is a rule, not a proof: Tier-1 checks
// every byte against it and refuses the frame (CCT_E_CAP) rather than write past the slab.
inline uint32_t j2k_slab_cap(uint32_t w, uint32_t h, uint32_t mb) { return (w * h * (mb + 2) + 3) / 4 + 64; }

struct J2kLayout {
	std::vector<J2kBlock> blocks;
	std::vector<J2kBand> bands;
	uint32_t tt_nodes = 1;   // nodes of the largest tag tree
	size_t slab_bytes = 0;   // a frame's slabs
	size_t bound = 0;        // cct_j2k_bound's expression for this layout
};
// Subbands in packet order and their code-blocks in raster order; caller-checked arguments: rows, cols 1 .. 65535,
// precision 2 .. 16, levels 0 .. 8, codeblock 32 or 64.
inline void j2k_layout(uint32_t rows, uint32_t cols, uint32_t precision, uint32_t levels, uint32_t codeblock, J2kLayout &L)
{
	L.blocks.clear(); L.bands.clear(); L.tt_nodes = 1; L.slab_bytes = 0;
	j2k_for_each_band(rows, cols, levels, [&](uint32_t orient, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
		const uint32_t gain = orient == 0 ? 0 : orient == 3 ? 2 : 1, mb = J2K_GUARD_BITS + precision + gain - 1;
		const uint32_t ncw = (w + codeblock - 1) / codeblock, nch = (h + codeblock - 1) / codeblock;
		J2kBand bd{(uint32_t)L.blocks.size(), w && h ? ncw : 0, w && h ? nch : 0, mb};
		L.bands.push_back(bd);
		if (!bd.ncw) return;
		const uint32_t nodes = j2k_tt_nodes(ncw, nch);
		L.tt_nodes = nodes > L.tt_nodes ? nodes : L.tt_nodes;
		for (uint32_t by = 0; by < h; by += codeblock)
			for (uint32_t bx = 0; bx < w; bx += codeblock) {
				J2kBlock b{};
				b.x0 = (uint16_t)(x0 + bx); b.y0 = (uint16_t)(y0 + by);
				b.w = (uint16_t)(w - bx < codeblock ? w - bx : codeblock); b.h = (uint16_t)(h - by < codeblock ? h - by : codeblock);
				b.orient = orient; b.mb = mb;
				b.slab_off = (uint32_t)L.slab_bytes; b.slab_cap = j2k_slab_cap(b.w, b.h, mb);
				L.slab_bytes += b.slab_cap;
				L.blocks.push_back(b);
			}
	});
	L.bound = J2K_HDR_MAX + 2 + (size_t)(levels + 1) * J2K_PKT_BYTES + L.blocks.size() * J2K_CB_HDR_BYTES + L.slab_bytes;
}

// Everything up to and including SOD (the JP2 boxes in front with jp2): -> its length; *psot_at and *jp2c_at (0 without
// jp2) are where Tier-2 patches Psot and the length of the jp2c box.  hdr holds J2K_HDR_MAX bytes.
inline uint32_t j2k_headers(uint32_t rows, uint32_t cols, uint32_t precision, uint32_t levels, uint32_t codeblock, bool jp2, uint8_t *hdr,
                            uint32_t *psot_at, uint32_t *jp2c_at)
{
	uint32_t n = 0;
	auto u8 = [&](uint32_t v) { hdr[n++] = (uint8_t)v; };
	auto u16 = [&](uint32_t v) { u8(v >> 8); u8(v); };
	auto u32 = [&](uint32_t v) { u16(v >> 16); u16(v & 0xFFFF); };
	auto tag = [&](const char *t) { for (int k = 0; k < 4; k++) u8((uint8_t)t[k]); };
	*jp2c_at = 0;
	if (jp2) {
		u32(12); tag("jP  "); u32(0x0D0A870A);
		u32(20); tag("ftyp"); tag("jp2 "); u32(0); tag("jp2 ");
		u32(45); tag("jp2h");
		u32(22); tag("ihdr"); u32(rows); u32(cols); u16(1); u8(precision - 1); u8(7); u8(0); u8(0);
		u32(15); tag("colr"); u8(1); u8(0); u8(0); u32(17);
		*jp2c_at = n;
		u32(0); tag("jp2c");
	}
	u16(0xFF4F);
	u16(0xFF51); u16(41); u16(0); u32(cols); u32(rows); u32(0); u32(0); u32(cols); u32(rows); u32(0); u32(0); u16(1); u8(precision - 1); u8(1); u8(1);
	const uint32_t cbe = codeblock == 64 ? 4 : 3;
	u16(0xFF52); u16(12); u8(0); u8(0); u16(1); u8(0); u8(levels); u8(cbe); u8(cbe); u8(0); u8(1);
	u16(0xFF5C); u16(3 + 1 + 3 * levels); u8(J2K_GUARD_BITS << 5); u8(precision << 3);
	for (uint32_t l = 0; l < levels; l++) { u8((precision + 1) << 3); u8((precision + 1) << 3); u8((precision + 2) << 3); }
	u16(0xFF90); u16(10); u16(0);
	*psot_at = n;
	u32(0); u8(0); u8(1);
	u16(0xFF93);
	return n;
}

// ---- JPEG 2000 Part-1 lossless decoder (jpeg2000_decode_kernels.hip) ------------------------------
// tests/jpeg2000_decode_model.py states it.  The host walks the markers (api_jpeg2000.cpp) and lays every distinct coding
// (levels, code-block exponents, Mb per subband) out once per call (j2k_dec_layout): on top of the same band walk, the Mb of
// every subband from QCD, where its tag trees begin, and the rectangular code-blocks.  A file reaches the device as the byte
// range of its tile data and a J2kDecFile; its state on the device is one J2kDecCb per code-block, the nodes of two tag trees
// per subband, a list of the chunks its packets hold, and the codeword segments the chunks are gathered into.
constexpr uint32_t J2K_DEC_MB_MAX = 19;     // magnitude bit-planes the Tier-1 word holds: bits 12 .. 30 (jpeg2000_device.h)
constexpr uint32_t J2K_DEC_TT_LEVELS = 16;  // 65535 / 4 + 1 = 16384 code-blocks a side: 15 levels
constexpr uint32_t J2K_DEC_ST_STREAM = 1u;
struct J2kDecBlock { uint16_t x0, y0, w, h; uint32_t orient, mb; };  // w, h <= 64
struct J2kDecBand { uint32_t cb0, ncw, nch, mb, tt0; };  // cb0, tt0: its first block and tag-tree node within the layout
struct J2kDecFile {
	uint64_t src;              // offset of the tile data (behind SOD) in the upload; its segments go to the same offset of segs
	uint32_t len;              // bytes of tile data
	uint32_t slot;             // the raster it fills: images + slot * rows * cols
	uint32_t precision, levels, layers, seq;  // seq 0: layer-major packets (LRCP), 1: resolution-major (the other four orders)
	uint32_t blk0, nblocks;    // its layout's blocks in the block table
	uint32_t band0;            // its layout's 1 + 3 * levels subbands in the band table
	uint32_t cb0;              // its first J2kDecCb among the pass's
	uint64_t tt0; uint32_t tt_nodes;  // its tag-tree bytes: 4 arrays of tt_nodes (inclusion low, value; zero planes low, value)
	uint64_t chunk0; uint32_t chunk_cap;  // its chunk list
	uint32_t xcb, ycb;         // code-block exponents: the LDS a block of this file takes
};
struct J2kDecCb {            // a code-block across the layers; its index minus the file's cb0 is its block in the layout
	uint32_t file;             // whose it is
	uint32_t passes, planes;   // coding passes so far; Mb - zero bit-planes
	uint32_t bytes, seg;       // bytes so far; where its segment begins (relative to the file's src)
	uint32_t lblock, included; // included: in some packet so far
	uint32_t pend;             // the bytes it has in the current packet; while the chunks are placed, the bytes placed so far
};
struct J2kDecChunk { uint32_t cb, src, len, dst; };  // cb within the file; src in the tile data, dst in the segments, both relative to the file's src
struct J2kDecArgs {
	const uint8_t *files; uint8_t *segs;
	const J2kDecFile *flist; uint32_t nfiles;
	const J2kDecBlock *blocks; const J2kDecBand *bands;
	J2kDecCb *cbs; uint32_t ncbs;
	uint8_t *tt; J2kDecChunk *chunks;
	uint32_t *status;          // nfiles, zero on entry: J2K_DEC_ST_STREAM
	int32_t *plane_a, *plane_b;  // one rows x cols plane per slot each
	uint32_t nslots, rows, cols, max_levels, out_bits, shift, stages;  // stages: 15 all, always in a release build (tuning.h, CCT_J2K_DEC_STAGES); 1 parse, 2 Tier-1, 4 transform, 8 finish
	void *images;
};
struct J2kDecRun { uint32_t cb0, ncbs, xcb, ycb; };  // consecutive files with the same code-block exponents: one Tier-1 launch
hipError_t launch_j2k_decode(const J2kDecArgs &a, const J2kDecRun *runs, size_t nruns, hipStream_t st);
inline size_t j2k_dec_lds_bytes(uint32_t xcb, uint32_t ycb) { return 776 + (size_t)((1u << xcb) + 2) * ((1u << ycb) + 2) * 4; }

struct J2kDecLayout {
	uint32_t levels, xcb, ycb, mb[25];
	std::vector<J2kDecBlock> blocks;
	std::vector<J2kDecBand> bands;
	uint32_t tt_nodes = 0;
};
// caller-checked: rows, cols 1 .. 65535, levels 0 .. 8, xcb, ycb 2 .. 6, mb[] <= J2K_DEC_MB_MAX
inline void j2k_dec_layout(uint32_t rows, uint32_t cols, J2kDecLayout &L)
{
	const uint32_t cw = 1u << L.xcb, ch = 1u << L.ycb;
	uint32_t nb = 0;
	L.blocks.clear(); L.bands.clear(); L.tt_nodes = 0;
	j2k_for_each_band(rows, cols, L.levels, [&](uint32_t orient, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
		const uint32_t mb = L.mb[nb++], ncw = (w + cw - 1) / cw, nch = (h + ch - 1) / ch;
		J2kDecBand bd{(uint32_t)L.blocks.size(), w && h ? ncw : 0, w && h ? nch : 0, mb, L.tt_nodes};
		L.bands.push_back(bd);
		if (!bd.ncw) return;
		L.tt_nodes += j2k_tt_nodes(ncw, nch);
		for (uint32_t by = 0; by < h; by += ch)
			for (uint32_t bx = 0; bx < w; bx += cw) {
				J2kDecBlock b{};
				b.x0 = (uint16_t)(x0 + bx); b.y0 = (uint16_t)(y0 + by);
				b.w = (uint16_t)(w - bx < cw ? w - bx : cw); b.h = (uint16_t)(h - by < ch ? h - by : ch);
				b.orient = orient; b.mb = mb;
				L.blocks.push_back(b);
			}
	});
	if (!L.tt_nodes) L.tt_nodes = 1;
}

}  // namespace cct
