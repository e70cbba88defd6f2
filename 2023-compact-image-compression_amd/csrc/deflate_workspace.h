// The HBM workspace of the device DEFLATE pass (deflate_kernels.hip), described once: the constants host and kernels share,
// the list of regions with their sizes and the passes that need them, the one function that binds DeflateArgs to them, and
// the accessors through which the kernels address what several things share.  The host (api.cpp deflate_locked) allocates
// and binds from this file; the kernels address through it.  Plain C++: a host compiler reads it without the HIP headers
// (tests/test_deflate_workspace_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DFL_HD __host__ __device__ __forceinline__
#else
#define DFL_HD inline
#endif

namespace cct {

struct BlockMeta {          // one DEFLATE block of a slice
	uint64_t bit_off;         // absolute bit offset of the 3 header bits inside the slice's output
	uint32_t type;            // 0 stored, 1 static trees, 2 dynamic trees
	uint32_t last;
	uint32_t first_sym, nsym;
	uint32_t in_begin, stored_len;
	uint32_t hdr_nbits, body_bits;
};
struct BlockTables {
	uint16_t lcode[286]; uint8_t llen[286];
	uint16_t dcode[30]; uint8_t dlen[30];
	uint32_t hdr_bits[160];
};
// The kernels' argument block.  It keeps its layout: the captured DEFLATE graphs are keyed by its bytes (deflate_locked), and
// for equal arguments dfl_bind gives every pointer the value it always had, so they hit and miss as before.
struct DeflateArgs {
	const uint8_t *in; size_t in_stride; const uint32_t *in_sizes;  // token payloads (device)
	uint64_t *rec_in, *rec_out;                                      // n * in_stride each: sort records (deflate_kernels.hip, "Sort records"), between / after the sort passes
	uint32_t pos_mask;                                               // position bits of a record's lower word: 2^22 - 1 (compact records, in_stride < 4 MiB) or all 32
	uint32_t *seg_begin, *seg_end;                                   // n
	void *mr;                                                        // n * in_stride * 8 bytes: match records, valid where they carry the tag *gen
	uint32_t *gen;                                                   // device counter of the passes run on this mr buffer, 1 .. 16383 (deflate_kernels.hip MatchRec)
	uint32_t *heavy_list, *sym, *run_ends;                           // n * in_stride each
	uint32_t *run_counts; int run_chunks;                            // n * 2 * run_chunks right behind sort_hist: run ends / starts per chunk of RUNLEN_OUT positions (run_chunks = chunks per slice)
	uint32_t *sort_hist;                                             // n * SORT_HIST: per slice the histograms of hash & 255 and of hash >> 8 (dfl_run_len_kernel -> sort passes)
	uint16_t *run_len;                                               // n * in_stride: equal bytes ahead (<= 258) | has_prev << 15
	uint32_t *rec32, *exit_pos, *exit_cnt;                           // n * in_stride each
	uint32_t *blk_entry, *blk_symbase;                               // n * in_stride / 64
	uint32_t *total_syms, *postloop_lit, *n_blocks, *adler, *heavy_count, *deep_count, *run_end_count;  // n
	uint32_t *blk_end;                                               // n * max_blocks
	uint32_t *blk_top;                                               // n * max_blocks: position at the top of the loop iteration that flushed the block (dfl_tree_kernel, window_base)
	BlockMeta *block_meta; BlockTables *block_tables;                // n * max_blocks
	int max_blocks;
	uint8_t *out; size_t out_stride; uint32_t *out_sizes;            // whole .cct files (header + zlib stream)
	uint8_t header13[16];
	// the zlib level (4 .. 9, all deflate_slow): deflate.c configuration_table entries and the second header byte
	uint32_t good, max_lazy, nice, max_chain, zlib_flg;
	// the zlib strategy (0 .. 4, deflate_kernels.hip "zlib strategies") and the shortest match deflate_slow keeps:
	// MIN_MATCH, or 6 under Z_FILTERED (matches of <= 5 bytes dropped)
	uint32_t strategy, min_len;
	// the zlib memLevel (8 or 9): hash bits (memLevel + 7) and symbols per block (lit_bufsize - 1)
	uint32_t hash_bits, block_syms;
	// waves per workgroup of dfl_tree_kernel, 1 or 16, or 0: chosen per pass (option "tree_waves"; deflate_kernels.hip launch_tree)
	uint32_t tree_waves;
};

// ---- shared constants ------------------------------------------------------------------------------
// sort histogram words per slice: 256 digits of hash & 255, then up to 256 of hash >> 8 (16-bit hash, memLevel 9)
constexpr int SORT_HIST = 512;
// positions a workgroup of dfl_run_len_kernel publishes: it scans 2048 (8 per lane), and for the first RUNLEN_OUT of them the
// scanned tail (>= 264 bytes) decides every length below the cap.  dfl_run_lists_kernel runs one workgroup per such chunk.
constexpr int RUNLEN_OUT = 2048 - 264;
// input positions per word of blk_entry / blk_symbase: the walk enters every 64-position block at most once
constexpr int BLK_ENTRY_GRAIN = 64;
// the per-slice counter arrays, n words each, in the order they lie at the head of their region
enum DflCounter { DFL_SEG_BEGIN, DFL_SEG_END, DFL_TOTAL_SYMS, DFL_POSTLOOP_LIT, DFL_N_BLOCKS, DFL_ADLER, DFL_HEAVY_COUNT,
                  DFL_DEEP_COUNT, DFL_RUN_END_COUNT, DFL_COUNTERS };

// chunks of RUNLEN_OUT positions per slice
DFL_HD int dfl_run_chunks(size_t in_stride) { return (int)(in_stride / RUNLEN_OUT + 1); }
// DEFLATE blocks a slice can have: one per block_syms symbols (a symbol covers at least one byte), the last one, an empty one
DFL_HD int dfl_max_blocks(size_t in_stride, uint32_t block_syms) { return (int)(in_stride / block_syms + 2); }
// words of blk_entry / blk_symbase per slice
DFL_HD size_t dfl_blk_words(size_t in_stride) { return in_stride / BLK_ENTRY_GRAIN; }
// words of sort_hist and, directly behind it, run_counts: dfl_offsets_kernel zeroes both as one extent
DFL_HD size_t dfl_hist_words(size_t n, size_t run_chunks) { return n * (SORT_HIST + 2 * run_chunks); }

// Bytes a zlib stream of n input bytes can take: zlib's compressBound at memLevel 8 (deflateBound's tight bound for the
// default parameters), deflateBound's general bound otherwise.  memLevel 9's 32767-symbol blocks can straddle a slide of the
// window, where zlib may not store them: random bytes under Z_FILTERED come out 0.09 % above compressBound.
DFL_HD size_t zlib_bound(size_t n, bool mem_level_8)
{
	return mem_level_8 ? n + (n >> 12) + (n >> 14) + (n >> 25) + 13 : n + ((n + 7) >> 3) + ((n + 63) >> 6) + 5 + 6;
}
// Strides of a pass's input and output slices, from the longest input: 16 bytes the kernels may read past the end, rounded
// to the 256 the pass asks for; 13 header bytes and the bound of the stream, rounded to 64.
inline size_t deflate_in_stride(size_t longest) { return (longest + 16 + 255) & ~(size_t)255; }
inline size_t deflate_out_stride(size_t in_stride, int mem_level) { return (13 + zlib_bound(in_stride, mem_level == 8) + 63) & ~(size_t)63; }

// ---- the regions -----------------------------------------------------------------------------------
// They are separate allocations, each grown on its own (DevBuf::ensure), never one arena: match records are valid by tag, which
// relies on their buffer keeping its address and contents from pass to pass, and an arena would move it whenever n or the
// stride changes; and a pass at its bound (2^30 payload bytes) needs 47 GB, which should not be one allocation.
enum DflRegion {
	DFL_R_REC_IN,       // sort records between the two sort passes
	DFL_R_REC_OUT,      // sorted records
	DFL_R_MATCH,        // match records
	DFL_R_RUNS,         // run lists, per slice four quarters of in_stride words (dfl_run_starts, dfl_run_info, dfl_run_rank)
	DFL_R_QUEUES,       // heavy queue growing up and deep queue growing down (dfl_deep_top), then the exit counts
	DFL_R_SYM,          // symbols, and the run-length words before them
	DFL_R_REC32,        // decision records
	DFL_R_EXIT_POS,     // exit of every position's 64-position block
	DFL_R_BLK_ENTRY,    // where the walk enters every 64-position block
	DFL_R_BLK_SYMBASE,  // symbols before that entry
	DFL_R_SMALL,        // the DFL_COUNTERS counter arrays, sort_hist, run_counts
	DFL_R_BLK_ENDS,     // blk_end, then blk_top
	DFL_R_META,         // BlockMeta
	DFL_R_TABLES,       // BlockTables
	DFL_R_GEN,          // tag counter of the match records
	DFL_REGIONS
};
// Which passes use a region.  Z_HUFFMAN_ONLY (2) and Z_RLE (3) run the short pass without hash chains: no sort records, match
// records, run lists or queues, and Z_HUFFMAN_ONLY no decision records or walk either.  A short pass neither grows nor clears
// what it does not need.
enum DflNeed { DFL_ALWAYS, DFL_CHAINS, DFL_WALK };
constexpr DflNeed DFL_REGION_NEED[DFL_REGIONS] = {
	DFL_CHAINS, DFL_CHAINS, DFL_CHAINS, DFL_CHAINS, DFL_CHAINS, DFL_ALWAYS, DFL_WALK, DFL_WALK, DFL_WALK, DFL_WALK,
	DFL_ALWAYS, DFL_ALWAYS, DFL_ALWAYS, DFL_ALWAYS, DFL_ALWAYS};
inline bool dfl_uses_chains(int strategy) { return strategy != 2 && strategy != 3; }
inline bool dfl_region_needed(int r, int strategy)
{
	return DFL_REGION_NEED[r] == DFL_ALWAYS || (DFL_REGION_NEED[r] == DFL_CHAINS ? dfl_uses_chains(strategy) : strategy != 2);
}

struct DflShape { size_t n, in_stride, max_blocks, run_chunks; };  // what the sizes depend on
inline DflShape dfl_shape(int n, size_t in_stride, uint32_t block_syms)
{
	return {(size_t)n, in_stride, (size_t)dfl_max_blocks(in_stride, block_syms), (size_t)dfl_run_chunks(in_stride)};
}
inline size_t dfl_region_bytes(int r, const DflShape &w)
{
	const size_t EB = w.n * w.in_stride;
	switch (r) {
	case DFL_R_REC_IN: case DFL_R_REC_OUT: case DFL_R_MATCH: return EB * 8;
	case DFL_R_RUNS: case DFL_R_QUEUES: case DFL_R_SYM: case DFL_R_REC32: case DFL_R_EXIT_POS: return EB * 4;
	case DFL_R_BLK_ENTRY: case DFL_R_BLK_SYMBASE: return EB / BLK_ENTRY_GRAIN * 4;
	case DFL_R_SMALL: return (DFL_COUNTERS * w.n + dfl_hist_words(w.n, w.run_chunks)) * 4;
	case DFL_R_BLK_ENDS: return w.n * w.max_blocks * 8;
	case DFL_R_META: return w.n * w.max_blocks * sizeof(BlockMeta);
	case DFL_R_TABLES: return w.n * w.max_blocks * sizeof(BlockTables);
	case DFL_R_GEN: return 256;
	}
	return 0;
}

// Every workspace pointer of DeflateArgs, from the regions' base addresses (of a region the pass does not need: whatever its
// buffer holds, nobody reads it).
inline void dfl_bind(DeflateArgs &a, void *const base[DFL_REGIONS], const DflShape &w)
{
	a.rec_in = (uint64_t *)base[DFL_R_REC_IN]; a.rec_out = (uint64_t *)base[DFL_R_REC_OUT];
	a.mr = base[DFL_R_MATCH]; a.gen = (uint32_t *)base[DFL_R_GEN];
	a.run_ends = (uint32_t *)base[DFL_R_RUNS];  // a region of their own: the lists are built while the sort runs (launch_deflate)
	a.heavy_list = (uint32_t *)base[DFL_R_QUEUES];
	a.exit_cnt = (uint32_t *)base[DFL_R_QUEUES];  // alias: the heavy / deep queues are dead once dfl_rec_kernel runs, which writes these
	a.sym = (uint32_t *)base[DFL_R_SYM];
	a.run_len = (uint16_t *)base[DFL_R_SYM];  // alias: 2 bytes per position, written before the sort and dead before the symbols are written
	a.rec32 = (uint32_t *)base[DFL_R_REC32]; a.exit_pos = (uint32_t *)base[DFL_R_EXIT_POS];
	a.blk_entry = (uint32_t *)base[DFL_R_BLK_ENTRY]; a.blk_symbase = (uint32_t *)base[DFL_R_BLK_SYMBASE];
	uint32_t *small = (uint32_t *)base[DFL_R_SMALL];
	a.seg_begin = small + DFL_SEG_BEGIN * w.n; a.seg_end = small + DFL_SEG_END * w.n; a.total_syms = small + DFL_TOTAL_SYMS * w.n;
	a.postloop_lit = small + DFL_POSTLOOP_LIT * w.n; a.n_blocks = small + DFL_N_BLOCKS * w.n; a.adler = small + DFL_ADLER * w.n;
	a.heavy_count = small + DFL_HEAVY_COUNT * w.n; a.deep_count = small + DFL_DEEP_COUNT * w.n;
	a.run_end_count = small + DFL_RUN_END_COUNT * w.n;
	a.sort_hist = small + DFL_COUNTERS * w.n;
	a.run_counts = a.sort_hist + SORT_HIST * w.n;  // directly behind sort_hist: dfl_offsets_kernel zeroes both (dfl_hist_words)
	a.run_chunks = (int)w.run_chunks;
	a.blk_end = (uint32_t *)base[DFL_R_BLK_ENDS]; a.blk_top = a.blk_end + w.n * w.max_blocks;
	a.block_meta = (BlockMeta *)base[DFL_R_META]; a.block_tables = (BlockTables *)base[DFL_R_TABLES];
	a.max_blocks = (int)w.max_blocks;
}

// ---- what the kernels address through ----------------------------------------------------------------
// Run lists of a slice (re = run_ends + s * in_stride, in_stride words, at most L / 4 runs): ends in the first quarter, starts
// in the second, length | byte << 16 in the third, and in the fourth the rank among the ends of every eighth position
// (in_stride / 8 words).
template <class T> DFL_HD T *dfl_run_starts(T *re, size_t in_stride) { return re + (in_stride >> 2); }
template <class T> DFL_HD T *dfl_run_info(T *re, size_t in_stride) { return re + (in_stride >> 1); }
DFL_HD size_t dfl_run_rank(size_t in_stride, uint32_t p) { return 3 * (in_stride >> 2) + (p >> 3); }  // index into re, for position p
// The heavy and deep queues of a slice share in_stride words (q = heavy_list + s * in_stride): the heavy queue grows up from
// q, the deep queue down from here
template <class T> DFL_HD T *dfl_deep_top(T *q, size_t in_stride) { return q + in_stride - 1; }

}  // namespace cct
