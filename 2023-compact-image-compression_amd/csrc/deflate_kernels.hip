// Device DEFLATE, byte-identical to zlib 1.2.11 `deflateInit2(level L, Z_DEFLATED, wbits 15, memLevel M,
// strategy S)` + one-shot Z_FINISH for L = 4 .. 9 and M = 8 or 9 -- level 9 with the default strategy is the stream CPython's
// zlib.compress(data, level=9) produces for the reference (src/codec/core.py:340).  zlib is a third-party dependency of the
// reference and is not vendored there; the algorithm is restated here in data-parallel form (CPU model
// of the same restatement, pinned against libz: oracle/deflate_model.c for level 9,
// tools/deflate_level_model.c for every level).  All six levels run deflate_slow, which inserts every
// string into the hash chains; the level enters only through good / max_lazy / nice / max_chain
// (DeflateArgs) in the match and decision kernels, and the second zlib header byte.
//
// zlib strategies (DeflateArgs::strategy): Z_DEFAULT_STRATEGY and Z_FIXED (static trees unless a stored block is
// smaller: dfl_tree_kernel) and Z_FILTERED (matches of <= 5 bytes dropped: match_of) run deflate_slow, levels 4 .. 9.
// Z_RLE (deflate_rle: greedy matches at distance 1 only) and Z_HUFFMAN_ONLY (deflate_huff: literals only) run at any
// level 1 .. 9 with the same bytes, as a short pass without the sort and match kernels (launch_deflate).
//
// zlib memLevel (DeflateArgs::hash_bits, block_syms): memLevel 8 hashes 3 bytes into 15 bits (hash_shift 5) and ends a block
// after 16383 tallied symbols; memLevel 9 into 16 bits (hash_shift 6), blocks of 32767 symbols.  Nothing else of deflate_slow,
// deflate_rle or deflate_huff depends on it.  The kernels that need the widths at compile time take them as template arguments
// (HB = hash bits, BS = block symbols); memLevel 9 runs on wide sort records only (api.cpp deflate_locked, "Sort records").
//
//   sort      stable two-pass LSD radix sort of (hash, position) per slice, the 15- or 16-bit rolling hash of 3 bytes
//             (deflate.c UPDATE_HASH) computed on the fly: a bucket in position order IS zlib's hash chain
//             (head/prev), walked backwards
//   runs      ordered list of the runs of >= 3 equal bytes and, per position, the equal bytes ahead
//   match     what longest_match() returns over the first max_chain / max_chain>>2 chain entries ("full", and
//             "quarter" once prev_length >= good_match), stopping at the first entry that reaches nice_match
//             (capped by the lookahead), with the NIL / MAX_DIST / lookahead rules of
//             deflate.c: one lane per position for short chains, one wave per position for long ones, and
//             the run list instead of the chain for strings that start a run (their bucket holds every
//             position of every run of that byte)
//   parse     deflate_slow's lazy evaluation as a walk over "decision positions": per position the
//             deferral chain is resolved locally, 64-position blocks are summarised by pointer
//             doubling (entry -> exit, symbol count), the block-to-block hop chain is walked
//             speculatively by 256 lanes per slice
//   symbols   visited positions emit literals / (length, distance) pairs in stream order
//   trees     per 16383- (32767-) symbol block: histograms, then build_tree / gen_bitlen / gen_codes /
//             scan_tree / build_bl_tree exactly as trees.c (the heap is replayed: ties are decided by heap
//             position), stored / static / dynamic choice
//   emit      code bits of every symbol at its prefix-summed bit offset; zlib header, Adler-32
// The launches of one pass are captured into a HIP graph by the caller (api.cpp).
#include <hip/hip_runtime.h>
#include <cstring>
#include <algorithm>

#include "cct_internal.h"
#include "wave_device.h"
#include "../../include/compact_hip.h"

namespace cct {
namespace {

constexpr int MIN_MATCH = 3, MAX_MATCH = 258, WSIZE = 32768;
constexpr int MIN_LOOKAHEAD = MAX_MATCH + MIN_MATCH + 1;
constexpr int MAX_DIST = WSIZE - MIN_LOOKAHEAD;  // 32506
constexpr int TOO_FAR = 4096;
constexpr int BLOCK_SYMS = 16383;                // lit_bufsize - 1 (memLevel 8; DeflateArgs::block_syms at run time)
constexpr int BLOCK_SYMS_ML9 = 32767;            // lit_bufsize - 1 (memLevel 9)
constexpr int L_CODES = 286, D_CODES = 30, BL_CODES = 19, HEAP_SIZE = 2 * L_CODES + 1;
constexpr int END_BLOCK = 256, MAX_BITS = 15, MAX_BL_BITS = 7;
constexpr uint32_t Z_FILTERED = 1, Z_HUFFMAN_ONLY = 2, Z_RLE = 3, Z_FIXED = 4;  // zlib.h strategies
// deflate_huff / deflate_rle instead of deflate_slow: the short pass (launch_deflate)
__host__ __device__ __forceinline__ bool short_pass(uint32_t strategy) { return strategy == Z_HUFFMAN_ONLY || strategy == Z_RLE; }

__constant__ uint8_t c_extra_lbits[29] = {0,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,0};
__constant__ uint8_t c_extra_dbits[30] = {0,0,0,0,1,1,2,2,3,3,4,4,5,5,6,6,7,7,8,8,9,9,10,10,11,11,12,12,13,13};
__constant__ uint8_t c_extra_blbits[19] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,2,3,7};
__constant__ uint8_t c_bl_order[19] = {16,17,18,0,8,7,9,6,10,5,11,4,12,3,13,2,14,1,15};
// tr_static_init tables, filled by the host once (cct::deflate_init_tables)
__constant__ uint8_t c_length_code[256];
__constant__ uint16_t c_base_length[29];
__constant__ uint8_t c_dist_code[512];
__constant__ uint16_t c_base_dist[30];
__constant__ uint16_t c_static_lcode[288];
__constant__ uint8_t c_static_llen[288];
__constant__ uint16_t c_static_dcode[30];

// deflate.c UPDATE_HASH over the three bytes of a string: hash_bits HB = memLevel + 7, hash_shift = (HB + 2) / 3.  The shift
// is at least HB / 3, so the hash of any earlier byte has left the mask: the three bytes alone decide it
template <int HB>
__device__ __forceinline__ uint32_t hash3(uint32_t b0, uint32_t b1, uint32_t b2)
{
	constexpr int SH = (HB + 2) / 3;
	return ((b0 << (2 * SH)) ^ (b1 << SH) ^ b2) & ((1u << HB) - 1u);
}

__device__ __forceinline__ int d_code(uint32_t dist) { return dist < 256 ? c_dist_code[dist] : c_dist_code[256 + (dist >> 7)]; }

struct MatchRec { uint16_t len_full, len_quarter, dist_full, dist_quarter; };
// Match records are only stored where there is something to say (a match of >= MIN_MATCH bytes): a record counts when it
// carries the tag of the current pass -- 14 bits in the spare upper bits of the two length fields (lengths are <= 258), taken
// from a device counter that dfl_offsets_kernel advances at the start of every pass (1 .. 16383; the host clears the buffer
// before the counter would come round, api.cpp deflate_locked).  Writing a "no match" record for every position instead cost
// 0.17 ms per batch (555 MB of stores), as much as the scattered stores it had saved in the match kernel.
constexpr uint32_t GEN_MAX = 16383;
__device__ __forceinline__ uint2 pack_match(uint32_t len_full, uint32_t len_quarter, uint32_t dist_full, uint32_t dist_quarter, uint32_t gen)
{
	return make_uint2((len_full | ((gen & 127u) << 9)) | ((len_quarter | ((gen >> 7) << 9)) << 16), dist_full | (dist_quarter << 16));
}
// The record of position p as the parse reads it: the stored one if it carries this pass's tag; else "no match" -- or, deep
// inside a run (in[p-1] == in[p] and at least max_len equal bytes ahead), the chain head p-1 at the cap, which nobody stores:
// rw = run-length word of p (dfl_run_len_kernel).  At every level the walk stops at that head: max_len >= nice_eff.
__device__ __forceinline__ MatchRec checked_match(MatchRec r, uint32_t gen, uint32_t rw, uint32_t p, uint32_t L)
{
	const uint32_t tag = (uint32_t)(r.len_full >> 9) | ((uint32_t)(r.len_quarter >> 9) << 7);
	const uint32_t lookahead = L - min(p, L);
	const uint32_t max_len = lookahead < (uint32_t)MAX_MATCH ? lookahead : (uint32_t)MAX_MATCH;
	const bool maximal = (rw >> 15) && (rw & 0x7FFFu) >= max_len && p + 2 < L;
	MatchRec o;
	const bool ok = tag == gen;
	o.len_full = ok ? (uint16_t)(r.len_full & 511u) : (uint16_t)(maximal ? max_len : 0u);
	o.len_quarter = ok ? (uint16_t)(r.len_quarter & 511u) : (uint16_t)(maximal ? max_len : 0u);
	o.dist_full = ok ? r.dist_full : (uint16_t)(maximal ? 1u : 0u);
	o.dist_quarter = ok ? r.dist_quarter : (uint16_t)(maximal ? 1u : 0u);
	return o;
}

// ------------------------------------------------------------------ 1. hash + sort by (hash, position)
// The chain of a string = the earlier strings with the same 15-bit (16-bit) hash, most recent first (deflate.c
// INSERT_STRING / prev[]).  Sorting the positions of a slice by (hash, position) lays every chain out as a
// contiguous run.  Stable LSD radix sort in two passes (hash & 255, then hash >> 8); ONE workgroup of 1024 lanes
// per slice walks its slice tile by tile with running digit offsets in LDS, so there is no cross-workgroup
// scan: pass A hashes the input on the fly (value = position = index) and also counts pass B's digits.
// Per tile: wave-level match-any gives each lane its rank among the equal digits of its wave, the 16 per-wave
// counts are prefix-summed per digit, and lanes scatter to offset[digit] + wave prefix + rank.  All waves of a
// slice write the same 256 (128) output streams tile after tile, which keeps the partially written lines in L2.
// (The barriers between a tile's scattered stores are lds_barrier(): __syncthreads() would drain vmcnt and serialise them.)
template <bool FIRST, int HB>
__global__ void __launch_bounds__(1024) dfl_sort_pass_kernel(DeflateArgs a)
{
	constexpr int BITS = FIRST ? 8 : HB - 8, NB = 1 << BITS;
	constexpr uint32_t HMASK = (1u << HB) - 1u;
	__shared__ uint32_t offs[256];
	__shared__ uint32_t wcnt[16][NB];
	const int s = blockIdx.x;
	const uint32_t L = a.in_sizes[s];
	const uint8_t *in = a.in + (size_t)s * a.in_stride;
	const size_t base = (size_t)s * a.in_stride;
	const uint32_t npos = L >= MIN_MATCH ? L - 2 : 0;
	// one 8-byte record per string: position | hash << 32.  The scatter below is bound by store transactions (every lane
	// of a store instruction hits another output stream), so key and value travel in one store, and the match kernels
	// get both with one scattered load
	const uint64_t *rec_src = a.rec_in + base;
	uint64_t *rec_dst = (FIRST ? a.rec_in : a.rec_out) + base;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint64_t lt_mask = (1ull << lane) - 1ull;
	if (tid < 256) offs[tid] = 0;
	__syncthreads();
	// digit histogram of this pass: counted by dfl_run_len_kernel, which reads the input in position order with the whole chip
	// (here one workgroup per slice would wait for its loads, and pass A paid an LDS atomic per element for pass B's histogram)
	if (tid < NB) offs[tid] = a.sort_hist[(size_t)s * SORT_HIST + (FIRST ? 0 : 256) + tid];
	__syncthreads();
	if (wave == 0) {  // exclusive scan of up to 256 bins: 4 per lane
		uint32_t v[4], sum = 0;
#pragma unroll
		for (int k = 0; k < 4; k++) { v[k] = offs[lane * 4 + k]; sum += v[k]; }
		uint32_t run = wave_incl_scan(sum) - sum;
#pragma unroll
		for (int k = 0; k < 4; k++) { offs[lane * 4 + k] = run; run += v[k]; }
	}
	__syncthreads();
	// A tile = 4096 elements: wave w owns elements [t0 + 256 w, t0 + 256 w + 256) and ranks them in four rounds of
	// 64 (running per-digit counts in its own LDS row), so the cross-wave prefix and its two barriers are paid
	// once per 4096 elements.  Loads of the next tile are issued before the current one is ranked.
#ifndef CCT_SORT_E
#define CCT_SORT_E 4  // pass B alone, per batch: 2: 366, 4: 359, 8: 330-343 us, 12 spills (1318 us) -- but with 8 the kernel needs 116
                      // VGPRs, a CU no longer holds its 16 waves next to an INFLATE workgroup, and in the pipelined bench the DEFLATE pass
                      // took 4.67 instead of 3.5 ms (13.3 K instead of 17.4 K MPixels/s): 4 (72 VGPRs)
#endif
	constexpr int E = CCT_SORT_E;
	constexpr int ND = E / 4;  // pass A: input dwords per lane (a wave's tile = 64 E positions = 16 E dwords)
	// Loads of the next tile are issued before the current one is ranked and taken after it.  Two things the compiler did with
	// the obvious code: inside a conditional it waits for every load right where it is issued (s_waitcnt vmcnt(0) before the
	// join), which made the "prefetch" four full memory round trips in a row per tile; and it moved the first use of the
	// loaded values past this tile's scattered stores, where waiting for the loads means waiting for the stores too (one
	// in-order counter).  So: the index is clamped instead of tested, the raw values pass through an empty asm right before
	// the stores (that is where the wait lands), and hash / position are derived after it.
	const uint32_t last = npos ? npos - 1 : 0;
	// Pass A reads the input as aligned dwords: the 64 E positions of a wave's tile need bytes [B, B + 64 E + 4), lane l loads the dwords
	// at B + 256 d + 4 l and everybody the one after the tile; a position takes its two dwords from the lanes that hold them (ds_bpermute) and
	// shifts its five bytes out.  (One byte-granular load per position and field was tried first: the pass went 0.44 -> 0.59 ms,
	// the address unit handles such loads lane by lane.)  Bytes past the end of the slice are whatever the buffer holds: the hash
	// of a valid position (p < L - 2) never sees them, and the match kernel does not use the compact fields of the last positions.
	static_assert(E % 4 == 0 && ND + 1 <= E, "pass A: whole dwords per lane, kept in ra[0 .. ND]");
#ifdef CCT_SORT_PROBE  // tuning builds only (results invalid)
	const bool compact = false;
#else
	const bool compact = HB == 15 && a.pos_mask != 0xFFFFFFFFu;  // (memLevel 8 only)
#endif
	const uint32_t dmax = (uint32_t)a.in_stride - 4u;
	// tile_base = first element of this wave's 256; ra/rb = the values as loaded: anything computed here is computed (and waited for) early
	auto fetch = [&](uint32_t tile_base, uint32_t (&ra)[E], uint32_t (&rb)[E]) {
		if (FIRST) {
#pragma unroll
			for (int d = 0; d < ND; d++) ra[d] = *reinterpret_cast<const uint32_t *>(in + min(tile_base + 256u * d + 4u * (uint32_t)lane, dmax));
			ra[ND] = *reinterpret_cast<const uint32_t *>(in + min(tile_base + 256u * ND, dmax));  // the dword after the tile, the same in every lane
#pragma unroll
			for (int e = 0; e < E; e++) rb[e] = compact ? a.run_len[base + min(tile_base + (uint32_t)(e * 64 + lane), last)] : 0u;  // see finish
		} else {
#pragma unroll
			for (int e = 0; e < E; e++) {
				const uint64_t r = rec_src[min(tile_base + (uint32_t)(e * 64 + lane), last)];
				ra[e] = (uint32_t)r; rb[e] = (uint32_t)(r >> 32);
			}
		}
	};
	// h = upper record word (hash in bits 0 .. HB-1), p = lower record word (position in the bits of a.pos_mask): see "Sort records"
	auto finish = [&](uint32_t tile_base, const uint32_t (&ra)[E], const uint32_t (&rb)[E], uint32_t (&h)[E], uint32_t (&p)[E]) {
#pragma unroll
		for (int e = 0; e < E; e++) {
			const uint32_t idx = tile_base + (uint32_t)(e * 64 + lane);
			if (FIRST) {
				const int la = (e & 3) * 16 + (lane >> 2);  // lane holding the dword of byte idx, in register e / 4
				const uint32_t da = (uint32_t)__builtin_amdgcn_ds_bpermute(la << 2, (int)ra[e >> 2]);
				uint32_t db = (uint32_t)__builtin_amdgcn_ds_bpermute(((la + 1) & 63) << 2, (int)ra[e >> 2]);
				if ((e & 3) == 3) {  // the last lanes take the next dword from the next register's lane 0 (or from the dword after the tile)
					const uint32_t nxt = (e >> 2) + 1 < ND ? (uint32_t)__builtin_amdgcn_readfirstlane((int)ra[(e >> 2) + 1 < ND ? (e >> 2) + 1 : 0]) : ra[ND];
					if (la == 63) db = nxt;
				}
				const uint32_t sh = (uint32_t)lane & 3u;
				const uint32_t w = __builtin_amdgcn_alignbyte(db, da, sh);  // bytes idx .. idx + 3
				const uint32_t b0 = w & 255u, b1 = (w >> 8) & 255u, b2 = (w >> 16) & 255u;
				h[e] = hash3<HB>(b0, b1, b2); p[e] = idx;
				if (compact) {
					// bytes 3 and 4 -- or, for a string that starts with three equal bytes (those go to the run matcher, nobody
					// compares their bytes 3 and 4), the run-length word of the position, which saves the match kernel a scattered load
					const uint32_t b4 = (db >> (8u * sh)) & 255u;
					const uint32_t f16 = (b0 == b1 && b1 == b2) ? rb[e] : ((w >> 24) | (b4 << 8));
					h[e] |= (f16 << 15) | ((b0 >> 7) << 31); p[e] |= (b1 << 22) | (((b0 >> 5) & 3u) << 30);
				}
			}
			else { h[e] = rb[e]; p[e] = ra[e]; }
			if (idx >= npos) { h[e] = 0; p[e] = idx; }
		}
	};
	uint32_t hn[E], pn[E];
	{
		uint32_t ra[E], rb[E];
		fetch((uint32_t)(wave * 64 * E), ra, rb);
		finish((uint32_t)(wave * 64 * E), ra, rb, hn, pn);
	}
	for (uint32_t t0 = 0; t0 < npos; t0 += 1024 * E) {
		uint32_t h[E], p[E], rk[E], ra[E], rb[E];
		const uint32_t idx0 = t0 + (uint32_t)(wave * 64 * E + lane);
#pragma unroll
		for (int e = 0; e < E; e++) { h[e] = hn[e]; p[e] = pn[e]; }
		const uint32_t next_base = t0 + (uint32_t)(1024 * E + wave * 64 * E);
		fetch(next_base, ra, rb);
		for (int k = lane; k < NB; k += 64) wcnt[wave][k] = 0;
#pragma unroll
		for (int e = 0; e < E; e++) {
			const bool valid = idx0 + e * 64 < npos;
			const uint32_t d = FIRST ? (h[e] & 255u) : ((h[e] & HMASK) >> 8);
			uint64_t same = __ballot(valid);  // lanes of this round with the same digit
#pragma unroll
			for (int b = 0; b < BITS; b++) {
				const bool bit = (d >> b) & 1u;
				const uint64_t bal = __ballot(bit);
				same &= bit ? bal : ~bal;
			}
			const uint32_t rank = (uint32_t)__popcll(same & lt_mask);
			uint32_t before = 0;
			if (valid) {
				before = wcnt[wave][d];  // equal digits of this wave's earlier rounds
				if (rank == 0) wcnt[wave][d] = before + (uint32_t)__popcll(same);
			}
			rk[e] = before + rank;
		}
		lds_barrier();
		if (tid < NB) {  // running offset of digit tid, handed out wave by wave
			uint32_t c[16], run = offs[tid];
#pragma unroll
			for (int w = 0; w < 16; w++) c[w] = wcnt[w][tid];
#pragma unroll
			for (int w = 0; w < 16; w++) { wcnt[w][tid] = run; run += c[w]; }
			offs[tid] = run;
		}
		lds_barrier();
#pragma unroll
		for (int e = 0; e < E; e++) asm volatile("" : "+v"(ra[e]), "+v"(rb[e]) :: "memory");
		finish(next_base, ra, rb, hn, pn);
#pragma unroll
		for (int e = 0; e < E; e++) {
			if (idx0 + e * 64 < npos) {
				const uint32_t d = FIRST ? (h[e] & 255u) : ((h[e] & HMASK) >> 8);
				const uint32_t dst = wcnt[wave][d] + rk[e];
				rec_dst[dst] = (uint64_t)p[e] | ((uint64_t)h[e] << 32);
			}
		}
	}
}

// ------------------------------------------------------------------ 2. longest_match for every position
// The chain of sorted index i = sorted entries i-1, i-2, ... of the same hash (deflate.c:1236-1386).
// Pass A: one lane per position walks at most LIGHT_STEPS candidates; positions whose chain is
// longer ("heavy": long runs of one byte put tens of thousands of strings in one bucket) are queued.
// Pass B: one WAVE per heavy position, 64 candidates per step.
constexpr int LIGHT_STEPS = 12;  // below max_chain at every level (16 .. 4096): the light walk never reaches the chain limit

// Block -> (slice, part) for the kernels that touch one slice's arrays at random (hash order): match records
// are scattered 8-byte stores and the string loads are scattered too, so they only stay on chip if the whole
// working set of a slice (~3 MB) sits in ONE L2 while it is being processed.  Blocks are dealt round-robin
// over the 8 XCDs (observed behaviour, used for speed only): blocks lin and lin + 8 share an L2, so the blocks
// with lin % 8 == c walk through slices c, c + 8, c + 16, ... one after the other.  gridDim.y is n rounded up to 8.
__device__ __forceinline__ bool xcd_slice(int n, int &s, uint32_t &part, uint32_t &nparts)
{
	const uint32_t lin = blockIdx.x + gridDim.x * blockIdx.y;
	const uint32_t c = lin & 7u, k = lin >> 3;
	nparts = gridDim.x;
	s = (int)(8u * (k / nparts) + c);
	part = k % nparts;
	return s < n;
}

__device__ __forceinline__ uint32_t nil_candidate(uint32_t p, uint32_t lookahead)
{
	// slide_hash NIL quirk at the very end of the input (see oracle/deflate_model.c)
	return (lookahead < (uint32_t)MIN_LOOKAHEAD && p >= 32506u + 32768u && (p - 32506u) % 32768u == 0) ? p - 32506u : 0xFFFFFFFFu;
}

// ------------------------------------------------------------------ 1b. run length ahead of every position
// run_len[p] = number of bytes equal to in[p] starting at p, capped at MAX_MATCH (and by the end of the input),
// with bit 15 = (p >= 2 && in[p-1] == in[p]).  The match kernels visit positions in hash order, where
// scanning the bytes would be a chain of uncoalesced loads; here the input is read once, in order.
// A workgroup scans 2048 positions (8 per lane) and publishes the first RUNLEN_OUT of them (deflate_workspace.h): for those
// the scanned tail (>= 264 bytes) decides every length below the cap.

// SORT = false (the Z_RLE pass): run-length words only, without the sort histograms and run-list counts nobody reads there.
// HB: hash bits (15 or 16, memLevel 8 or 9)
template <bool SORT, int HB>
__global__ void __launch_bounds__(256) dfl_run_len_kernel(DeflateArgs a)
{
	constexpr int NH = 256 + (1 << (HB - 8));  // hash & 255, then hash >> 8
	__shared__ uint32_t wtot[4];  // per wave: has_change << 31 | distance from the wave's first position to its first change
	__shared__ uint32_t hist[SORT ? NH : 1];  // digits of the sort: hash & 255 of every string of this workgroup's positions, then hash >> 8
	if (SORT) for (int t = threadIdx.x; t < NH; t += 256) hist[t] = 0;
	__syncthreads();
	const int s = blockIdx.y;
	const uint32_t L = a.in_sizes[s];
	const uint8_t *in = a.in + (size_t)s * a.in_stride;
	uint16_t *rl = a.run_len + (size_t)s * a.in_stride;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t nchunks = (L + RUNLEN_OUT - 1) / RUNLEN_OUT;
	for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
		const uint32_t c0 = c * RUNLEN_OUT;
		const uint32_t g = c0 + threadIdx.x * 8;  // first of this lane's 8 positions
		uint8_t b[12];                            // in[g-1 .. g+10]
		if (g + 12 <= L && g >= 1) {
			uint64_t w;
			__builtin_memcpy(&w, in + g, 8);
#pragma unroll
			for (int k = 0; k < 8; k++) b[k + 1] = (uint8_t)(w >> (8 * k));
			b[0] = in[g - 1];
			uint32_t w2; __builtin_memcpy(&w2, in + g + 8, 4);
			b[9] = (uint8_t)w2; b[10] = (uint8_t)(w2 >> 8); b[11] = (uint8_t)(w2 >> 16);
		} else {
#pragma unroll
			for (int k = 0; k < 12; k++) { const int64_t y = (int64_t)g - 1 + k; b[k] = (y >= 0 && y < (int64_t)L) ? in[y] : 0; }
		}
		// the sort's digit histograms (UPDATE_HASH of the three bytes from every published position that starts a string).
		// A quarter of a CT payload is runs of one byte: a lane whose strings all hash alike adds them in one go, and so does
		// a wave (every lane adding 1 to the same two counters made this kernel 0.31 instead of 0.09 ms)
		if (SORT) {
			uint32_t hk[8], cnt = 0, h0 = 0;
			bool same = true;
#pragma unroll
			for (int k = 0; k < 8; k++) {
				const bool v = threadIdx.x * 8 + k < (uint32_t)RUNLEN_OUT && g + k + 2 < L;
				hk[k] = v ? hash3<HB>(b[k + 1], b[k + 2], b[k + 3]) : 0xFFFFFFFFu;
				if (v) { if (!cnt) h0 = hk[k]; else same &= hk[k] == h0; cnt++; }
			}
			const bool wave_same = __all(same && cnt == 8 && h0 == (uint32_t)__builtin_amdgcn_readfirstlane((int)h0));
			if (wave_same) {
				if (lane == 0) { atomicAdd(&hist[h0 & 255u], 512u); atomicAdd(&hist[256u + (h0 >> 8)], 512u); }
			} else if (same) {
				if (cnt) { atomicAdd(&hist[h0 & 255u], cnt); atomicAdd(&hist[256u + (h0 >> 8)], cnt); }
			} else {
#pragma unroll
				for (int k = 0; k < 8; k++)
					if (hk[k] != 0xFFFFFFFFu) { atomicAdd(&hist[hk[k] & 255u], 1u); atomicAdd(&hist[256u + (hk[k] >> 8)], 1u); }
			}
		}
		uint32_t chg = 0;  // bit k: the run containing position g+k ends at g+k
#pragma unroll
		for (int k = 0; k < 8; k++) chg |= (uint32_t)(b[k + 1] != b[k + 2] || g + k + 1 >= L) << k;
		// suffix scan over lanes of (has_change, distance to first change): spans combine as
		//   (cA, nA) . (cB, nB) = (cA | cB, cA ? nA : nA + nB)       with n = 8 * span for a change-free span
		uint32_t hc = chg != 0, n = hc ? (uint32_t)__ffs((int)chg) - 1u : 8u;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t hb = (uint32_t)__shfl_down((int)hc, d, 64), nb = (uint32_t)__shfl_down((int)n, d, 64);
			if (lane + d < 64 && !hc) { n += nb; hc = hb; }
		}
		__syncthreads();  // wtot of the previous chunk has been read by everyone
		if (lane == 0) wtot[wave] = (hc << 31) | n;
		__syncthreads();
		uint32_t xh = 0, xn = 0;  // the waves after this one
		for (int w = 3; w > wave; w--) {
			const uint32_t t = wtot[w];
			if (t >> 31) { xh = 1; xn = t & 0x7FFFFFFFu; } else xn += t & 0x7FFFFFFFu;
		}
		if (!xh) xn += 1024;  // nothing scanned beyond: only reached by positions that are not published
		const uint32_t nfull = hc ? n : n + xn;  // distance from g to the first change at or after g
		uint32_t nnext = (uint32_t)__shfl_down((int)nfull, 1, 64);  // the same for g + 8
		if (lane == 63) nnext = xn;
		uint16_t out[8];
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const uint32_t rest = chg >> k;
			uint32_t r = rest ? (uint32_t)__ffs((int)rest) : (8u - k) + nnext + 1u;
			if (r > (uint32_t)MAX_MATCH) r = MAX_MATCH;
			out[k] = (uint16_t)(r | ((g + k >= 2 && b[k] == b[k + 1]) ? 0x8000u : 0u));
		}
		if (threadIdx.x * 8 < (uint32_t)RUNLEN_OUT && g < L) {
			if (g + 8 <= L && threadIdx.x * 8 + 8 <= (uint32_t)RUNLEN_OUT) __builtin_memcpy(rl + g, out, 16);
			else {
#pragma unroll
				for (int k = 0; k < 8; k++) if (g + k < L && threadIdx.x * 8 + k < (uint32_t)RUNLEN_OUT) rl[g + k] = out[k];
			}
		}
		// entries this chunk contributes to the lists of run ends and run starts (dfl_run_lists_kernel): position p ends a run of
		// >= 3 three bytes on (exactly three equal bytes from p, the fourth inside the input) and starts one when >= 3 equal bytes
		// follow and the byte before differs
		if (SORT) {
			// from the "changes after this byte" bits of in[g-1 .. g+9] (bit i: in[g-1+i] != in[g+i], or the right byte is past the
			// end, or -- bit 0 -- there is no byte before position 0): position p = g+k, pair p <-> bit k+1
			uint32_t cx = g == 0 ? 1u : 0u;
#pragma unroll
			for (int i = 0; i < 11; i++) cx |= (uint32_t)(b[i] != b[i + 1] || g + (uint32_t)i >= L) << i;
			const uint32_t t8 = threadIdx.x * 8;
			const uint32_t npub = t8 < (uint32_t)RUNLEN_OUT ? min(min(8u, (uint32_t)RUNLEN_OUT - t8), g < L ? L - g : 0u) : 0u;  // published positions of the lane
			const uint32_t pubm = (1u << npub) - 1u;
			const uint32_t ne3 = g + 3 < L ? min(8u, L - 3u - g) : 0u;                 // positions with p + 3 < L
			const uint32_t run3 = ~(cx >> 1) & ~(cx >> 2);                             // three equal bytes from p
			const uint32_t me = run3 & (cx >> 3) & pubm & ((1u << ne3) - 1u);          // ... and the fourth differs, inside the input
			const uint32_t ms = run3 & cx & pubm;                                      // ... and the byte before differs
			uint32_t ce = 0, cs = 0;  // wave totals; run boundaries are rare (inside a long run there is none): most waves skip this
			if (__any((me | ms) != 0)) { ce = wave_sum((uint32_t)__popc(me)); cs = wave_sum((uint32_t)__popc(ms)); }
			if (lane == 0 && (ce | cs)) {  // (counters zeroed with the sort histograms: no barrier, no store where there is no run)
				uint32_t *cnt = a.run_counts + (size_t)s * 2 * a.run_chunks;
				if (ce) atomicAdd(&cnt[2 * c], ce);
				if (cs) atomicAdd(&cnt[2 * c + 1], cs);
			}
		}
	}
	if (!SORT) return;
	__syncthreads();
	for (int t = threadIdx.x; t < NH; t += 256)
		if (hist[t]) atomicAdd(&a.sort_hist[(size_t)s * SORT_HIST + t], hist[t]);
}

// length of the common prefix of x and y, continuing from len, capped at cap; 8 bytes per step
__device__ __forceinline__ int common_prefix(const uint8_t *x, const uint8_t *y, int len, int cap)
{
	while (len + 8 <= cap) {
		uint64_t u, v;
		__builtin_memcpy(&u, x + len, 8);
		__builtin_memcpy(&v, y + len, 8);
		const uint64_t d = u ^ v;
		if (d) return len + ((__ffsll((long long)d) - 1) >> 3);
		len += 8;
	}
	while (len < cap && x[len] == y[len]) len++;
	return len;
}

// Sort records.  Wide (any slice size): position | hash << 32.  Compact (slices below 4 MiB, a.pos_mask = 2^22 - 1): the record
// also identifies the first five bytes b0..b4 of its string,
//   lower word: position (22 bits) | b1 << 22 | (b0 >> 5 & 3) << 30        upper word: hash (15 bits) | b3 << 15 | b4 << 23 | (b0 >> 7) << 31
// Two strings of one bucket start with the same three bytes exactly when b1 and the top three bits of b0 agree (the hash then
// pins b2 and the rest of b0), so the match kernel decides every candidate whose match is shorter than five bytes -- nearly all
// of them on token payloads -- from the records alone, which are read in sorted order (coalesced); before, every position paid
// a scattered load for its own string and one per candidate.  Compact records exist at memLevel 8 only: the 16-bit hash of
// memLevel 9 would leave four top bits of b0 unpinned, and the record has no bit to spare.  A wide record's upper word is the
// hash alone (15 or 16 bits).
__device__ __forceinline__ uint32_t rec_hash(uint64_t r, uint32_t pos_mask)
{
	return (uint32_t)(r >> 32) & (pos_mask == 0xFFFFFFFFu ? 0xFFFFFFFFu : 0x7FFFu);
}
__device__ __forceinline__ uint32_t rec_pos(uint64_t r, uint32_t pos_mask) { return (uint32_t)r & pos_mask; }
constexpr uint32_t COMPACT_POS_BITS = 22, COMPACT_POS_MASK = (1u << COMPACT_POS_BITS) - 1u;

// longest_match over at most LIGHT_STEPS chain entries, strings read from the input (wide records, and the last seven positions
// of a slice with compact ones).  kind: 0 = best/best_q (full chain) and best1/best_q1 (the first `quarter` entries) hold the
// result, 1 = heavy (longer chain), 2 = starts a run (run_r).
__device__ __forceinline__ void light_match_from_memory(const uint8_t *in, const uint64_t *recs, const uint16_t *rl, uint32_t pos_mask,
                                                        uint32_t L, uint32_t i, uint32_t p, uint32_t h, uint32_t nice, int quarter,
                                                        int &kind, int &best, uint32_t &best_q, int &best1, uint32_t &best_q1,
                                                        uint32_t &run_r)
{
	const uint32_t lookahead = L - p;
	const int max_len = lookahead < (uint32_t)MAX_MATCH ? (int)lookahead : MAX_MATCH;
	const int nice_eff = (int)min(lookahead, nice);  // nice_match clamped to the lookahead (<= max_len)
	const uint32_t nil_q = nil_candidate(p, lookahead);
	int count = 0;
	const uint8_t *sp = in + p;
	// strings that START a run of three equal bytes share one bucket with every other position of
	// every run of that byte (tens of thousands of entries); dfl_match_run_kernel evaluates them from
	// the list of run ends instead of walking the chain
	// the first 8 bytes of the string decide most things; in hash order every access to the slice is its own
	// L2 transaction, so the run-length word is only fetched for the strings that need it
	const bool wide = p + 8 <= L;  // then max_len >= 8 and sp[0..7] is inside the input
	uint64_t ow = 0;
	if (wide) __builtin_memcpy(&ow, sp, 8);
	const bool in_run = wide ? (((ow >> 8) ^ ow) & 0xFFFFu) == 0 : (sp[1] == sp[0] && sp[2] == sp[0]);
	if (in_run) {
		const uint32_t rw = rl[p];
		run_r = rw & 0x7FFFu;  // >= 3, <= max_len by construction
		if ((rw >> 15) && (int)run_r >= nice_eff) { best = best1 = (int)run_r; best_q = best_q1 = p - 1; }  // chain head p-1 yields r: the walk ends there
		else kind = 2;
		return;
	}
	for (int64_t j = (int64_t)i - 1; j >= 0; j--) {
		const uint64_t rj = recs[j];
		if (rec_hash(rj, pos_mask) != h) break;
		if (count == LIGHT_STEPS) { kind = 1; break; }           // heavy: finish cooperatively
		const uint32_t q = rec_pos(rj, pos_mask);
		const uint32_t dist = p - q;
		if (q == 0 || q == nil_q) break;                         // NIL ends the chain
		if (count == 0 ? dist > (uint32_t)MAX_DIST : dist >= (uint32_t)MAX_DIST) break;
		const uint8_t *mp = in + q;
		{                                                        // (best < nice_eff here: the walk ends when it is reached)
			int len = 0;
			if (wide) {  // one 8-byte load decides most candidates (the loads of mp are the uncoalesced ones)
				if (best < 8 || mp[best] == sp[best]) {
					uint64_t cw;
					__builtin_memcpy(&cw, mp, 8);
					const uint64_t d = cw ^ ow;
					len = d ? (__ffsll((long long)d) - 1) >> 3 : common_prefix(mp, sp, 8, max_len);
				}
			} else if (mp[best] == sp[best]) len = common_prefix(mp, sp, 0, max_len);
			if (len > best) {
				best = len; best_q = q;
				if (count < quarter) { best1 = len; best_q1 = q; }  // still inside the first max_chain >> 2 entries
			}
		}
		count++;
		if (best >= nice_eff) break;                             // len >= nice_match: the first such entry ends the walk
	}
}

// QL: the quarter chain (max_chain >> 2) ends inside the light walk (levels 4 and 5), so the lane records it on its own;
// otherwise the light walk never gets past it and the quarter record is the full one.
//
// Time: the kernel is bound by neither its instructions nor its bytes: its waves are parked two thirds of their life
// (DESIGN.md 5), so a turn leaves as few round trips on its path as it can, and a wave makes many turns (launch_deflate), since
// its entry (a chain of scalar loads, the first records) and its last flush are the part that nothing overlaps.
//  - The records of the wave's NEXT turn are requested before this turn's chain walk and waited for at the top of the next
//    turn (same clamped addresses as the turn itself would use: past the last turn they re-read records below npos).
//  - Queued positions (kind 1 and 2) collect in a region of LDS that the wave owns (no barrier: LDS traffic of one wave keeps
//    program order) with the two counts in registers.  A list is flushed after the wave's last turn, and earlier whenever fewer
//    than 64 entries of its region are free: one returning atomicAdd of the whole count, then contiguous stores.  Before, lane 0
//    paid two returning atomics on the slice's two counters in every turn, behind the turn's scattered stores.
//    The order of the entries in the two lists depended on which wave's atomic won before and does now; dfl_match_heavy_kernel
//    and dfl_match_run_kernel treat every entry on its own, so the bytes of the result do not depend on it.
// MATCH_Q entries per wave and list: 2 KiB * MATCH_Q / 256 per wave, 8 KiB per workgroup at 256, and eight workgroups of a CU
// hold 64 of its 160 KiB: the 8 waves per SIMD that the registers allow stay.
#ifndef DFL_MATCH_Q
#define DFL_MATCH_Q 256
#endif
#ifndef DFL_MATCH_GRID
#define DFL_MATCH_GRID 32  // workgroups per slice with compact records, at least (launch_deflate)
#endif
constexpr uint32_t MATCH_Q = DFL_MATCH_Q;
static_assert(MATCH_Q >= 128 && (MATCH_Q & 63) == 0, "a turn appends up to 64 entries to a list");

template <bool CMP, bool QL>
__global__ void __launch_bounds__(256) dfl_match_kernel(DeflateArgs a, int n)
{
	__shared__ uint32_t queue[4][2][MATCH_Q];  // [wave][0 heavy, 1 run]
	int s; uint32_t part, nparts;
	if (!xcd_slice(n, s, part, nparts)) return;
	const uint32_t L = a.in_sizes[s], gen = *a.gen;  // (both requested at entry, neither behind the other)
	const uint8_t *in = a.in + (size_t)s * a.in_stride;
	const size_t base = (size_t)s * a.in_stride;
	const uint32_t npos = L >= MIN_MATCH ? L - 2 : 0;
	const uint64_t *recs = a.rec_out + base;  // sorted records, see "Sort records"
	uint2 *mr = reinterpret_cast<uint2 *>(a.mr) + base;
	uint32_t *heavy = a.heavy_list + base;
	const uint16_t *rl = a.run_len + base;
	const int lane = threadIdx.x & 63;
	const uint64_t lt_mask = (1ull << lane) - 1ull;
	const int quarter = QL ? (int)(a.max_chain >> 2) : LIGHT_STEPS + 1;
	const uint32_t stride = nparts * 256u;
	uint32_t i0 = part * 256u;
	if (i0 >= npos) return;  // (the whole workgroup: nothing to read, nothing queued)
	uint32_t *qh = queue[threadIdx.x >> 6][0], *qr = queue[threadIdx.x >> 6][1];
	uint32_t nh = 0, nr = 0;  // entries waiting in qh / qr (wave-uniform)
	// lane l takes entry l, l + 64, ...; the heavy list grows upwards, the run list downwards from the end
	auto flush = [&](const uint32_t *q, uint32_t cnt, uint32_t *counter, bool down) {
		uint32_t b = 0;
		if (lane == 0) b = atomicAdd(counter, cnt);
		b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
		__builtin_amdgcn_wave_barrier();  // one wave: LDS order is program order; keep the compiler to it as well
		for (uint32_t k = (uint32_t)lane; k < cnt; k += 64u) {
			if (down) *(dfl_deep_top(heavy, a.in_stride) - (b + k)) = q[k];
			else heavy[b + k] = q[k];
		}
		__builtin_amdgcn_wave_barrier();
	};
	// sorted index i and, with compact records, i - 64 (lane l: index (wave's first) + l - 64, unused where that is negative)
	auto rec_at = [&](uint32_t i) { return recs[min(i, npos - 1)]; };
	auto rec_before = [&](uint32_t i) { return recs[min(i >= 64 ? i - 64 : 0u, npos - 1)]; };
	uint64_t ri_next = rec_at(i0 + threadIdx.x), rb_next = CMP ? rec_before(i0 + threadIdx.x) : 0ull;
	for (; i0 < npos; i0 += stride) {  // wave-uniform trip count
		const uint32_t i = i0 + threadIdx.x;
		const bool valid = i < npos;
		int kind = 0;  // 0: record written, 1: queue for the cooperative heavy pass, 2: queue for the run pass
		int best = 0, best1 = 0;
		uint32_t best_q = 0, best_q1 = 0, run_r = 0;
		const uint64_t ri = ri_next, rb = rb_next;
		ri_next = rec_at(i + stride);
		if (CMP) rb_next = rec_before(i + stride);
		const uint32_t p = rec_pos(ri, CMP ? COMPACT_POS_MASK : 0xFFFFFFFFu);
		const uint32_t h = rec_hash(ri, CMP ? COMPACT_POS_MASK : 0xFFFFFFFFu);
		bool from_memory = valid;
		bool found = false;  // something to store (see MatchRec)
		if (CMP) {
			// The chain of sorted index i is i-1, i-2, ...: the records of the lanes below, then of the 64 indices before the wave.
			// Both sit in registers (one coalesced load each) and move up one lane per step, so a step waits for nothing; with
			// one load per step a wave paid a memory round trip for every entry of its longest chain.
			const uint32_t lo_i = (uint32_t)ri, hi_i = (uint32_t)(ri >> 32), lo_b = (uint32_t)rb, hi_b = (uint32_t)(rb >> 32);
			const uint32_t lookahead = L - p;
			const int max_len = lookahead < (uint32_t)MAX_MATCH ? (int)lookahead : MAX_MATCH;
			const int nice_eff = (int)min(lookahead, a.nice);  // nice_match clamped to the lookahead (<= max_len)
			const bool fast = valid && p + 8 <= L;  // max_len >= 8; the compact fields of the record are those of the string
			from_memory = valid && !fast;
			const uint32_t nil_q = nil_candidate(p, lookahead);
			const uint32_t b1 = (lo_i >> 22) & 255u;
			const bool in_run = h == (((b1 << 10) ^ (b1 << 5) ^ b1) & 0x7FFFu) && (((lo_i >> 30) | ((hi_i >> 31) << 2)) == (b1 >> 5));
			if (fast && in_run) {  // the record carries the run-length word in place of bytes 3 and 4
				const uint32_t rw = (hi_i >> 15) & 0xFFFFu;
				run_r = rw & 0x7FFFu;
				if (!((rw >> 15) && (int)run_r >= nice_eff)) kind = 2;
				else if ((int)run_r < max_len) { best = best1 = (int)run_r; best_q = best_q1 = p - 1; found = true; }  // chain head p-1 reaches nice
				// (else: chain head p-1 at the cap, which the parse knows from the run-length word, checked_match)
			}
			bool act = fast && !in_run;
			// NIL (position 0, and the slide_hash quirk, which sits at distance MAX_DIST exactly) and the window as one bound on the
			// candidate's position: the chain head may be MAX_DIST away, later entries must be closer
			const uint32_t qmin_head = (p > (uint32_t)MAX_DIST ? p - (uint32_t)MAX_DIST : 1u) + (nil_q != 0xFFFFFFFFu ? 1u : 0u);  // (nil_q, when there is one, is p - MAX_DIST)
			const uint32_t qmin_rest = p >= (uint32_t)MAX_DIST ? p - (uint32_t)MAX_DIST + 1u : 1u;
			const uint32_t steps_i = min(i, (uint32_t)LIGHT_STEPS + 1u);  // chain entries that exist at all
			uint32_t clo = lo_i, chi = hi_i;
#pragma unroll
			for (int k = 1; k <= LIGHT_STEPS + 1; k++) {
				// candidate i - k: shift the records up one lane, lane 0 takes index (wave's first) - k from the second register
				clo = wave_shift_up(clo, (uint32_t)__builtin_amdgcn_readlane((int)lo_b, 64 - k));
				chi = wave_shift_up(chi, (uint32_t)__builtin_amdgcn_readlane((int)hi_b, 64 - k));
				if (!__any(act)) break;
				const uint32_t x = hi_i ^ chi;
				const uint32_t q = clo & COMPACT_POS_MASK;
				// the chain ends: before the first record, at another hash, at NIL / outside the window
				if ((uint32_t)k > steps_i || (x & 0x7FFFu) != 0 || q < (k == 1 ? qmin_head : qmin_rest)) act = false;
				if (act) {
					if (k == LIGHT_STEPS + 1) { kind = 1; act = false; }  // a 13th entry: heavy
					else {
						// three bytes in common (less never counts): then x holds the differences of bytes 3 and 4 only
						if (best < nice_eff && (((lo_i ^ clo) >> 22) | (x >> 31)) == 0) {
							int len;
							if (x & 0x007F8000u) len = 3;
							else if (x) len = 4;
							else if (best < 5 || in[q + best] == in[p + best]) len = common_prefix(in + q, in + p, 5, max_len);
							else len = 0;
							if (len > best) {
								best = len; best_q = q; found = true;
								if (QL && k <= quarter) { best1 = len; best_q1 = q; }
							}
						}
						if (best >= nice_eff) act = false;  // len >= nice_match: the first such entry ends the walk
					}
				}
			}
		}
		if (from_memory) {
			light_match_from_memory(in, recs, rl, CMP ? COMPACT_POS_MASK : 0xFFFFFFFFu, L, i, p, h, a.nice, quarter, kind, best, best_q,
			                        best1, best_q1, run_r);
			found = kind == 0 && best >= MIN_MATCH;
		}
		if (found && kind == 0) {  // shorter than MIN_MATCH never counts (match_of); queued positions are written by their kernels
			if (!QL) { best1 = best; best_q1 = best_q; }
			mr[p] = pack_match((uint32_t)best, (uint32_t)best1, p - best_q, best1 ? p - best_q1 : 0u, gen);
		}
		// queued positions go to the wave's regions (at least 64 entries of each are free here)
		const uint64_t bh = __ballot(kind == 1), br = __ballot(kind == 2);
		if (kind == 1) qh[nh + (uint32_t)__popcll(bh & lt_mask)] = i;
		if (kind == 2) qr[nr + (uint32_t)__popcll(br & lt_mask)] = i;
		nh += (uint32_t)__popcll(bh); nr += (uint32_t)__popcll(br);
		if (nh > MATCH_Q - 64u) { flush(qh, nh, &a.heavy_count[s], false); nh = 0; }
		if (nr > MATCH_Q - 64u) { flush(qr, nr, &a.deep_count[s], true); nr = 0; }
	}
	if (nh) flush(qh, nh, &a.heavy_count[s], false);
	if (nr) flush(qr, nr, &a.deep_count[s], true);
}

// Wave-cooperative longest_match for one position whose chain is long: 64 candidates per step, at most max_chain in all.
// Returns the packed MatchRec (lo = len_full | len_quarter << 16, hi = dist_full | dist_quarter << 16), wave-uniform.
// In chain order the walk ends at the first entry whose length reaches nice_eff, so in a step that is the lowest such lane and
// no later lane counts; the quarter walk is the prefix of the first max_chain >> 2 entries (4, 8, 32 of them at levels 4 to 6:
// inside the first step).
__device__ __forceinline__ void coop_longest_match(const uint8_t *in, const uint64_t *recs, uint32_t L,
                                                   uint32_t i, uint32_t p, uint32_t pos_mask, int lane, uint32_t nice, uint32_t max_chain,
                                                   uint32_t &lo, uint32_t &hi)
{
	const uint32_t h = rec_hash(recs[i], pos_mask);
	const uint32_t lookahead = L - p;
	const int max_len = lookahead < (uint32_t)MAX_MATCH ? (int)lookahead : MAX_MATCH;
	const int nice_eff = (int)min(lookahead, nice);  // nice_match clamped to the lookahead (<= max_len)
	const uint32_t quarter = max_chain >> 2;
	const int steps = (int)((max_chain + 63) >> 6);
	const uint32_t nil_q = nil_candidate(p, lookahead);
	const uint8_t *sp = in + p;
	int best = 0;
	uint32_t best_q = 0;
	int len_q = -1;
	uint32_t q_q = 0;
	// longest length among the lanes of `cand`, earliest candidate (lowest lane) that reaches it
	auto pick = [&](uint64_t cand, int len, uint32_t q, int &b_len, uint32_t &b_q) {
		for (int b = 8; b >= 0; b--) {
			const uint64_t mb = __ballot((len >> b) & 1) & cand;
			if (mb) cand = mb;
		}
		const int win = __builtin_amdgcn_readfirstlane(__ffsll((long long)cand) - 1);
		b_len = __builtin_amdgcn_readlane(len, win);
		b_q = (uint32_t)__builtin_amdgcn_readlane((int)q, win);
	};
	auto rec_of_round = [&](int r) { const int64_t j = (int64_t)i - 1 - (int64_t)(r * 64 + lane); return recs[j >= 0 ? j : 0]; };
	uint64_t rj_next = rec_of_round(0);
	for (int r = 0; r < steps; r++) {
		const int64_t j = (int64_t)i - 1 - (int64_t)(r * 64 + lane);
		const uint64_t rj = j >= 0 ? rj_next : ~0ull;
		rj_next = rec_of_round(r + 1);  // (requested before this round's strings are compared)
		const bool in_chain = j >= 0 && rec_hash(rj, pos_mask) == h && (uint32_t)(r * 64 + lane) < max_chain;
		const uint32_t q = in_chain ? rec_pos(rj, pos_mask) : 0u;
		const uint32_t dist = p - q;
		const bool term = !in_chain || q == 0 || q == nil_q ||
		                  ((r == 0 && lane == 0) ? dist > (uint32_t)MAX_DIST : dist >= (uint32_t)MAX_DIST);
		const uint64_t tmask = __ballot(term);
		const int nvalid = tmask ? (__ffsll((long long)tmask) - 1) : 64;
		int len = 0;
		if (lane < nvalid) {  // (best < nice_eff here: the walk ends when it is reached)
			const uint8_t *mp = in + q;
			if (mp[best] == sp[best]) len = common_prefix(mp, sp, 0, max_len);
		}
		const uint64_t nice_m = __ballot(len >= nice_eff);
		const uint64_t upto = nice_m ? ((nice_m & (0 - nice_m)) << 1) - 1u : ~0ull;  // lanes up to the first that reaches nice
		const int best_before = best;
		const uint32_t best_q_before = best_q;
		const uint64_t cand = __ballot(len > best_before) & upto;
		if (cand) pick(cand, len, q, best, best_q);
		const uint32_t qb = quarter - (uint32_t)(r * 64);  // the quarter walk ends inside this step, after lane qb - 1
		if ((uint32_t)(r * 64) < quarter && qb <= 64u) {
			const uint64_t cq = cand & (qb == 64u ? ~0ull : (1ull << qb) - 1u);
			if (cq == cand) { len_q = best; q_q = best_q; }
			else if (cq) pick(cq, len, q, len_q, q_q);
			else { len_q = best_before; q_q = best_q_before; }
		}
		if (nice_m || nvalid < 64) break;
	}
	if (len_q < 0) { len_q = best; q_q = best_q; }
	lo = (uint32_t)best | ((uint32_t)len_q << 16);
	hi = (best ? p - best_q : 0u) | ((len_q ? p - q_q : 0u) << 16);
}

__global__ void __launch_bounds__(256) dfl_match_heavy_kernel(DeflateArgs a, int n)
{
	int s; uint32_t part, nparts;
	if (!xcd_slice(n, s, part, nparts)) return;
	const uint32_t L = a.in_sizes[s];
	const uint8_t *in = a.in + (size_t)s * a.in_stride;
	const size_t base = (size_t)s * a.in_stride;
	const uint64_t *recs = a.rec_out + base;  // sorted (hash, position) records: position | hash << 32
	uint2 *mr = reinterpret_cast<uint2 *>(a.mr) + base;
	const uint32_t *heavy = a.heavy_list + base;
	const uint32_t nheavy = a.heavy_count[s];
	const int lane = threadIdx.x & 63;
	const uint32_t gen = *a.gen;
	for (uint32_t e = part * (blockDim.x >> 6) + (threadIdx.x >> 6); e < nheavy; e += nparts * (blockDim.x >> 6)) {
		const uint32_t i = heavy[e];
		const uint32_t p = rec_pos(recs[i], a.pos_mask);
		uint32_t lo, hi;
		coop_longest_match(in, recs, L, i, p, a.pos_mask, lane, a.nice, a.max_chain, lo, hi);
		if (lane == 0) mr[p] = pack_match(lo & 0xFFFFu, lo >> 16, hi & 0xFFFFu, hi >> 16, gen);
	}
}

// ------------------------------------------------------------------ 2c. positions deep inside a run of one byte
// For p with in[p-3..p+2] all equal to b and r further b's ahead (r < max_len), the chain head is p-1
// and yields exactly r.  Only a candidate q that is r bytes before the END of an earlier run of b,
// followed by the same byte c = in[p+r], can be longer.  So instead of max_chain chain steps the lane scans
// the (much shorter) list of run ends backwards.  Chain-length limits translate into position limits
// through the sorted order: the first K chain entries are the sorted indices i-1 .. i-K.
// Ordered lists of the ends AND starts of runs of >= 3 equal bytes, per slice, from the run-length words: position p puts
// p + 3 on the list of ends when exactly three equal bytes start at p and the fourth byte lies inside the input, and p on the
// list of starts when >= 3 equal bytes start at p and the byte before differs.  dfl_run_len_kernel has counted the entries of
// every chunk of RUNLEN_OUT positions; a workgroup sums the counts of the chunks before its own and writes its entries at that
// offset (a workgroup prefix sum places them, so both lists come out in position order); dfl_run_info_kernel pairs the k-th
// start with the k-th end (run length without scanning).  Until round 3 one workgroup per slice walked its 8192-byte
// chunks in a row, computing the flags byte by byte (0.18 ms per batch).
// Buffer (in_stride words of its own, at most L/4 runs): ends, starts, length|byte<<16 and the rank of every eighth position
// among the ends, a quarter each (deflate_workspace.h: dfl_run_starts, dfl_run_info, dfl_run_rank).
__global__ void __launch_bounds__(256) dfl_run_lists_kernel(DeflateArgs a)
{
	__shared__ uint32_t wsum[4], base_es[2];
	const int s = blockIdx.y;
	const uint32_t L = a.in_sizes[s];
	const uint32_t c = blockIdx.x;
	const uint32_t c0 = c * RUNLEN_OUT;
	if (c0 >= L) return;
	const uint8_t *in = a.in + (size_t)s * a.in_stride;
	const uint16_t *rl = a.run_len + (size_t)s * a.in_stride;
	uint32_t *re = a.run_ends + (size_t)s * a.in_stride;
	uint32_t *rs = dfl_run_starts(re, a.in_stride);
	const uint32_t *cnt = a.run_counts + (size_t)s * 2 * a.run_chunks;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t g = c0 + (uint32_t)tid * 8;
	// the lane's eight run-length words: one aligned 16-byte load (g is a multiple of 8; in_stride a multiple of 256)
	uint4 wv = make_uint4(0, 0, 0, 0);
	if (tid * 8 < RUNLEN_OUT && g < L) wv = *reinterpret_cast<const uint4 *>(rl + g);
	const bool first_two_equal = L >= 2 && in[0] == in[1];  // the "same as before" bit of a word is only kept from position 2 on
	if (wave == 0) {  // entries of the chunks before this one
		uint32_t be = 0, bs = 0;
		for (uint32_t q = lane; q < c; q += 64) { be += cnt[2 * q]; bs += cnt[2 * q + 1]; }
		be = wave_sum(be); bs = wave_sum(bs);
		if (lane == 0) { base_es[0] = be; base_es[1] = bs; }
	}
	const uint32_t w32[4] = {wv.x, wv.y, wv.z, wv.w};
	uint32_t me = 0, ms = 0;
#pragma unroll
	for (int k = 0; k < 8; k++) {
		const uint32_t w = (w32[k >> 1] >> (16 * (k & 1))) & 0xFFFFu, r = w & 0x7FFFu, p = g + (uint32_t)k;
		const bool pub = (uint32_t)tid * 8 + k < (uint32_t)RUNLEN_OUT && p < L;
		const bool prev_eq = p >= 2 ? (w >> 15) != 0 : (p == 1 && first_two_equal);
		me |= (uint32_t)(pub && r == 3u && p + 3 < L) << k;
		ms |= (uint32_t)(pub && r >= 3u && !prev_eq) << k;
	}
	// both counts in one scan: a workgroup has at most 8 * 256 = 2048 of either (its first barrier also publishes base_es)
	uint32_t tot;
	const uint32_t ex = wg_excl_scan<4>((uint32_t)__popc(me) | (uint32_t)__popc(ms) << 16, wsum, tot);
	uint32_t ie = base_es[0] + (ex & 0xFFFFu), is = base_es[1] + (ex >> 16);
	const uint32_t tot_e = base_es[0] + (tot & 0xFFFFu);
	// rank table for the run matcher: ends put on the list by the positions before g (last quarter of the slice's buffer): the
	// "last run end <= p" of a position is then one lookup and a step or two instead of a binary search of twelve dependent loads
	if ((uint32_t)tid * 8 < (uint32_t)RUNLEN_OUT && g < L) re[dfl_run_rank(a.in_stride, g)] = ie;
#pragma unroll
	for (int k = 0; k < 8; k++) {
		if ((me >> k) & 1u) re[ie++] = g + k + 3;
		if ((ms >> k) & 1u) rs[is++] = g + k;
	}
	if (tid == 0 && c0 + RUNLEN_OUT >= L) a.run_end_count[s] = tot_e;  // the slice's last chunk
}

__global__ void __launch_bounds__(256) dfl_run_info_kernel(DeflateArgs a)
{
	const int s = blockIdx.y;
	const uint8_t *in = a.in + (size_t)s * a.in_stride;
	const uint32_t *re = a.run_ends + (size_t)s * a.in_stride;
	const uint32_t *rs = dfl_run_starts(re, a.in_stride);
	uint32_t *rl = dfl_run_info(a.run_ends + (size_t)s * a.in_stride, a.in_stride);
	const uint32_t nre = a.run_end_count[s];
	for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nre; t += gridDim.x * blockDim.x) {
		const uint32_t x = re[t], len = x - rs[t];
		rl[t] = (len < 511u ? len : 511u) | ((uint32_t)in[x - 1] << 16);
	}
}

// Positions p whose string starts with three equal bytes b (r = number of b's from p, capped).
// Every candidate of that bucket that can reach length 3 is itself a position of some run of b:
//   * p-1 (when in[p-1] == b) is the chain head and yields exactly r;
//   * a position q of an EARLIER run [s_j, e_j) yields min(e_j - q, r), plus the common prefix of what
//     follows both runs when e_j - q == r; descending q inside a run, the first position reaching the run's
//     maximum is q = e_j - r (run long enough) or the lowest position still inside the chain limits.
// So the lane scans run ends backwards, one O(1) step per run.  The limits of deflate.c become position
// limits: the first K chain entries are the sorted indices i-1 .. i-K (K = max_chain, and max_chain >> 2
// for the good_match variant); distance < MAX_DIST; position 0 is NIL.
// nice_match: inside a run the candidates come as d = e_j - q = 3, 4, ...; the walk ends at the first that
// reaches nice_eff.  When nice_eff < r that is q = e_j - nice_eff with length exactly nice_eff, before the
// longer extension at q = e_j - r is seen: a run is counted down to k = min(r, nice_eff) bytes at most
// (proved against the chain walk in tools/deflate_level_model.c, run_rule).
__global__ void __launch_bounds__(256) dfl_match_run_kernel(DeflateArgs a, int n)
{
	int s; uint32_t part, nparts;
	if (!xcd_slice(n, s, part, nparts)) return;
	const uint32_t L = a.in_sizes[s];
	const uint8_t *in = a.in + (size_t)s * a.in_stride;
	const size_t base = (size_t)s * a.in_stride;
	const uint64_t *recs = a.rec_out + base;  // sorted (hash, position) records: position | hash << 32
	uint2 *mr = reinterpret_cast<uint2 *>(a.mr) + base;
	const uint32_t *deep = dfl_deep_top(a.heavy_list + base, a.in_stride);  // grows downwards from the end
	const uint32_t ndeep = a.deep_count[s];
	const uint32_t *re = a.run_ends + base;
	const uint32_t *rl = dfl_run_info(re, a.in_stride);
	const uint32_t nre = a.run_end_count[s];
	const uint32_t gen = *a.gen;
	const uint32_t quarter = a.max_chain >> 2;
	for (uint32_t e = part * blockDim.x + threadIdx.x; e < ndeep; e += nparts * blockDim.x) {
		const uint32_t i = *(deep - e);
		// the four records a position can need depend on its sorted index only: requested together (clamped, not tested)
		const uint64_t ri = recs[i];
		const uint64_t r_head = recs[i >= 1 ? i - 1 : 0], r_quarter = recs[i >= quarter ? i - quarter : 0], r_full = recs[i >= a.max_chain ? i - a.max_chain : 0];
		const uint32_t p = rec_pos(ri, a.pos_mask);
		const uint32_t h = rec_hash(ri, a.pos_mask);
		const uint32_t lookahead = L - p;
		const uint32_t max_len = lookahead < (uint32_t)MAX_MATCH ? lookahead : (uint32_t)MAX_MATCH;
		const uint32_t nice_eff = min(lookahead, a.nice);  // nice_match clamped to the lookahead (<= max_len)
		const uint8_t b = in[p], b_prev = in[p >= 1 ? p - 1 : 0];
		const uint32_t r = a.run_len[base + p] & 0x7FFFu;  // run length from p, capped at max_len
		const uint32_t k = min(r, nice_eff);               // bytes of an earlier run that can count
		const bool has_prev = p >= 2 && b_prev == b;  // position 0 is NIL
		uint32_t best4 = has_prev ? r : 0u, q4 = p - 1, best1 = best4, q1 = p - 1;
		bool scan = true;
		if (!has_prev) {  // chain head rules of deflate_slow / longest_match
			const uint64_t rh = i >= 1 ? r_head : ~0ull;
			const bool have_head = i >= 1 && rec_hash(rh, a.pos_mask) == h;
			const uint32_t hq = have_head ? rec_pos(rh, a.pos_mask) : 0u;
			if (!have_head || hq == 0 || hq == nil_candidate(p, lookahead) || p - hq > (uint32_t)MAX_DIST) scan = false;
			else if (p - hq == (uint32_t)MAX_DIST) {  // only the head itself may sit at distance MAX_DIST
				uint32_t len = 0;
				len = (uint32_t)common_prefix(in + hq, in + p, 0, (int)max_len);
				best4 = best1 = len; q4 = q1 = hq;
				scan = false;
			}
		}
		if (scan && best4 < nice_eff) {
			const bool ext_ok = r < max_len;  // bytes after the run can only matter below the cap
			const uint8_t c = ext_ok ? in[p + r] : 0;
			const uint32_t qw = p >= (uint32_t)MAX_DIST ? p - (uint32_t)MAX_DIST + 1 : 1u;  // dist < MAX_DIST, q != NIL
			uint32_t qmin4 = qw, qmin1 = qw;
			if (i >= a.max_chain && rec_hash(r_full, a.pos_mask) == h) qmin4 = max(qmin4, rec_pos(r_full, a.pos_mask));
			if (i >= quarter && rec_hash(r_quarter, a.pos_mask) == h) qmin1 = max(qmin1, rec_pos(r_quarter, a.pos_mask));
			// number of run ends <= p (none lies strictly inside p's own run): an end x comes from position x - 3, so these are the
			// entries of the positions below p - 2 -- the rank table gives those below the 8-aligned part, the rest is a step or two
			uint32_t lo = 0;
			if (p >= 3) {
				lo = re[dfl_run_rank(a.in_stride, p - 2)];
				while (lo < nre && re[lo] <= p) lo++;
			}
			// (the entry of the next step is requested before this one is evaluated: the loop is a chain of dependent lookups otherwise)
			uint32_t x_n = lo ? re[lo - 1] : 0u, lw_n = lo ? rl[lo - 1] : 0u;
			for (int64_t t = (int64_t)lo - 1; t >= 0; t--) {
				const uint32_t x = x_n;
				const uint32_t lw = lw_n;          // min(run length, 511) | run byte << 16
				{ const int64_t tn = t > 0 ? t - 1 : 0; x_n = re[tn]; lw_n = rl[tn]; }
				if (x < qmin4 + 3) break;          // even q = x-3 is outside the first max_chain entries / the window
				if ((lw >> 16) != b) continue;     // a run of another byte
				const uint32_t m = min(min(lw & 0xFFFFu, k), x - qmin4);  // run length counted down to qmin4, capped at k
				if (m >= 3) {
					uint32_t q, len;
					if (m == r) {
						q = x - r; len = r;
						if (ext_ok && in[x] == c) len = (uint32_t)common_prefix(in + q, in + p, (int)r + 1, (int)max_len);
					} else { q = x - m; len = m; }
					if (len > best4) { best4 = len; q4 = q; }
					// the same run seen through the quarter limit
					if (x >= qmin1 + 3) {
						const uint32_t m1 = min(m, x - qmin1);
						if (m1 == m) { if (len > best1) { best1 = len; q1 = q; } }
						else if (m1 >= 3 && m1 > best1) { best1 = m1; q1 = x - m1; }
					}
					if (best4 >= nice_eff) break;
				}
				if (x - m <= qmin4) break;  // the run was cut by the limit: older runs are outside
			}
		}
		mr[p] = pack_match(best4, best1, best4 ? p - q4 : 0u, best1 ? p - q1 : 0u, gen);
	}
}

// ------------------------------------------------------------------ 3a. decision records + block summaries
// rec32: bits 0..7 k (deferred literals), 8..16 match length (0 = none), 17..31 distance
// lazy = max_lazy_match, good = good_match of the level, minl = DeflateArgs::min_len (3, or 6 under Z_FILTERED)
__device__ __forceinline__ void match_of(const MatchRec &r, uint32_t p, uint32_t npos, int prev_len, int lazy, int good, int minl,
                                         int &len, int &dist)
{
	// deflate_slow: match_length after longest_match + filter / TOO_FAR rule, given prev_length (deflate.c:1863-1880); r = record
	// of p.  zlib drops a match of <= 5 bytes under Z_FILTERED: the same as requiring minl = 6 bytes here (a length longest_match
	// returns without beating prev_length is "no match" either way), and a 3-byte match never survives it for the TOO_FAR test
	len = 2; dist = 0;
	if (p >= npos || prev_len >= lazy) return;
	const int l = prev_len >= good ? r.len_quarter : r.len_full;
	const int d = prev_len >= good ? r.dist_quarter : r.dist_full;
	if (l > prev_len && l >= minl) { len = l; dist = d; }
	if (len == MIN_MATCH && dist > TOO_FAR) len = 2;
}
__device__ __forceinline__ void match_at(const MatchRec *mr, const uint16_t *rl, uint32_t gen, uint32_t p, uint32_t npos, int prev_len,
                                         int lazy, int good, int minl, int &len, int &dist)
{
	len = 2; dist = 0;
	if (p >= npos || prev_len >= lazy) return;
	match_of(checked_match(mr[p], gen, rl[p], p, npos + 2), p, npos, prev_len, lazy, good, minl, len, dist);
}

__global__ void __launch_bounds__(256) dfl_rec_kernel(DeflateArgs a)
{
	const int s = blockIdx.y;
	const uint32_t L = a.in_sizes[s];
	const size_t base = (size_t)s * a.in_stride;
	const uint32_t npos = L >= MIN_MATCH ? L - 2 : 0;
	const MatchRec *mr = reinterpret_cast<const MatchRec *>(a.mr) + base;
	const uint16_t *rl = a.run_len + base;
	const uint32_t nblk64 = (L + 63) / 64;
	const int lane = threadIdx.x & 63;
	const uint32_t gen = *a.gen;
	const int lazy = (int)a.max_lazy, good = (int)a.good, minl = (int)a.min_len;
	// the lane's own record and its right neighbour's (what the first deferral test reads) are requested together and without a
	// branch (a load inside a conditional is waited for on the spot, which made them two round trips in a row), one turn ahead
	const uint32_t lastp = npos ? npos - 1 : 0;
	const uint32_t wb_step = gridDim.x * (blockDim.x >> 6);
	struct Req { MatchRec m0, m1; uint32_t w0, w1; };
	auto request = [&](uint32_t wb) {
		const uint32_t p = wb * 64 + lane, pa = min(p, lastp), pb = min(p + 1, lastp);
		return Req{mr[pa], mr[pb], rl[pa], rl[pb]};
	};
	const uint32_t wb0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	Req nx = request(wb0);
	for (uint32_t wb = wb0; wb < nblk64; wb += wb_step) {
		const uint32_t p = wb * 64 + lane;
		const uint32_t blk_end = wb * 64 + 64;
		uint32_t rec = 0, nxt = blk_end, cnt = 0;
		const uint32_t pa = min(p, lastp), pb = min(p + 1, lastp);
		const Req cq = nx;
		nx = request(wb + wb_step);
		const MatchRec r0 = checked_match(cq.m0, gen, cq.w0, pa, L), r1 = checked_match(cq.m1, gen, cq.w1, pb, L);
		if (p < L) {
			int len, dist;
			match_of(r0, p, npos, 2, lazy, good, minl, len, dist);
			if (len < MIN_MATCH) { rec = 0; nxt = p + 1; cnt = 1; }  // literal in[p]
			else {
				uint32_t k = 0;
				for (;;) {  // lazy evaluation: defer while the next position has a longer match
					int l2, d2;
					if (k == 0) match_of(r1, p + 1, npos, len, lazy, good, minl, l2, d2);
					else match_at(mr, rl, gen, p + k + 1, npos, len, lazy, good, minl, l2, d2);
					if (l2 > len) { len = l2; dist = d2; k++; } else break;
				}
				rec = k | ((uint32_t)len << 8) | ((uint32_t)dist << 17);
				nxt = p + k + (uint32_t)len;
				cnt = k + 1;
			}
		}
		a.rec32[base + p] = rec;  // in_stride >= L rounded up to 256, so p < stride
		// entry -> exit summary of this 64-position block by pointer doubling
#pragma unroll
		for (int r = 0; r < 6; r++) {
			const bool inside = nxt < blk_end;
			const int j = inside ? (int)(nxt - wb * 64) : lane;
			const uint32_t n2 = __shfl(nxt, j), c2 = __shfl(cnt, j);
			if (inside) { nxt = n2; cnt += c2; }
		}
		a.exit_pos[base + p] = (nxt - blk_end) | (cnt << 16);  // both < 1024: one word per position (entry -> exit offset past the block, symbols)
	}
}

// ------------------------------------------------------------------ 3a'. the parse of the short passes
// deflate_rle: at position p > 0 with >= 3 bytes of lookahead and in[p-1] == in[p] == in[p+1] == in[p+2], the match (distance 1)
// runs over every byte equal to in[p-1] from p, capped at MAX_MATCH and at the end of the input; otherwise in[p] is a literal.
// The parse is greedy (no lazy step), so a position's record needs only its run-length word: the length is the word's low
// bits, and in[p-1] == in[p] is its bit 15 -- except at p = 1, where bit 15 is clear (the hash chains never match position 0,
// the run matcher's rule) but deflate_rle compares in[0] and in[1]: in[0] == in[1] is run_len[0] >= 2.  Same rec32 / exit_pos
// format as dfl_rec_kernel (k = 0 deferred literals, one symbol per decision position), so the walk and the symbols kernel
// follow it unchanged.
__global__ void __launch_bounds__(256) dfl_rle_rec_kernel(DeflateArgs a)
{
	const int s = blockIdx.y;
	const uint32_t L = a.in_sizes[s];
	const size_t base = (size_t)s * a.in_stride;
	const uint16_t *rl = a.run_len + base;
	const uint32_t nblk64 = (L + 63) / 64;
	const int lane = threadIdx.x & 63;
	const uint32_t lastp = L ? L - 1 : 0;
	const uint32_t wb_step = gridDim.x * (blockDim.x >> 6);
	const uint32_t wb0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	uint32_t nx = rl[min(wb0 * 64 + lane, lastp)];  // one turn ahead, index clamped instead of tested
	for (uint32_t wb = wb0; wb < nblk64; wb += wb_step) {
		const uint32_t p = wb * 64 + lane;
		const uint32_t blk_end = wb * 64 + 64;
		const uint32_t rw = nx;
		nx = rl[min((wb + wb_step) * 64 + lane, lastp)];
		const uint32_t rw0 = (uint32_t)__shfl((int)rw, 0);  // run_len[0] in the wave of block 0
		const bool prev_eq = p >= 2 ? (rw >> 15) != 0 : (p == 1 && (rw0 & 0x7FFFu) >= 2u);
		const uint32_t run = rw & 0x7FFFu;
		uint32_t rec = 0, nxt = blk_end, cnt = 0;
		if (p < L) {
			const bool m = prev_eq && run >= (uint32_t)MIN_MATCH;  // (run >= 3 implies the lookahead >= 3)
			rec = m ? (run << 8) | (1u << 17) : 0u;
			nxt = p + (m ? run : 1u);
			cnt = 1;
		}
		a.rec32[base + p] = rec;
#pragma unroll
		for (int r = 0; r < 6; r++) {
			const bool inside = nxt < blk_end;
			const int j = inside ? (int)(nxt - wb * 64) : lane;
			const uint32_t n2 = __shfl(nxt, j), c2 = __shfl(cnt, j);
			if (inside) { nxt = n2; cnt += c2; }
		}
		a.exit_pos[base + p] = (nxt - blk_end) | (cnt << 16);
	}
}

// deflate_huff: every byte is a literal, so symbol p is in[p] and block m ends at input position BS (m + 1) (BS = 16383 or
// 32767, memLevel 8 or 9), flushed in the loop iteration of its last literal: no parse, no walk.  Four positions per lane
// (in_stride is a multiple of 256: the dword and the four symbols stay inside the slice)
template <uint32_t BS>
__global__ void __launch_bounds__(256) dfl_huff_symbols_kernel(DeflateArgs a)
{
	const int s = blockIdx.y;
	const uint32_t L = a.in_sizes[s];
	const size_t base = (size_t)s * a.in_stride;
	const uint32_t *in4 = reinterpret_cast<const uint32_t *>(a.in + base);
	uint4 *sym4 = reinterpret_cast<uint4 *>(a.sym + base);
	uint32_t *bend = a.blk_end + (size_t)s * a.max_blocks, *btop = a.blk_top + (size_t)s * a.max_blocks;
	if (blockIdx.x == 0 && threadIdx.x == 0) a.total_syms[s] = L;
	const uint32_t nq = (L + 3) / 4;
	for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += gridDim.x * blockDim.x) {
		const uint32_t w = in4[q], p0 = 4 * q;
		uint32_t v[4];
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const uint32_t p = p0 + (uint32_t)k;
			v[k] = p < L ? (w >> (8 * k)) & 255u : 0u;
			if (p < L && p % BS == BS - 1) { bend[p / BS] = p + 1; btop[p / BS] = p; }
		}
		sym4[q] = make_uint4(v[0], v[1], v[2], v[3]);
	}
}

// ------------------------------------------------------------------ 3b. block-to-block walk (one workgroup per slice)
// The parse enters 64-position block b at exit_pos[previous entry]; that hop chain is serial (~4500 hops per
// slice), but its only state is the position, and chains that start at different positions merge as soon as
// they share one decision position.  So the slice is cut into WALK_T segments: every lane hops through its own
// segment from a speculative start (the segment boundary), then restarts from where its predecessor really
// landed until no start moves any more (lane k is final after k passes at the latest; typically 2-3 passes
// of ~18 hops).  A prefix sum over the symbol counts gives every lane its symbol base, and a last pass
// publishes entry position and symbol base of every block the parse really enters.
#ifndef CCT_WALK_T
#define CCT_WALK_T 256
#endif
constexpr int WALK_T = CCT_WALK_T;  // lanes (= segments) per slice; measured per batch: 128: 85, 256: 77, 512: 89, 1024: 163 us (more segments, more restart passes)
__global__ void __launch_bounds__(WALK_T) dfl_walk_kernel(DeflateArgs a, int n)
{
	__shared__ uint32_t s_land[WALK_T];
	__shared__ uint32_t s_wsum[WALK_T / 64];
	const int s = blockIdx.x;
	(void)n;
	const uint32_t L = a.in_sizes[s];
	const size_t base = (size_t)s * a.in_stride;
	const size_t bbase = (size_t)s * dfl_blk_words(a.in_stride);
	const uint32_t *exit_rec = a.exit_pos + base;  // (offset of the exit past the entry's block) | symbols << 16
	const int tid = threadIdx.x;
	const uint32_t seg = (((L + WALK_T - 1) / WALK_T) + 63) & ~63u;
	const uint32_t seg_end = min(L, (uint32_t)(tid + 1) * seg);
	uint32_t start = min(L, (uint32_t)tid * seg), land = start, cnt = 0;
	auto hop_through = [&]() {
		uint32_t cur = start, c = 0;
		while (cur < seg_end) { const uint32_t e = exit_rec[cur]; c += e >> 16; cur = (cur & ~63u) + 64u + (e & 0xFFFFu); }
		land = cur; cnt = c;
	};
	hop_through();
	for (;;) {
		__syncthreads();
		s_land[tid] = land;
		__syncthreads();
		const uint32_t pl = tid ? s_land[tid - 1] : 0u;
		const bool moved = tid > 0 && pl != start;
		if (!__syncthreads_or(moved)) break;
		if (moved) { start = pl; hop_through(); }
	}
	// symbols before this lane's segment
	uint32_t total;
	uint32_t syms = wg_excl_scan<WALK_T / 64>(cnt, s_wsum, total);
	if (tid == 0) a.total_syms[s] = total;
	for (uint32_t cur = start; cur < seg_end;) {
		const uint32_t b = cur >> 6;
		a.blk_entry[bbase + b] = cur;
		a.blk_symbase[bbase + b] = syms;
		const uint32_t e = exit_rec[cur];
		syms += e >> 16;
		cur = (cur & ~63u) + 64u + (e & 0xFFFFu);
	}
}

// ------------------------------------------------------------------ 3c. symbols in stream order
// sym32: bits 0..7 lc (literal or length-3), bits 16..31 distance (0 = literal); BS = symbols per block (memLevel 8 or 9).
// A block ends where its last symbol's input ends (blk_end) and is flushed in the loop iteration that tallied that symbol: its
// top is the symbol's position under deflate_rle, one more under deflate_slow, which tallies a string once it has looked at the
// next one (blk_top, dfl_tree_kernel)
template <uint32_t BS>
__global__ void __launch_bounds__(256) dfl_symbols_kernel(DeflateArgs a)
{
	const int s = blockIdx.y;
	const uint32_t L = a.in_sizes[s];
	const uint8_t *in = a.in + (size_t)s * a.in_stride;
	const size_t base = (size_t)s * a.in_stride;
	const size_t bbase = (size_t)s * dfl_blk_words(a.in_stride);
	const uint32_t nblk64 = (L + 63) / 64;
	const int lane = threadIdx.x & 63;
	uint32_t *sym = a.sym + base;
	uint32_t *bend = a.blk_end + (size_t)s * a.max_blocks, *btop = a.blk_top + (size_t)s * a.max_blocks;
	const uint32_t lazy = short_pass(a.strategy) ? 0u : 1u;
	// everything a block needs is requested without a branch (a load inside a conditional is waited for on the spot: entry,
	// record, symbol base and the literal byte used to be four round trips in a row) -- and one turn ahead
	const uint32_t wb_step = gridDim.x * (blockDim.x >> 6), wb_last = nblk64 ? nblk64 - 1 : 0;
	struct Req { uint32_t entry, symbase, rec; uint8_t lit0; };
	auto request = [&](uint32_t wb) {
		const uint32_t wbc = min(wb, wb_last), pc = min(wbc * 64 + lane, L - 1);  // L > 0 where the loop runs
		return Req{a.blk_entry[bbase + wbc], a.blk_symbase[bbase + wbc], a.rec32[base + pc], in[pc]};
	};
	const uint32_t wb0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	Req nx = nblk64 ? request(wb0) : Req{0xFFFFFFFFu, 0, 0, 0};
	for (uint32_t wb = wb0; wb < nblk64; wb += wb_step) {
		const uint32_t p = wb * 64 + lane;
		const Req cur_req = nx;
		nx = request(wb + wb_step);
		const uint32_t entry = cur_req.entry, symbase = cur_req.symbase;
		uint32_t rec = cur_req.rec;
		const uint8_t lit0 = cur_req.lit0;
		if (entry == 0xFFFFFFFFu) continue;  // block jumped over by a match
		if (p >= L) rec = 0;
		const uint32_t k = rec & 0xFFu, len = (rec >> 8) & 0x1FFu, dist = rec >> 17;
		const uint32_t nxt = len ? p + k + len : p + 1;
		const uint32_t cnt = len ? k + 1 : 1;
		// which lanes are decision positions: a literal position hands over to its neighbour, so the chain from the
		// entry covers whole stretches of lanes up to the next position that starts a match, and only the matches
		// need a hop (wave-uniform loop on the scalar unit)
		const uint64_t jump = __ballot(len != 0);
		const uint32_t nvalid = min(64u, L - wb * 64);
		uint64_t visited = 0;
		uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)(entry - wb * 64));
		while (cur < nvalid) {
			const uint64_t rest = jump >> cur;
			if (!rest) { visited |= ~0ull << cur; break; }
			const int d = __ffsll((long long)rest) - 1;  // lanes cur .. cur + d are visited, the last one jumps
			visited |= (d >= 63 ? ~0ull : ((2ull << d) - 1ull)) << cur;
			cur = (uint32_t)__builtin_amdgcn_readlane((int)nxt, (int)cur + d) - wb * 64;
		}
		if (nvalid < 64) visited &= (1ull << nvalid) - 1ull;
		const bool mine = (visited >> lane) & 1ull;
		// exclusive prefix of symbol counts over the visited lanes
		const uint32_t v = mine ? cnt : 0u;
		uint32_t off = symbase + wave_incl_scan(v) - v;
		if (mine) {
			if (p == L - 1) a.postloop_lit[s] = 1;  // the literal tallied after deflate_slow's main loop
			for (uint32_t t = 0; t < (len ? k : 1u); t++, off++) {  // literals
				sym[off] = t ? in[p + t] : lit0;
				if (off % BS == BS - 1) { bend[off / BS] = p + t + 1; btop[off / BS] = p + t + lazy; }
			}
			if (len) {
				sym[off] = (len - MIN_MATCH) | (dist << 16);
				if (off % BS == BS - 1) { bend[off / BS] = p + k + len; btop[off / BS] = p + k + lazy; }
			}
		}
	}
}

// ------------------------------------------------------------------ 4. Huffman trees per block (trees.c)
// One WAVE per (slice, block).  trees.c's heap decides ties by heap position, so the heap itself is replayed
// (with its sifts overlapped, one lane each: tree_heap); everything around it (histogram, leaf list, bit-length
// statistics, code assignment) is done by all 64 lanes, and the tables the serial parts index are staged in LDS (a __constant__ lookup with a
// per-lane index is a global load: ~10x the latency of an LDS read when nothing hides it).
// The working set decides how many blocks a CU works on at once (the serial heap replay is pure LDS latency, so
// resident waves are what hides it): just under 8 KB each, so that sixteen of them fit the 160 KB of a CU and a slice's blocks
// (13 on a bench payload) run as one workgroup on one CU, one wave for every block of a 256-slice batch in a single round
// (dfl_tree_kernel<16>; measured placement: profiles/tree_placement.log).  Hence the aliasing below: the histogram
// counters live in the heap array, the length/distance code tables of the histogram phase in dad[], codes are kept for
// leaves only, the header bits go straight to HBM and the static code lengths are a formula.
struct TreeScratch {  // one block's working set, in LDS
	uint16_t freq[HEAP_SIZE], dad[HEAP_SIZE], len[HEAP_SIZE], code[L_CODES + 2];      // literal/length tree
	uint16_t dfreq[2 * D_CODES + 1], ddad[2 * D_CODES + 1], dlen[2 * D_CODES + 1], dcode[D_CODES + 2];
	uint16_t bfreq[2 * BL_CODES + 1], bdad[2 * BL_CODES + 1], blen[2 * BL_CODES + 1], bcode[BL_CODES + 1];
	// heap entries carry their own sort key: freq << 15 | depth << 10 | node, so that trees.c's smaller(n, m)
	// is (e_n >> 10) <= (e_m >> 10) and one 64-bit LDS read fetches both children (freq <= 32768: 16 bits at memLevel 9;
	// depth <= 22 for that total weight: 5 bits; node < 573: 10 bits)
	alignas(16) uint32_t heap[HEAP_SIZE + 11];  // + a sink slot for each lane of the heap replay (tree_heap)
	uint32_t bl_count[MAX_BITS + 1];
	uint16_t next_code[MAX_BITS + 1];
	int heap_len, heap_max, max_code, overflow, lmax, dmax;
	uint32_t opt_len, static_len, dyn_body_bits;
	// dynamic-block header (14 + 3*19 + up to 316 * 14 bits), assembled by the whole wave with LDS atomics
	uint32_t hdr_bits[160];
	uint32_t hdr_nbits;
	int ntok, btype, max_blindex;
	// staged tables
	uint8_t extra_l[29], extra_d[30], extra_bl[19], bl_order[19];
	// histogram phase only (see above)
	__device__ __forceinline__ uint32_t *hist_l() { return heap; }
	__device__ __forceinline__ uint32_t *hist_d() { return heap + L_CODES + 2; }
	__device__ __forceinline__ uint8_t *length_code() { return reinterpret_cast<uint8_t *>(dad); }
	__device__ __forceinline__ uint8_t *dist_code() { return reinterpret_cast<uint8_t *>(dad) + 256; }
	// header phase: the run-length tokens of the two code-length sequences (scan_tree records them, the wave emits them);
	// dad[] of the literal/length tree is free by then.  token = symbol 0..18 | extra-bits value << 5
	__device__ __forceinline__ uint16_t *tok() { return dad; }
};
static_assert(16 * sizeof(TreeScratch) <= 160 * 1024, "a workgroup of 16 tree waves has to fit the LDS of a CU");
// A tree wave shares its TreeScratch with no other wave, so what orders its phases is wave-local: the LDS operations of one
// wave complete in program order, and the compiler is kept to that order.  (A workgroup barrier would hang: waves of one
// workgroup leave early or work on different trees.)
__device__ __forceinline__ void tree_wave_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}
static_assert(HEAP_SIZE >= L_CODES + D_CODES, "token list fits dad[]");
static_assert((HEAP_SIZE + 1) * 4 >= (L_CODES + 2 + D_CODES) * 4 && HEAP_SIZE * 2 >= 768, "aliases fit");
// tr_static_init's literal/length code lengths (trees.c:255-258)
__device__ __forceinline__ uint32_t static_llen(int n) { return n <= 143 ? 8u : n <= 255 ? 9u : n <= 279 ? 7u : 8u; }

// LDS-typed pointers: a view chosen at run time (one copy of the tree code serves all three alphabets) still
// compiles to ds_* instructions
typedef __attribute__((address_space(3))) uint16_t lds_u16;
struct TreeView { lds_u16 *freq, *dad, *len, *code; };

// trees.c pqdownheap(k) on the lane's own node: the level-parallel heapify runs one per lane (disjoint subtrees)
__device__ __forceinline__ void pqdownheap(TreeScratch &S, int k, int hl)
{
	// smaller(a, b) of trees.c is (a >> 10) <= (b >> 10) on these entries, i.e. a <= (b | 1023): one OR instead of two shifts
	const uint32_t v = S.heap[k];
	for (int j = k << 1; j <= hl; j = k << 1) {
		const uint2 pr = *reinterpret_cast<const uint2 *>(&S.heap[j]);  // j is even: children j, j+1 in one read
		const int right = (j < hl && pr.y <= (pr.x | 1023u)) ? 1 : 0;
		const uint32_t e = right ? pr.y : pr.x;
		if (v <= (e | 1023u)) break;
		S.heap[k] = e;
		k = j + right;
	}
	S.heap[k] = v;
}

// build_tree + gen_bitlen + gen_codes (trees.c:486-700) in five phases.  The overflow repair is serial (one lane per
// block); the heap replay runs a few sifts side by side, and the phases around them use all 64 lanes on one block at a time.
// kind: 0 literal/length, 1 distance, 2 bit-length
__device__ __forceinline__ TreeView view_of(TreeScratch &S, int kind)
{
	if (kind == 0) return TreeView{(lds_u16 *)S.freq, (lds_u16 *)S.dad, (lds_u16 *)S.len, (lds_u16 *)S.code};
	if (kind == 1) return TreeView{(lds_u16 *)S.dfreq, (lds_u16 *)S.ddad, (lds_u16 *)S.dlen, (lds_u16 *)S.dcode};
	return TreeView{(lds_u16 *)S.bfreq, (lds_u16 *)S.bdad, (lds_u16 *)S.blen, (lds_u16 *)S.bcode};
}
__device__ __forceinline__ int elems_of(int kind) { return kind == 0 ? L_CODES : kind == 1 ? D_CODES : BL_CODES; }

// (whole wave) leaves with a non-zero frequency, in symbol order: the initial heap array
__device__ void tree_leaves(TreeScratch &S, int kind)
{
	const TreeView t = view_of(S, kind);
	const int lane = threadIdx.x & 63, elems = elems_of(kind);
	const uint64_t lt_mask = (1ull << lane) - 1ull;
	int max_code = -1;
	uint32_t nleaf = 0;
	for (int n0 = 0; n0 < elems; n0 += 64) {
		const int n = n0 + lane;
		const uint32_t f = n < elems ? t.freq[n] : 0u;
		const uint64_t bal = __ballot(f != 0);
		if (f != 0) S.heap[1 + nleaf + (uint32_t)__popcll(bal & lt_mask)] = (f << 15) | (uint32_t)n;  // depth 0
		else if (n < elems) t.len[n] = 0;
		if (bal) max_code = n0 + 63 - __clzll((long long)bal);
		nleaf += (uint32_t)__popcll(bal);
	}
	if (lane == 0) { S.heap_len = (int)nleaf; S.max_code = max_code; }
}

// (whole wave) the heap replay proper (trees.c:625-668), exact to the heap position, so that ties are decided as zlib does.
// A sift is a chain of dependent LDS round trips, one per heap level; the replay overlaps them instead of running them in
// a row (tools/tree_schedule_model.cpp models this schedule and checks it against trees.c):
//  - heapify: trees.c sifts every node of a depth before any node above it, and the nodes of one depth have disjoint
//    subtrees, so one round per depth sifts all of them at once, one lane each;
//  - main loop: the sifts A (pqremove: heap[h] sinks from the root) and B (the new node sinks from the root) depend on each
//    other only at the root.  So they run one lane each, TREE_SIFTS lanes round robin, every sift one level per tick, and a
//    new one starts every other tick at the earliest (a tick reads the child pairs, then writes the holes: a sift two
//    levels behind the one ahead reads only what that one has written).  B needs the root left by A's first level, the next
//    A the root left by B's first level.  A also takes the last slot h: it waits while h lies in the subtree of a moving
//    sift's hole.  Then no sift in flight ever touches h again, and its bound check agrees with the sequential one.
constexpr int TREE_SIFTS = 8;  // at most 5 in flight: one starts every other tick, none lasts more than 9 ticks
__device__ void tree_heap(TreeScratch &S, int kind)
{
	const TreeView t = view_of(S, kind);
	const int lane = threadIdx.x & 63;
	int max_code = S.max_code, h = S.heap_len;
	while (h < 2) {  // (uniform) at least two codes, trees.c:612-621
		const int node = max_code < 2 ? ++max_code : 0;
		h++;
		if (lane == 0) {
			t.freq[node] = 1; S.opt_len--;
			S.heap[h] = (1u << 15) | (uint32_t)node;
			if (kind == 0) S.static_len -= static_llen(node);
			else if (kind == 1) S.static_len -= 5;
		}
	}
	tree_wave_sync();
	for (int d = 31 - __clz(h >> 1); d >= 0; d--) {  // heapify, deepest inner level first
		const int lo = 1 << d, hi = min((2 << d) - 1, h >> 1);
		for (int n0 = lo; n0 <= hi; n0 += 64) {
			if (n0 + lane <= hi) pqdownheap(S, n0 + lane, h);
			__builtin_amdgcn_wave_barrier();  // one wave: LDS order is program order; keep the compiler to it as well
		}
	}
	if (lane < TREE_SIFTS) {
		// the lane's sift: value v, hole k, heap length hl.  A lane whose sift is over keeps reading below its last hole
		// (harmless) and writes to a slot of its own past the heap: the step has no branch
		uint32_t v = 0, k = 1, hl = 0, w = 0;
		bool moving = false;
		const uint32_t sink = HEAP_SIZE + 3 + lane;
		auto tick = [&]() {  // one level of every sift in flight: read the child pair, then write the hole
			const uint32_t j = k << 1;  // <= 2 * 286: the pair lies inside heap[]
			const uint2 pr = *reinterpret_cast<const uint2 *>(&S.heap[j]);
			const uint32_t right = (j < hl && pr.y <= (pr.x | 1023u)) ? 1u : 0u;
			const uint32_t e = right ? pr.y : pr.x;
			const bool go = moving && j <= hl && v > (e | 1023u);
			w = go ? e : v;  // the hole at k receives the smaller child, or v (which then stays there)
			uint32_t at = moving ? k : sink;
			asm volatile("" : "+v"(at), "+v"(w));  // both as selects: left alone, the compiler splits the store into two branches
			S.heap[at] = w;
			k = go ? j + right : k;
			moving = go;
			__builtin_amdgcn_wave_barrier();  // one wave: LDS order is program order; keep the compiler to it as well
		};
		auto start = [&](int slot, uint32_t x) {
			const bool me = lane == slot;
			v = me ? x : v; k = me ? 1u : k; hl = me ? (uint32_t)h : hl; moving = moving || me;
		};
		int node = elems_of(kind), hm = HEAP_SIZE, slot = 0;
		uint32_t en = S.heap[1];  // the root the next A removes
		for (;;) {  // one iteration of trees.c's loop: A, an idle tick, B, an idle tick
			// A takes the last slot h: not while h lies in the subtree of a moving sift's hole
			while (__ballot(moving && ((uint32_t)h >> (__clz(k | 1u) - __clz(h))) == k)) tick();
			h--;
			start(slot, S.heap[h + 1]);
			tick();
			const uint32_t em = (uint32_t)__builtin_amdgcn_readlane((int)w, slot);  // A has left em at the root
			const uint32_t f = (en >> 15) + (em >> 15);
			const uint32_t dn = (en >> 10) & 31u, dm = (em >> 10) & 31u;
			const uint32_t d = (dn >= dm ? dn : dm) + 1;
			if (lane == 0) {
				S.heap[hm - 1] = en; S.heap[hm - 2] = em;
				t.freq[node] = (uint16_t)f;
				t.dad[en & 1023u] = t.dad[em & 1023u] = (uint16_t)node;
			}
			hm -= 2;
			slot = (slot + 1) & (TREE_SIFTS - 1);
			tick();
			start(slot, (f << 15) | (d << 10) | (uint32_t)node);  // B: the new node
			tick();
			en = (uint32_t)__builtin_amdgcn_readlane((int)w, slot);
			slot = (slot + 1) & (TREE_SIFTS - 1);
			node++;
			if (h < 2) break;
			tick();
		}
		while (__ballot(moving)) tick();
		if (lane == 0) {
			S.heap[--hm] = en;
			S.heap_len = h; S.heap_max = hm;
			S.max_code = max_code;
		}
	}
}

// (whole wave) gen_bitlen's first loop and its statistics
__device__ void tree_depths(TreeScratch &S, int kind)
{
	const TreeView t = view_of(S, kind);
	const int lane = threadIdx.x & 63;
	const int max_length = kind == 2 ? MAX_BL_BITS : MAX_BITS;
	const int base = kind == 0 ? 257 : 0;
	const int max_code = S.max_code, heap_max = S.heap_max;
	const uint32_t root = S.heap[heap_max];
	// trees.c:506-520: depth of every node = depth of its parent + 1, clamped to max_length; `overflow` counts the nodes
	// that had to be clamped.  Parents precede children in the sorted tail, so trees.c does it in one serial pass; here
	// all nodes of a level are done at once, level after level.
	constexpr uint16_t UNKNOWN = 0xFFFF;
	for (int h = heap_max + 1 + lane; h < HEAP_SIZE; h += 64) t.len[S.heap[h] & 1023u] = UNKNOWN;
	if (lane == 0) t.len[root & 1023u] = 0;
	if (lane <= MAX_BITS) S.bl_count[lane] = 0;
	tree_wave_sync();
	for (bool again = true; again;) {
		again = false;
		for (int h0 = heap_max + 1; h0 < HEAP_SIZE; h0 += 64) {
			const int h = h0 + lane;
			bool unknown = false;
			if (h < HEAP_SIZE) {
				const int n = (int)(S.heap[h] & 1023u);
				if (t.len[n] == UNKNOWN) {
					const uint32_t ld = t.len[t.dad[n]];
					if (ld == UNKNOWN) unknown = true;
					else t.len[n] = (uint16_t)min(ld + 1u, (uint32_t)max_length);
				}
			}
			if (__ballot(unknown)) again = true;
		}
		tree_wave_sync();
	}
	int overflow = 0;
	for (int h0 = heap_max + 1; h0 < HEAP_SIZE; h0 += 64) {
		const int h = h0 + lane;
		const bool clamped = h < HEAP_SIZE && t.len[t.dad[S.heap[h] & 1023u]] == (uint32_t)max_length;
		overflow += (int)__popcll(__ballot(clamped));
	}
	// bl_count / opt_len / static_len over the leaves (every leaf of the tree has freq != 0)
	uint32_t o = 0, st = 0;
	for (int n = lane; n <= max_code; n += 64) {
		const uint32_t f = t.freq[n];
		if (f == 0) continue;
		const uint32_t bits = t.len[n];
		atomicAdd(&S.bl_count[bits], 1u);
		uint32_t xbits = 0;
		if (n >= base) xbits = kind == 0 ? S.extra_l[n - base] : kind == 1 ? S.extra_d[n] : S.extra_bl[n];
		o += f * (bits + xbits);
		if (kind == 0) st += f * (static_llen(n) + xbits);
		else if (kind == 1) st += f * (5u + xbits);
	}
	o = wave_sum(o); st = wave_sum(st);
	if (lane == 0) { S.overflow = overflow; S.opt_len += o; S.static_len += st; }
}

// (one lane) gen_bitlen's overflow repair (rare) and the first code of every length
__device__ void tree_fix(TreeScratch &S, int kind)
{
	const TreeView t = view_of(S, kind);
	const int max_length = kind == 2 ? MAX_BL_BITS : MAX_BITS;
	const int max_code = S.max_code;
	int overflow = S.overflow;
	if (overflow > 0) {  // move leaves down until the Kraft sum fits (trees.c:540-571)
		int bits, n, m, h = HEAP_SIZE;
		do {
			bits = max_length - 1;
			while (S.bl_count[bits] == 0) bits--;
			S.bl_count[bits]--; S.bl_count[bits + 1] += 2; S.bl_count[max_length]--;
			overflow -= 2;
		} while (overflow > 0);
		for (bits = max_length; bits != 0; bits--) {
			n = (int)S.bl_count[bits];
			while (n != 0) {
				m = (int)(S.heap[--h] & 1023u);
				if (m > max_code) continue;
				if ((uint32_t)t.len[m] != (uint32_t)bits) {
					S.opt_len += ((uint32_t)bits - t.len[m]) * t.freq[m];
					t.len[m] = (uint16_t)bits;
				}
				n--;
			}
		}
	}
	uint32_t code = 0;
	for (int bits = 1; bits <= MAX_BITS; bits++) { code = (code + S.bl_count[bits - 1]) << 1; S.next_code[bits] = (uint16_t)code; }
}

// (whole wave) gen_codes: symbol n gets next_code[len] + (number of lower symbols with the same length), bit-reversed
__device__ void tree_codes(TreeScratch &S, int kind)
{
	const TreeView t = view_of(S, kind);
	const int lane = threadIdx.x & 63, max_code = S.max_code;
	const uint64_t lt_mask = (1ull << lane) - 1ull;
	uint32_t seen[MAX_BITS + 1];
#pragma unroll
	for (int b = 1; b <= MAX_BITS; b++) seen[b] = S.next_code[b];
	for (int n0 = 0; n0 <= max_code; n0 += 64) {
		const int n = n0 + lane;
		const int len = n <= max_code ? (int)t.len[n] : 0;
		uint32_t mine = 0;
#pragma unroll
		for (int b = 1; b <= MAX_BITS; b++) {
			const uint64_t bal = __ballot(len == b);
			if (len == b) mine = seen[b] + (uint32_t)__popcll(bal & lt_mask);
			seen[b] += (uint32_t)__popcll(bal);
		}
		if (len != 0) t.code[n] = (uint16_t)(__brev(mine) >> (32 - len));
	}
}

// scan_tree + the token side of send_tree (trees.c:703-800), by the whole wave.  trees.c walks the code lengths with a
// small state machine (count, max_count, min_count, prevlen); its state is reset at every change of value, so what it emits
// for a maximal run of R equal lengths v depends on (v, R) only:
//   v != 0:  R < 4: v, R times.   4 <= R <= 6: v, then REP_3_6(R - 1).   R >= 7: v, REP_3_6(6), then REP_3_6(6) for every
//            further six, and for the r = (R - 7) % 6 left over r times v (r < 3) or REP_3_6(r)
//   v == 0:  REPZ_11_138(138) for every 138, and for the r = R % 138 left over r times 0 (r < 3), REPZ_3_10(r) (r <= 10) or
//            REPZ_11_138(r)
// (the first chunk of a non-zero run is cut at 7 = literal + repeat of 6, later ones at 6; zero runs at 138).  So every run
// start computes its tokens on its own; a prefix sum over the runs gives the place in the token list.
// token = symbol 0..18 | extra-bits value << 5; bit-length frequencies are counted in S.hdr_bits[0..18] (free until the
// header is written) and moved to bfreq by the caller.
__device__ void scan_tree_wave(TreeScratch &S, const TreeView &t, int max_code)
{
	const int lane = threadIdx.x & 63;
	constexpr int NCH = (L_CODES + 63) / 64;  // 5 chunks of 64 positions
	const int n_el = max_code + 1;
	uint32_t v[NCH];
	uint64_t startmask[NCH];
#pragma unroll
	for (int c = 0; c < NCH; c++) {
		const int n = c * 64 + lane;
		v[c] = n < n_el ? (uint32_t)t.len[n] : 0xFFFFu;
		const uint32_t before = n == 0 ? 0xFFFFFFFFu : (uint32_t)t.len[max(n - 1, 0)];
		startmask[c] = __ballot(n < n_el && v[c] != before);
	}
	uint16_t *tk = S.tok();
	uint32_t base = (uint32_t)S.ntok;
#pragma unroll
	for (int c = 0; c < NCH; c++) {
		if (c * 64 >= n_el) break;  // (uniform)
		const int n = c * 64 + lane;
		const bool start = (startmask[c] >> lane) & 1ull;
		// run length: distance to the next run start (or to the end of the sequence)
		uint32_t R = 0;
		if (start) {
			int nxt = n_el;
			const uint64_t rest = lane < 63 ? startmask[c] >> (lane + 1) : 0ull;
			if (rest) nxt = n + (int)__ffsll((long long)rest);
			else {
#pragma unroll
				for (int c2 = NCH - 1; c2 > c; c2--) if (startmask[c2]) nxt = min(nxt, c2 * 64 + (int)__ffsll((long long)startmask[c2]) - 1);
				// (descending loop with min: the nearest following chunk that has a start wins)
			}
			R = (uint32_t)(nxt - n);
		}
		const uint32_t val = v[c];
		// tokens of the run
		uint32_t nlit_head = 0, nrep6 = 0, tail_lit = 0, tail_sym = 0xFFFFFFFFu, nbig = 0;
		if (start) {
			if (val != 0) {
				if (R < 4) nlit_head = R;
				else if (R <= 6) { nlit_head = 1; tail_sym = 16u | ((R - 4u) << 5); }
				else {
					nlit_head = 1; nrep6 = 1 + (R - 7u) / 6u;
					const uint32_t r = (R - 7u) % 6u;
					if (r < 3) tail_lit = r; else tail_sym = 16u | ((r - 3u) << 5);
				}
			} else {
				nbig = R / 138u;
				const uint32_t r = R % 138u;
				if (r < 3) tail_lit = r;
				else if (r <= 10) tail_sym = 17u | ((r - 3u) << 5);
				else tail_sym = 18u | ((r - 11u) << 5);
			}
		}
		const uint32_t ntok = nlit_head + nrep6 + nbig + tail_lit + (tail_sym != 0xFFFFFFFFu ? 1u : 0u);
		uint32_t chunk_tok;
		const uint32_t ex = wave_excl_scan(ntok, chunk_tok);
		if (start) {
			uint32_t w = base + ex;
			for (uint32_t i = 0; i < nlit_head; i++) tk[w++] = (uint16_t)val;
			for (uint32_t i = 0; i < nrep6; i++) tk[w++] = (uint16_t)(16u | (3u << 5));
			for (uint32_t i = 0; i < nbig; i++) tk[w++] = (uint16_t)(18u | (127u << 5));
			for (uint32_t i = 0; i < tail_lit; i++) tk[w++] = (uint16_t)val;
			if (tail_sym != 0xFFFFFFFFu) tk[w++] = (uint16_t)tail_sym;
			if (nlit_head + tail_lit) atomicAdd(&S.hdr_bits[val], nlit_head + tail_lit);
			if (nrep6) atomicAdd(&S.hdr_bits[16], nrep6);
			if (nbig) atomicAdd(&S.hdr_bits[18], nbig);
			if (tail_sym != 0xFFFFFFFFu) atomicAdd(&S.hdr_bits[tail_sym & 31u], 1u);
		}
		base += chunk_tok;
	}
	if (lane == 0) S.ntok = (int)base;
}

// `n` bits of `value` at bit position `pos` of the (zeroed) header image
__device__ __forceinline__ void hdr_or(TreeScratch &S, uint32_t pos, uint32_t value, uint32_t n)
{
	const uint32_t w = pos >> 5, sh = pos & 31u;
	atomicOr(&S.hdr_bits[w], value << sh);
	if (sh + n > 32u) atomicOr(&S.hdr_bits[w + 1], value >> (32u - sh));
}

// (whole wave) the header of a dynamic block (trees.c send_all_trees): HLIT, HDIST, HCLEN, the code lengths of the
// bit-length alphabet in bl_order, then the tokens scan_tree recorded, each at its prefix-summed bit offset
__device__ void send_header(TreeScratch &S)
{
	const int lane = threadIdx.x & 63;
	const int nbl = S.max_blindex + 1;
	if (lane == 0) hdr_or(S, 0, (uint32_t)(S.lmax + 1 - 257) | ((uint32_t)(S.dmax + 1 - 1) << 5) | ((uint32_t)(nbl - 4) << 10), 14);
	if (lane < nbl) hdr_or(S, 14u + 3u * (uint32_t)lane, S.blen[S.bl_order[lane]], 3);
	uint32_t base = 14u + 3u * (uint32_t)nbl;
	const uint16_t *tk = S.tok();
	const int nt = S.ntok;
	for (int c0 = 0; c0 < nt; c0 += 64) {
		const int i = c0 + lane;
		uint32_t nbits = 0, val = 0;
		if (i < nt) {
			const uint32_t sym = tk[i] & 31u, ex = tk[i] >> 5;
			const uint32_t cl = S.blen[sym];
			nbits = cl + S.extra_bl[sym];
			val = (uint32_t)S.bcode[sym] | (ex << cl);
		}
		uint32_t chunk_bits;
		const uint32_t ex = wave_excl_scan(nbits, chunk_bits);
		if (nbits) hdr_or(S, base + ex, val, nbits);
		base += chunk_bits;
	}
	if (lane == 0) S.hdr_nbits = base;
}

// Absolute position of window[0] at the top of the loop iteration at position `top` (deflate.c fill_window).  The window
// holds 64 KiB; fill_window runs once the lookahead is <= lam (deflate_slow: < MIN_LOOKAHEAD, deflate_rle: <= MAX_MATCH,
// deflate_huff: 0) and slides it by 32 KiB when strstart >= 32768 + MAX_DIST.  While input is left the window is full after
// every fill, so slide k happens at top 32768 (k - 1) + 65536 - lam; once the input is all in, at most one more follows, at
// the first top >= max(base + 65274, L - lam).
__device__ __forceinline__ uint32_t window_base(uint32_t top, uint32_t L, uint32_t strategy)
{
	const uint32_t lam = strategy == Z_HUFFMAN_ONLY ? 0u : strategy == Z_RLE ? (uint32_t)MAX_MATCH : (uint32_t)MIN_LOOKAHEAD - 1u;
	const uint32_t kf = L >= 65536u ? (L - 65536u) / 32768u + 1u : 0u;  // slides with a full window
	uint32_t k = 0;
	if (top >= 65536u - lam) k = min((top - (65536u - lam)) / 32768u + 1u, kf);
	if (k == kf && 32768u * k + (uint32_t)(WSIZE + MAX_DIST) <= top && L <= top + lam) k++;
	return 32768u * k;
}
#ifdef CCT_TREE_PROF
// tuning builds only (tools/debug/tree_prof.sh): where and when every tree wave that has a block ran.  One record per
// (slice, block), written by lane 0 at the wave's exit; the buffer belongs to the library (a capture allocates nothing), the
// tool clears it before the call it looks at and reads it afterwards.  No other code reads it.
struct TreeProbe { uint32_t hw_id, xcc_id, slice, block; uint64_t rt0, rt1, cycles; };  // rt*: s_memrealtime (100 MHz), cycles: s_memtime delta
constexpr int TREE_PROBE_CAP = 16384;
__device__ TreeProbe g_tree_probe[TREE_PROBE_CAP];
extern "C" int cct_tree_prof_reset()
{
	void *p;
	if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_tree_probe)) != hipSuccess) return -1;
	return hipMemset(p, 0, sizeof(TreeProbe) * TREE_PROBE_CAP) == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}
extern "C" int cct_tree_prof_read(void *out, int cap)  // -> records copied (32 bytes each; rt1 == 0: no wave wrote it)
{
	const int n = cap < TREE_PROBE_CAP ? cap : TREE_PROBE_CAP;
	if (hipDeviceSynchronize() != hipSuccess) return -1;
	return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tree_probe), sizeof(TreeProbe) * (size_t)n) == hipSuccess ? n : -1;
}
#define TREE_PROBE_ENTER() const uint64_t prt0 = __builtin_amdgcn_s_memrealtime(), pmt0 = __builtin_amdgcn_s_memtime()
#define TREE_PROBE_EXIT(s_, m_, max_blocks_) do { \
		const uint64_t pmt1 = __builtin_amdgcn_s_memtime(), prt1 = __builtin_amdgcn_s_memrealtime(); \
		const uint32_t pidx = (uint32_t)(s_) * (uint32_t)(max_blocks_) + (uint32_t)(m_); \
		if (lane == 0 && pidx < (uint32_t)TREE_PROBE_CAP) \
			g_tree_probe[pidx] = TreeProbe{(uint32_t)__builtin_amdgcn_s_getreg(4 | (31 << 11)) /* HW_ID */, \
			                               (uint32_t)__builtin_amdgcn_s_getreg(20 | (31 << 11)) /* XCC_ID */, \
			                               (uint32_t)(s_), (uint32_t)(m_), prt0, prt1, pmt1 - pmt0}; \
	} while (0)
#else
#define TREE_PROBE_ENTER() do {} while (0)
#define TREE_PROBE_EXIT(s_, m_, max_blocks_) do {} while (0)
#endif
// DEFLATE blocks of slice s: one flush per 16383 (32767) tallied symbols inside the loop, plus the final flush
__device__ __forceinline__ uint32_t tree_nblocks(const DeflateArgs &a, int s)
{
	const uint32_t T = a.total_syms[s], BS = a.block_syms;
	uint32_t nfull = T / BS;
	// the post-loop literal never flushes (deflate_slow only: deflate_huff and deflate_rle have none, and there a symbol count that
	// is a multiple of the block size ends the stream with an empty final block)
	if (T % BS == 0 && nfull > 0 && !short_pass(a.strategy) && a.postloop_lit[s]) nfull--;
	return nfull + 1;
}
// One wave per block: histograms + trees (trees.c _tr_flush_block); lane 0 runs the serial parts (overflow repair, block type).
// A workgroup is WAVES waves of one slice, each with a TreeScratch of its own: wave w of workgroup (s, c) takes block
// c * WAVES + w of slice s, and a wave whose block does not exist leaves at once.  The waves share nothing, so nothing in
// here or below may be a workgroup barrier (tree_wave_sync).  WAVES = 16 claims the LDS of a whole CU for the slice; slices
// are the fast grid index (launch_tree).
// a.tree_waves == 0: both instantiations are launched and the waves that have a block choose, all alike, from what only the
// device knows, the blocks of every slice: sixteen waves per workgroup where the workgroups that have a block then fit the
// CUs in one round (a 16-wave workgroup has a CU to itself, whatever its slice holds: launch_tree), one wave otherwise
template <int WAVES>
__global__ void __launch_bounds__(64 * WAVES) dfl_tree_kernel(DeflateArgs a, uint32_t cus)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t tree_lds[];  // WAVES * sizeof(TreeScratch)
	const int wave = WAVES == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (uniform, and known to be)
	const int s = blockIdx.x, n = gridDim.x, m = blockIdx.y * WAVES + wave, lane = threadIdx.x & 63;
	TreeScratch &S = reinterpret_cast<TreeScratch *>(tree_lds)[wave];
	const uint32_t T = a.total_syms[s];
	const uint32_t L = a.in_sizes[s];
	const uint32_t BS = a.block_syms;
	const uint32_t nblocks = tree_nblocks(a, s);
	BlockMeta *meta = a.block_meta + (size_t)s * a.max_blocks;
	if ((uint32_t)m >= nblocks) return;  // (wave-uniform)
	if (a.tree_waves == 0) {
		uint32_t wgs = 0;  // workgroups of sixteen waves that have a block
		for (int i = lane; i < n; i += 64) wgs += (tree_nblocks(a, i) + 15u) / 16u;
		wgs = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum(wgs));
		if ((wgs <= cus ? 16 : 1) != WAVES) return;
	}
	const uint32_t *bend = a.blk_end + (size_t)s * a.max_blocks;
	TREE_PROBE_ENTER();
#ifdef CCT_TREE_PROF  // tuning builds only: phase times of one wave
	long long tp[16]; int tpi = 0;
#define TREE_STAMP() do { if (tpi < 16) tp[tpi++] = clock64(); } while (0)
#else
#define TREE_STAMP() do {} while (0)
#endif
	TREE_STAMP();

	const bool last = (uint32_t)m == nblocks - 1;
	const uint32_t first = (uint32_t)m * BS;
	const uint32_t nsym = last ? T - first : BS;
	{
		const uint32_t *sym = a.sym + (size_t)s * a.in_stride + first;
		for (int i = lane; i < HEAP_SIZE; i += 64) { S.freq[i] = 0; S.len[i] = 0; }
		for (int i = lane; i < L_CODES + 2; i += 64) S.code[i] = 0;
		for (int i = lane; i < 2 * D_CODES + 1; i += 64) { S.dfreq[i] = 0; S.dlen[i] = 0; S.ddad[i] = 0; }
		for (int i = lane; i < D_CODES + 2; i += 64) S.dcode[i] = 0;
		for (int i = lane; i < 2 * BL_CODES + 1; i += 64) { S.bfreq[i] = 0; S.blen[i] = 0; S.bdad[i] = 0; }
		for (int i = lane; i < BL_CODES + 1; i += 64) S.bcode[i] = 0;
		uint8_t *length_code = S.length_code(), *dist_code = S.dist_code();
		{  // the constant tables, all loads first: one round trip instead of sixteen in a row (a per-lane index into
			// __constant__ memory is a global load, and a load feeding an LDS store in a rolled loop is waited for at once)
			uint8_t dc[8], lc4[4];
#pragma unroll
			for (int k = 0; k < 8; k++) dc[k] = c_dist_code[lane + 64 * k];
#pragma unroll
			for (int k = 0; k < 4; k++) lc4[k] = c_length_code[lane + 64 * k];
			const int l29 = min(lane, 28), l30 = min(lane, 29), l19 = min(lane, 18);
			const uint8_t xl = c_extra_lbits[l29], xd = c_extra_dbits[l30], xb = c_extra_blbits[l19], bo = c_bl_order[l19];
#pragma unroll
			for (int k = 0; k < 8; k++) dist_code[lane + 64 * k] = dc[k];
#pragma unroll
			for (int k = 0; k < 4; k++) length_code[lane + 64 * k] = lc4[k];
			if (lane < 29) S.extra_l[lane] = xl;
			if (lane < 30) S.extra_d[lane] = xd;
			if (lane < 19) { S.extra_bl[lane] = xb; S.bl_order[lane] = bo; }
		}
		uint32_t *hl = S.hist_l(), *hd = S.hist_d();
		for (int i = lane; i < L_CODES; i += 64) hl[i] = 0;
		if (lane < D_CODES) hd[lane] = 0;
		tree_wave_sync();
		// sixteen loads in flight (one wave per block, nothing else hides HBM latency), and the next sixteen requested before
		// these are counted: the index is clamped instead of tested so that the loads carry no branch
		{
			const uint32_t lasts = nsym ? nsym - 1 : 0;
			uint32_t nv[16];
#pragma unroll
			for (int k = 0; k < 16; k++) nv[k] = sym[min((uint32_t)(k * 64 + lane), lasts)];
			for (uint32_t i0 = 0; i0 < nsym; i0 += 64 * 16) {
				uint32_t v[16];
#pragma unroll
				for (int k = 0; k < 16; k++) v[k] = nv[k];
#pragma unroll
				for (int k = 0; k < 16; k++) nv[k] = sym[min(i0 + 1024u + (uint32_t)(k * 64 + lane), lasts)];
#pragma unroll
				for (int k = 0; k < 16; k++) {
					if (i0 + (uint32_t)(k * 64 + lane) >= nsym) continue;
					const uint32_t dist = v[k] >> 16, lc = v[k] & 0xFFu;
					if (dist == 0) atomicAdd(&hl[lc], 1u);
					else {
						const uint32_t d1 = dist - 1;
						atomicAdd(&hl[length_code[lc] + 256 + 1], 1u);
						atomicAdd(&hd[d1 < 256 ? dist_code[d1] : dist_code[256 + (d1 >> 7)]], 1u);
					}
				}
			}
		}
		tree_wave_sync();
		for (int i = lane; i < L_CODES; i += 64) S.freq[i] = (uint16_t)hl[i];
		if (lane < D_CODES) S.dfreq[lane] = (uint16_t)hd[lane];
		for (int i = lane; i < 160; i += 64) S.hdr_bits[i] = 0;
		if (lane == 0) { S.opt_len = 0; S.static_len = 0; S.hdr_nbits = 0; S.ntok = 0; S.btype = 0; S.max_blindex = 0; }
		tree_wave_sync();
		if (lane == 0) S.freq[END_BLOCK] = 1;
		for (int i = lane; i < HEAP_SIZE; i += 64) S.dad[i] = 0;  // held the code tables of the histogram
	}
	tree_wave_sync();
	TREE_STAMP();
#pragma unroll 1
	for (int kind = 0; kind < 3; kind++) {  // literal/length, distance, then the bit-length tree over both
		if (kind == 2) {
			if (lane == 0) S.dyn_body_bits = S.opt_len;  // code + extra bits of all symbols and END_BLOCK
			tree_wave_sync();
			scan_tree_wave(S, view_of(S, 0), S.lmax);
			tree_wave_sync();  // (the token count of the first sequence is the base of the second)
			scan_tree_wave(S, view_of(S, 1), S.dmax);
			tree_wave_sync();
			if (lane < BL_CODES) { S.bfreq[lane] = (uint16_t)S.hdr_bits[lane]; S.hdr_bits[lane] = 0; }
			tree_wave_sync();
		}
		tree_leaves(S, kind);
		tree_wave_sync();
		TREE_STAMP();
		tree_heap(S, kind);
		tree_wave_sync();
		TREE_STAMP();
		tree_depths(S, kind);
		tree_wave_sync();
		if (lane == 0) {
			tree_fix(S, kind);
			if (kind == 0) S.lmax = S.max_code; else if (kind == 1) S.dmax = S.max_code;
		}
		tree_wave_sync();
		tree_codes(S, kind);
		tree_wave_sync();
		TREE_STAMP();
	}
	if (lane == 0) {
		const uint32_t in_begin = m == 0 ? 0u : bend[m - 1];
		const uint32_t in_end = last ? L : bend[m];
		int max_blindex;
		for (max_blindex = BL_CODES - 1; max_blindex >= 3; max_blindex--)
			if (S.blen[S.bl_order[max_blindex]] != 0) break;
		S.opt_len += 3 * ((uint32_t)max_blindex + 1) + 5 + 5 + 4;
		uint32_t opt_lenb = (S.opt_len + 3 + 7) >> 3;
		const uint32_t static_lenb = (S.static_len + 3 + 7) >> 3;
		if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
		const uint32_t stored_len = in_end - in_begin;
		// stored blocks need block_start >= 0 in window coordinates (trees.c: buf != NULL).  At memLevel 8 a block that an
		// incompressible verdict could apply to spans < 32 KiB of input, so its start is always inside the window; 32767
		// literals can span a slide of the window
		const bool in_window = in_begin >= window_base(last ? L : a.blk_top[(size_t)s * a.max_blocks + m], L, a.strategy);
		BlockMeta bm;
		bm.in_begin = in_begin; bm.stored_len = stored_len; bm.first_sym = first; bm.nsym = nsym; bm.last = last ? 1u : 0u;
		if (in_window && stored_len + 4 <= opt_lenb) {
			bm.type = 0; bm.hdr_nbits = 0; bm.body_bits = 0;
		} else if (a.strategy == Z_FIXED || static_lenb == opt_lenb) {  // trees.c _tr_flush_block
			bm.type = 1; bm.hdr_nbits = 0; bm.body_bits = S.static_len;
		} else {
			bm.type = 2; bm.hdr_nbits = 0;  // hdr_nbits follows below, once the wave has written the header
			bm.body_bits = S.dyn_body_bits;
		}
		S.btype = (int)bm.type; S.max_blindex = max_blindex;
		meta[m] = bm;
		if (m == 0) a.n_blocks[s] = nblocks;
	}
	tree_wave_sync();
	BlockTables *bt = a.block_tables + ((size_t)s * a.max_blocks + m);
	if (S.btype == 2) {  // (uniform)
		send_header(S);
		tree_wave_sync();
		for (int i = lane; i * 32 < (int)S.hdr_nbits; i += 64) bt->hdr_bits[i] = S.hdr_bits[i];
		if (lane == 0) meta[m].hdr_nbits = S.hdr_nbits;
	}
	tree_wave_sync();
	TREE_STAMP();
#ifdef CCT_TREE_PROF
	if (s == 0 && m == 0 && lane == 0) {
		printf("[tree prof] waves=%d:", WAVES);
		for (int i = 1; i < tpi; i++) printf(" %lld", tp[i] - tp[i - 1]);
		printf("  (hist | leaves0 heap0 rest0 | scan+leaves1 heap1 rest1 | scan_tree+leaves2 heap2 rest2 | final)\n");
	}
#endif
	// publish the code tables for the emit kernel
	for (int i = lane; i < L_CODES; i += 64) { bt->lcode[i] = S.code[i]; bt->llen[i] = (uint8_t)S.len[i]; }
	if (lane < D_CODES) { bt->dcode[lane] = S.dcode[lane]; bt->dlen[lane] = (uint8_t)S.dlen[lane]; }
	TREE_PROBE_EXIT(s, m, a.max_blocks);
}

// ------------------------------------------------------------------ 5. Adler-32 + layout
__global__ void __launch_bounds__(256) dfl_adler_kernel(DeflateArgs a)
{
	__shared__ unsigned long long sa[256], sb[256];
	const int s = blockIdx.x;
	const uint32_t L = a.in_sizes[s];
	const uint8_t *in = a.in + (size_t)s * a.in_stride;
	unsigned long long A = 0, B = 0;
	// 16 bytes per step: A += sum d, B += (L - i0) * sum d - sum k * d_k.  Eight steps' loads are in flight together (the rolled
	// loop waited for each one: one workgroup per slice, nothing else hides the latency)
	const uint32_t nfull = L / 16;
	constexpr int U = 8;
	for (uint32_t g0 = threadIdx.x; g0 < nfull; g0 += blockDim.x * U) {
		uint4 v[U];
#pragma unroll
		for (int u = 0; u < U; u++) v[u] = *reinterpret_cast<const uint4 *>(in + (size_t)min(g0 + (uint32_t)u * blockDim.x, nfull - 1) * 16);
#pragma unroll
		for (int u = 0; u < U; u++) {
			const uint32_t g = g0 + (uint32_t)u * blockDim.x;
			if (g >= nfull) continue;
			const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
			uint32_t sd = 0, sk = 0;
#pragma unroll
			for (int k = 0; k < 16; k++) { const uint32_t d = (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu; sd += d; sk += (uint32_t)k * d; }
			A += sd;
			B += (unsigned long long)(L - g * 16) * sd - sk;
		}
	}
	if (threadIdx.x == 0)
		for (uint32_t i = nfull * 16; i < L; i++) { const unsigned long long d = in[i]; A += d; B += (unsigned long long)(L - i) * d; }
	sa[threadIdx.x] = A; sb[threadIdx.x] = B;
	__syncthreads();
	for (int st = 128; st > 0; st >>= 1) {
		if ((int)threadIdx.x < st) { sa[threadIdx.x] += sa[threadIdx.x + st]; sb[threadIdx.x] += sb[threadIdx.x + st]; }
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		const uint32_t lo = (uint32_t)((1ull + sa[0]) % 65521ull);
		const uint32_t hi = (uint32_t)(((unsigned long long)L + sb[0]) % 65521ull);
		a.adler[s] = (hi << 16) | lo;
	}
}

// bit offsets of every block, .cct header, zlib header, Adler trailer, final size: one wave per slice.  The blocks' records are
// loaded side by side, 64 at a time; only the running offset is serial (a stored block rounds it up to a byte), and that runs
// in registers.  (One lane per slice paid a memory round trip per block, one after the other.)
__global__ void __launch_bounds__(64) dfl_layout_kernel(DeflateArgs a, int n)
{
	const int s = blockIdx.x, lane = threadIdx.x;
	if (s >= n) return;
	uint8_t *out = a.out + (size_t)s * a.out_stride;
	BlockMeta *meta = a.block_meta + (size_t)s * a.max_blocks;
	const uint32_t nb = a.n_blocks[s];
	const uint32_t ad = a.adler[s];
	uint64_t bit = 8ull * 15;
	for (uint32_t m0 = 0; m0 < nb; m0 += 64) {
		const uint32_t m = m0 + (uint32_t)lane, cnt = min(64u, nb - m0);
		const BlockMeta bm = meta[min(m, nb - 1)];
		// bits of the block behind its 3 header bits (stored: behind the byte boundary that follows them -- _tr_stored_block:
		// 3 header bits, bi_windup, LEN, NLEN, bytes)
		const uint32_t flags = (bm.type == 0 ? 1u : 0u) | (bm.last ? 2u : 0u);
		const uint64_t size = bm.type == 0 ? 32 + 8ull * bm.stored_len : 3ull + bm.hdr_nbits + bm.body_bits;
		uint64_t mine = 0;
		for (uint32_t j = 0; j < cnt; j++) {
			const uint32_t fj = __shfl(flags, (int)j);
			const uint64_t zj = __shfl((unsigned long long)size, (int)j);
			if (j == (uint32_t)lane) mine = bit;
			bit = (fj & 1u) ? ((bit + 3 + 7) & ~7ull) + zj : bit + zj;
			if (fj & 2u) bit = (bit + 7) & ~7ull;  // bi_windup
		}
		if (m < nb) meta[m].bit_off = mine;
	}
	if (lane == 0) {
		for (int i = 0; i < 13; i++) out[i] = a.header13[i];
		out[13] = 0x78; out[14] = (uint8_t)a.zlib_flg;  // CMF/FLG for wbits 15 and the level (deflate.c:819-836)
		const uint64_t byte = bit >> 3;
		out[byte + 0] = (uint8_t)(ad >> 24); out[byte + 1] = (uint8_t)(ad >> 16);
		out[byte + 2] = (uint8_t)(ad >> 8);  out[byte + 3] = (uint8_t)ad;
		a.out_sizes[s] = (uint32_t)(byte + 4);
	}
}

// ------------------------------------------------------------------ 6. bit emission
__device__ __forceinline__ void or_bits(uint32_t *words, uint64_t bit, uint64_t value, int nbits)
{
	// value has nbits <= 48 significant bits; LSB-first packing (send_bits, trees.c:187-228)
	if (nbits == 0) return;
	const uint64_t w = bit >> 5;
	const int sh = (int)(bit & 31);
	const uint64_t lo = value << sh;                       // bits 0..63 of value << sh
	const uint64_t hi = sh ? (value >> (64 - sh)) : 0ull;  // bits 64.. (nbits <= 48, sh <= 31)
	atomicOr(&words[w], (uint32_t)lo);
	if (sh + nbits > 32) atomicOr(&words[w + 1], (uint32_t)(lo >> 32));
	if (sh + nbits > 64) atomicOr(&words[w + 2], (uint32_t)hi);
}

// A lane codes EMIT_K consecutive symbols and joins their bits in registers, so the workgroup scan, its barriers and the flush
// come once per EMIT_T symbols, and a lane ORs merged words into LDS (four 9-bit literals: two words) instead of every code.
#ifndef CCT_EMIT_K
#define CCT_EMIT_K 4
#endif
constexpr int EMIT_K = CCT_EMIT_K;
constexpr int EMIT_T = 256 * EMIT_K;                  // symbols per iteration of a workgroup
constexpr int EMIT_LIMBS = (EMIT_K * 48 + 63) / 64;   // 64-bit limbs of a lane's bit string (a symbol: <= 48 bits)
constexpr int EMIT_WBUF = EMIT_T * 48 / 32 + 8;       // words of an iteration: 31 bits of offset + EMIT_T * 48 bits, rounded up
__global__ void __launch_bounds__(256) dfl_emit_kernel(DeflateArgs a)
{
	__shared__ uint32_t wsum[2][4];
	const int s = blockIdx.y, m = blockIdx.x;
	if ((uint32_t)m >= a.n_blocks[s]) return;
	const BlockMeta bm = a.block_meta[(size_t)s * a.max_blocks + m];
	const BlockTables *bt = a.block_tables + ((size_t)s * a.max_blocks + m);
	uint8_t *out = a.out + (size_t)s * a.out_stride;
	uint32_t *words = reinterpret_cast<uint32_t *>(out);
	const uint8_t *in = a.in + (size_t)s * a.in_stride;
	uint64_t bit = bm.bit_off;
	if (bm.type == 0) {
		if (threadIdx.x == 0) or_bits(words, bit, (uint64_t)bm.last, 3);
		const uint64_t byte = ((bit + 3 + 7) & ~7ull) >> 3;
		if (threadIdx.x == 0) {
			out[byte] = (uint8_t)(bm.stored_len & 0xFF); out[byte + 1] = (uint8_t)(bm.stored_len >> 8);
			out[byte + 2] = (uint8_t)(~bm.stored_len & 0xFF); out[byte + 3] = (uint8_t)((~bm.stored_len >> 8) & 0xFF);
		}
		for (uint32_t i = threadIdx.x; i < bm.stored_len; i += blockDim.x) out[byte + 4 + i] = in[bm.in_begin + i];
		return;
	}
	if (threadIdx.x == 0) or_bits(words, bit, (uint64_t)((bm.type << 1) + bm.last), 3);
	bit += 3;
	if (bm.type == 2) {
		for (uint32_t i = threadIdx.x; i * 32 < bm.hdr_nbits; i += blockDim.x) {
			const int nb = (int)min(32u, bm.hdr_nbits - i * 32);
			or_bits(words, bit + 32ull * i, bt->hdr_bits[i], nb);
		}
		bit += bm.hdr_nbits;
	}
	const uint32_t *sym = a.sym + (size_t)s * a.in_stride + bm.first_sym;
	const bool dyn = bm.type == 2;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	// code tables of this block in LDS; code bits of EMIT_T symbols are merged into LDS words first, so the
	// output sees one store per 32-bit word instead of two or three atomics per symbol
	__shared__ uint16_t t_lcode[L_CODES + 2], t_dcode[D_CODES + 2];
	__shared__ uint8_t t_llen[L_CODES + 2], t_dlen[D_CODES + 2];
	__shared__ uint32_t wbuf[2][EMIT_WBUF];  // two iterations' words: one is flushed and zeroed while the next one fills the other
	// the symbol -> code tables of trees.c, staged in LDS: a __constant__ lookup with a per-lane index is a global
	// load, and every iteration with a match in it would wait for four of them in a row
	__shared__ uint8_t t_length_code[256], t_dist_code[512], t_extra_l[32], t_extra_d[32];
	__shared__ uint16_t t_base_length[32], t_base_dist[32];
	{  // every table entry this lane stages is requested before the first is stored (clamped indices, no branches around the
		// loads): one memory round trip instead of a dozen in a row.  blockDim.x == 256
		const int t = threadIdx.x, t2 = min(t + 256, L_CODES - 1), td = min(t, D_CODES - 1), t29 = min(t, 28), t30 = min(t, 29);
		const uint16_t *lsrc = dyn ? bt->lcode : c_static_lcode, *dsrc = dyn ? bt->dcode : c_static_dcode;
		const uint8_t *llsrc = dyn ? bt->llen : c_static_llen;
		const uint16_t lc0 = lsrc[t], lc1 = lsrc[t2];
		const uint8_t ll0 = llsrc[t], ll1 = llsrc[t2];
		const uint16_t dc = dsrc[td];
		uint8_t dl = bt->dlen[td];
		if (!dyn) dl = 5;
		const uint8_t k0 = c_dist_code[t], k1 = c_dist_code[t + 256], lcd = c_length_code[t];
		const uint8_t xl = c_extra_lbits[t29], xd = c_extra_dbits[t30];
		const uint16_t bl = c_base_length[t29], bd = c_base_dist[t30];
		t_lcode[t] = lc0; t_llen[t] = ll0;
		if (t + 256 < L_CODES) { t_lcode[t + 256] = lc1; t_llen[t + 256] = ll1; }
		if (t < D_CODES) { t_dcode[t] = dc; t_dlen[t] = dl; }
		t_dist_code[t] = k0; t_dist_code[t + 256] = k1; t_length_code[t] = lcd;
		if (t < 29) { t_extra_l[t] = xl; t_base_length[t] = bl; }
		if (t < 30) { t_extra_d[t] = xd; t_base_dist[t] = bd; }
	}
	for (int i = threadIdx.x; i < 2 * EMIT_WBUF; i += blockDim.x) (&wbuf[0][0])[i] = 0;
	__syncthreads();
	// the symbols of the next iteration are requested before these are coded (index clamped, not tested: a load inside a
	// conditional is waited for on the spot)
	const uint32_t last_sym = bm.nsym ? bm.nsym - 1 : 0;
	uint32_t vnext[EMIT_K];
#pragma unroll
	for (int k = 0; k < EMIT_K; k++) vnext[k] = sym[min((uint32_t)(threadIdx.x * EMIT_K + k), last_sym)];
	uint64_t run = bit;  // bit position of the iteration's first symbol, kept by every lane
	int par = 0;
	for (uint32_t base = 0; base <= bm.nsym; base += EMIT_T, par ^= 1) {  // one extra slot for END_BLOCK
		const uint32_t i0 = base + threadIdx.x * EMIT_K;
		uint32_t v[EMIT_K];
#pragma unroll
		for (int k = 0; k < EMIT_K; k++) v[k] = vnext[k];
#pragma unroll
		for (int k = 0; k < EMIT_K; k++) vnext[k] = sym[min(i0 + (uint32_t)(EMIT_T + k), last_sym)];
		// the lane's symbols back to back, from bit 0 of acc
		uint64_t acc[EMIT_LIMBS];
#pragma unroll
		for (int j = 0; j < EMIT_LIMBS; j++) acc[j] = 0;
		uint32_t ltot = 0;
#pragma unroll
		for (int k = 0; k < EMIT_K; k++) {
			const uint32_t i = i0 + k;
			uint64_t bits = 0;
			int nb = 0;
			if (i < bm.nsym) {
				uint32_t dist = v[k] >> 16;
				const uint32_t lc = v[k] & 0xFFu;
				if (dist == 0) {
					bits = t_lcode[lc];
					nb = t_llen[lc];
				} else {  // compress_block, trees.c:1070-1110
					int code = t_length_code[lc];
					const int lsym = code + 256 + 1;
					bits = t_lcode[lsym];
					nb = t_llen[lsym];
					int extra = t_extra_l[code];
					if (extra) { bits |= (uint64_t)(lc - t_base_length[code]) << nb; nb += extra; }
					dist--;
					code = dist < 256 ? t_dist_code[dist] : t_dist_code[256 + (dist >> 7)];
					bits |= (uint64_t)t_dcode[code] << nb;
					nb += t_dlen[code];
					extra = t_extra_d[code];
					if (extra) { bits |= (uint64_t)(dist - t_base_dist[code]) << nb; nb += extra; }
				}
			} else if (i == bm.nsym) {
				bits = t_lcode[END_BLOCK];
				nb = t_llen[END_BLOCK];
			}
			const uint32_t q = ltot >> 6, r = ltot & 63;
			const uint64_t lo = bits << r, hi = r ? bits >> (64 - r) : 0ull;
#pragma unroll
			for (int j = 0; j < EMIT_LIMBS; j++) {
				if (q == (uint32_t)j) acc[j] |= lo;
				if (q + 1 == (uint32_t)j) acc[j] |= hi;
			}
			ltot += (uint32_t)nb;
		}
		// exclusive scan of the lanes' bit counts over the workgroup.  Not wg_excl_scan: the wave sums alternate between two rows
		// like the word buffers, which saves its second barrier (see the end of the loop)
		const uint32_t inc = wave_incl_scan(ltot);
		if (lane == 63) wsum[par][wave] = inc;
		__syncthreads();
		uint32_t wb = 0, tot = 0;
		for (int w = 0; w < 4; w++) { if (w < wave) wb += wsum[par][w]; tot += wsum[par][w]; }
		uint32_t *wbf = wbuf[par];
		const uint32_t lbit = (uint32_t)(run & 31) + wb + inc - ltot;  // bit position inside wbuf
		if (ltot) {
			// acc << sh as 32-bit words: word j = a[j] << sh | a[j - 1] >> (32 - sh), with a[] the 32-bit halves of acc
			const uint32_t w0 = lbit >> 5, sh = lbit & 31, nw = (sh + ltot + 31) >> 5;
#pragma unroll
			for (int j = 0; j <= 2 * EMIT_LIMBS; j++) {
				const uint32_t aj = j < 2 * EMIT_LIMBS ? (uint32_t)(acc[j >> 1] >> (32 * (j & 1))) : 0u;
				const uint32_t ap = j > 0 ? (uint32_t)(acc[(j - 1) >> 1] >> (32 * ((j - 1) & 1))) : 0u;
				const uint32_t w = (uint32_t)((((uint64_t)aj << 32) | ap) >> (32 - sh));
				if ((uint32_t)j < nw && w) atomicOr(&wbf[w0 + j], w);  // (the first and the last word are shared with the neighbours)
			}
		}
		__syncthreads();
		// the words strictly inside the iteration's bit range are its own: plain stores, zeros included.  The first and the last
		// are shared with the header, the neighbouring iterations, the next block or the trailer
		const uint32_t nwords = ((uint32_t)(run & 31) + tot + 31) >> 5;
		const uint64_t gw = run >> 5;
		for (uint32_t k = threadIdx.x; k < nwords; k += blockDim.x) {
			const uint32_t w = wbf[k];
			wbf[k] = 0;
			if (k == 0 || k == nwords - 1) { if (w) atomicOr(&words[gw + k], w); }
			else words[gw + k] = w;
		}
		run += tot;
		// (no barrier here: the next iteration fills the other buffer and the other wsum row, and comes back to these only after
		// its own two barriers)
	}
}

// files back to back (exclusive scan of sizes by one workgroup: chunks of 256 with a running carry, then a grid copy) for ONE
// device->host copy
__global__ void __launch_bounds__(256) dfl_pack_offsets_kernel(const uint32_t *sizes, int n, uint64_t *offsets, int exact)
{
	__shared__ uint64_t wsum[4];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	uint64_t carry = 0;
	for (int base = 0; base < n; base += 256) {
		const int i = base + t;
		const uint32_t sz = i < n ? sizes[i] : 0u;
		const uint64_t v = exact ? sz : (uint64_t)((sz + 15u) & ~15u);
		// wg_excl_scan written out: no test reaches offsets past 2^32, so this kernel is checked by its instructions staying what
		// they were, and the helper's second barrier in front of the store (here it follows it) changes them
		const uint64_t inc = wave_incl_scan(v);
		if (lane == 63) wsum[wave] = inc;
		__syncthreads();
		uint64_t wb = 0, tot = 0;
		for (int w = 0; w < 4; w++) { if (w < wave) wb += wsum[w]; tot += wsum[w]; }
		if (i < n) offsets[i] = carry + wb + inc - v;
		carry += tot;
		__syncthreads();
	}
	if (t == 0) offsets[n] = carry;
}
__global__ void __launch_bounds__(256) dfl_pack_kernel(const uint8_t *src, size_t stride, const uint32_t *sizes,
                                                       const uint64_t *offsets, uint8_t *dst)
{
	const int s = blockIdx.y;
	const uint32_t n16 = (sizes[s] + 15u) >> 4;
	const uint4 *in = reinterpret_cast<const uint4 *>(src + (size_t)s * stride);
	uint4 *out = reinterpret_cast<uint4 *>(dst + offsets[s]);
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += gridDim.x * blockDim.x) out[i] = in[i];
}

__global__ void dfl_offsets2_kernel(DeflateArgs a, int n)
{
	// blk_entry := "not entered" for the walk kernel
	const size_t per = dfl_blk_words(a.in_stride);
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)n * per; i += (size_t)gridDim.x * blockDim.x)
		a.blk_entry[i] = 0xFFFFFFFFu;
}

__global__ void dfl_offsets_kernel(DeflateArgs a, int n)
{
	if (blockIdx.x == 0) {
		for (int s = threadIdx.x; s < n; s += blockDim.x) { a.postloop_lit[s] = 0; a.heavy_count[s] = 0; a.deep_count[s] = 0; a.run_end_count[s] = 0; }  // (run_end_count: an empty slice has no chunk that would write it)
		if (threadIdx.x == 0) *a.gen = *a.gen % GEN_MAX + 1u;  // tag of this pass's match records (see MatchRec)
	}
	// sort histograms and, right behind them (dfl_bind), the run-list counters of dfl_run_len_kernel (a memset node of a few
	// megabytes at the head of the graph waited for the copy engine: with the files of the pass before still on the wire a pass
	// of 1024^2 slices started 3 ms late)
	const size_t nrc = dfl_hist_words((size_t)n, (size_t)a.run_chunks);
	for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nrc; t += (size_t)gridDim.x * blockDim.x) a.sort_hist[t] = 0;
}

// Zeroes of the output, by need: dfl_layout_kernel's trailer and dfl_emit_kernel OR their bits into zeros, and nothing before
// the layout kernel reads `out`.  A file is at most 13 + zlib_bound(in_size, memLevel) bytes; the slack covers the
// 32-bit words of or_bits / dfl_emit_kernel that straddle the end and the 16-byte units dfl_pack_kernel copies.  Beyond that the
// stride keeps whatever the pass before left there: nobody reads it.  W: bytes per store, 16 when the stride allows it.
constexpr uint32_t CLEAR_SLACK = 64;
__device__ __forceinline__ size_t clear_bytes(const DeflateArgs &a, int s)
{
	// mirrors zlib_bound(L, memLevel == 8) of deflate_workspace.h, written out: through the call the compiler orders this kernel's
	// scalar instructions differently (12 more bytes of code), and device code stays as it is
	const size_t L = a.in_sizes[s];
	const size_t bound = a.block_syms == (uint32_t)BLOCK_SYMS ? L + (L >> 12) + (L >> 14) + (L >> 25) + 13
	                                                          : L + ((L + 7) >> 3) + ((L + 63) >> 6) + 5 + 6;
	return min(a.out_stride, (13 + bound + CLEAR_SLACK + 15) & ~(size_t)15);
}
template <typename W>
__global__ void __launch_bounds__(256) dfl_clear_kernel(DeflateArgs a)
{
	const int s = blockIdx.y;
	const size_t units = clear_bytes(a, s) / sizeof(W);  // (the stride is a multiple of sizeof(W): launch_clear)
	W *out = reinterpret_cast<W *>(a.out + (size_t)s * a.out_stride);
	W zero{};
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < units; i += (size_t)gridDim.x * blockDim.x) out[i] = zero;
}
static void launch_clear(const DeflateArgs &a, int n, hipStream_t st)
{
	if (a.out_stride % 16 == 0 && (uintptr_t)a.out % 16 == 0) hipLaunchKernelGGL(dfl_clear_kernel<uint4>, dim3(16, n), dim3(256), 0, st, a);
	else hipLaunchKernelGGL(dfl_clear_kernel<uint32_t>, dim3(32, n), dim3(256), 0, st, a);
}

}  // namespace

// deflate.c configuration_table (the deflate_slow levels) and the zlib header's level_flags
bool deflate_level_args(int level, DeflateArgs &a)
{
	static const uint32_t T[6][5] = {
		{4, 4, 16, 16, 0x5E}, {8, 16, 32, 32, 0x5E}, {8, 16, 128, 128, 0x9C},
		{8, 32, 128, 256, 0xDA}, {32, 128, 258, 1024, 0xDA}, {32, 258, 258, 4096, 0xDA},
	};
	if (level < 4 || level > 9) return false;
	const uint32_t *t = T[level - 4];
	a.good = t[0]; a.max_lazy = t[1]; a.nice = t[2]; a.max_chain = t[3]; a.zlib_flg = t[4];
	return true;
}

// (level, strategy) -> DeflateArgs.  deflate.c: level_flags is 0 for strategy >= Z_HUFFMAN_ONLY (Z_FIXED included) or level < 2;
// deflate_huff and deflate_rle read no configuration_table entry, so every level 1 .. 9 gives the same stream (and graph)
bool deflate_strategy_args(int level, int strategy, DeflateArgs &a)
{
	if (strategy < 0 || strategy > (int)Z_FIXED) return false;
	a.strategy = (uint32_t)strategy;
	a.min_len = strategy == (int)Z_FILTERED ? 6u : (uint32_t)MIN_MATCH;
	if (short_pass((uint32_t)strategy)) {
		if (level < 1 || level > 9) return false;
		a.good = a.max_lazy = a.nice = a.max_chain = 0;
		a.zlib_flg = 0x01;
		return true;
	}
	if (!deflate_level_args(level, a)) return false;
	if (strategy == (int)Z_FIXED) a.zlib_flg = 0x01;
	return true;
}

// deflate.c deflateInit2: hash_bits = memLevel + 7, lit_bufsize = 1 << (memLevel + 6) (a block ends after lit_bufsize - 1 symbols)
bool deflate_mem_level_args(int mem_level, DeflateArgs &a)
{
	if (mem_level != 8 && mem_level != 9) return false;
	a.hash_bits = (uint32_t)mem_level + 7u;
	a.block_syms = (1u << (mem_level + 6)) - 1u;
	return true;
}

static int g_tree_cus = 0;  // CUs of the device (deflate_init_tables; launch_tree)
// host: trees.c tr_static_init tables -> constant memory
hipError_t deflate_init_tables()
{
	uint8_t length_code[256]; uint16_t base_length[29]; uint8_t dist_code[512]; uint16_t base_dist[30];
	uint16_t static_lcode[288]; uint8_t static_llen[288]; uint16_t static_dcode[30];
	static const int xl[29] = {0,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,0};
	static const int xd[30] = {0,0,0,0,1,1,2,2,3,3,4,4,5,5,6,6,7,7,8,8,9,9,10,10,11,11,12,12,13,13};
	int length = 0, code, n, dist = 0;
	for (code = 0; code < 28; code++) {
		base_length[code] = (uint16_t)length;
		for (n = 0; n < (1 << xl[code]); n++) length_code[length++] = (uint8_t)code;
	}
	length_code[length - 1] = (uint8_t)code;
	base_length[28] = 0;
	for (code = 0; code < 16; code++) {
		base_dist[code] = (uint16_t)dist;
		for (n = 0; n < (1 << xd[code]); n++) dist_code[dist++] = (uint8_t)code;
	}
	dist >>= 7;
	for (; code < 30; code++) {
		base_dist[code] = (uint16_t)(dist << 7);
		for (n = 0; n < (1 << (xd[code] - 7)); n++) dist_code[256 + dist++] = (uint8_t)code;
	}
	uint16_t bl_count[16] = {0}, next_code[16];
	n = 0;
	while (n <= 143) { static_llen[n++] = 8; bl_count[8]++; }
	while (n <= 255) { static_llen[n++] = 9; bl_count[9]++; }
	while (n <= 279) { static_llen[n++] = 7; bl_count[7]++; }
	while (n <= 287) { static_llen[n++] = 8; bl_count[8]++; }
	unsigned c = 0;
	for (int bits = 1; bits <= 15; bits++) { c = (c + bl_count[bits - 1]) << 1; next_code[bits] = (uint16_t)c; }
	auto rev = [](unsigned v, int len) { unsigned r = 0; do { r |= v & 1; v >>= 1; r <<= 1; } while (--len > 0); return r >> 1; };
	for (n = 0; n < 288; n++) static_lcode[n] = (uint16_t)rev(next_code[static_llen[n]]++, static_llen[n]);
	for (n = 0; n < 30; n++) static_dcode[n] = (uint16_t)rev((unsigned)n, 5);
	hipError_t e;
	if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_length_code), length_code, sizeof length_code)) != hipSuccess) return e;
	if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_base_length), base_length, sizeof base_length)) != hipSuccess) return e;
	if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_dist_code), dist_code, sizeof dist_code)) != hipSuccess) return e;
	if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_base_dist), base_dist, sizeof base_dist)) != hipSuccess) return e;
	if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_static_lcode), static_lcode, sizeof static_lcode)) != hipSuccess) return e;
	if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_static_llen), static_llen, sizeof static_llen)) != hipSuccess) return e;
	if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_static_dcode), static_dcode, sizeof static_dcode)) != hipSuccess) return e;
	// (once per process, not per launch: launch_tree)
	int dev;
	if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
	if ((e = hipDeviceGetAttribute(&g_tree_cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
	return hipFuncSetAttribute(reinterpret_cast<const void *>(dfl_tree_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize,
	                           (int)(16 * sizeof(TreeScratch)));
}

// The tree kernel at a.tree_waves waves per workgroup, slices the fast grid index (dfl_tree_kernel).  Sixteen waves are faster
// where they apply and much slower where they do not: a workgroup of sixteen claims the LDS of a whole CU, so a CU holds as
// many tree waves as that chunk of its slice has blocks (one wave per workgroup: up to 20), and the workgroups that have a
// block must fit the CUs in one round.  Measured, dfl_tree_kernel in us at 1 / 16 waves (profiles/tree_placement.log):
// 256 slices of 13 blocks 375 / 357, of 2 blocks 278 / 280; 300 slices of 13 blocks 382 / 700; 512 slices of 52 blocks
// 1965 / 2644; 2048 slices of 1 block 214 / 1358; and with few slices thirteen waves on each of a few CUs lose to one or two on
// many, 64 slices of 13 blocks 324 / 334 (128: 359 / 337).  So, for a.tree_waves == 0: one wave below TREE_WAVES16_MIN_SLICES
// and above one slice per CU, where sixteen cannot win; in between the device chooses, because only it knows how many blocks
// the slices have (the host knows max_blocks, a bound from the stride that is 34 where the bench payloads have 13): both
// instantiations are launched and the one not chosen leaves at once.  launch_deflate refuses any value but 0, 1 and 16
// before it launches a kernel; the LDS limit of dfl_tree_kernel<16> is raised once, by deflate_init_tables.
constexpr int TREE_WAVES16_MIN_SLICES = 128;
template <int WAVES>
static void launch_tree_waves(const DeflateArgs &a, int n, hipStream_t st)
{
	// slices are the fast grid index: the workgroups that have blocks then follow each other in dispatch order whatever
	// max_blocks is.  (Blocks first for the one-wave kernel where there are more slices than CUs, the order it used to have,
	// was tried and gained nothing: 300 slices of 13 blocks 501 us against 386, 2048 of 3 blocks 687 against 692.)
	hipLaunchKernelGGL(dfl_tree_kernel<WAVES>, dim3(n, (a.max_blocks + WAVES - 1) / WAVES), dim3(64 * WAVES),
	                   WAVES * sizeof(TreeScratch), st, a, (uint32_t)g_tree_cus);
}
static void launch_tree(const DeflateArgs &a0, int n, hipStream_t st)
{
	DeflateArgs a = a0;
	if (a.tree_waves == 0 && (n < TREE_WAVES16_MIN_SLICES || n > g_tree_cus)) a.tree_waves = 1;
	if (a.tree_waves != 1) launch_tree_waves<16>(a, n, st);
	if (a.tree_waves != 16) launch_tree_waves<1>(a, n, st);
}

// One DEFLATE pass.  `side` + `ev` (four events without timing), when given, let kernels that do not depend on each other share
// the chip: the run lists are written while the match kernel runs (its waves fill the chip, so the side kernels mostly end
// with it -- but they no longer come after it), and the two tail-bound matchers (long chains: a few waves walking thousands
// of entries; runs: a binary search + scan per position) run side by side, with the Adler-32 sums behind the shorter one --
//     main:  run lengths, sort A, sort B ─┬─ match ─────┬─ run matcher ──────────┬─ decisions, walk, symbols, trees, emit
//     side:                               └─ run lists, ─┴─ heavy matcher, Adler ─┘
//                                            clear, blk_entry
// Under stream capture this becomes the same fork / join in the graph.  Next to the SORT passes nothing may run: pass B took
// 0.60 instead of 0.34 ms beside the run-list kernels (profiles/r03_deflate_fork.log).
//
// The short pass of Z_RLE / Z_HUFFMAN_ONLY has no hash chains: no sort, no match kernels, no run lists.  Z_RLE keeps the run-length
// words (without the sort's histograms), its own greedy parse, the walk and the symbols kernel; Z_HUFFMAN_ONLY writes its symbols
// directly.  Both then share the trees, layout and emit of the long pass.  It has no side branch: everything but the Adler-32 sums
// depends on the kernel before it, and the sums are a small fraction of the pass, so it runs on `st` alone whether or not a side
// stream is given.
static hipError_t launch_deflate_short(const DeflateArgs &a, int n, hipStream_t st)
{
	const bool ml9 = a.block_syms == (uint32_t)BLOCK_SYMS_ML9;
	const int gx = (int)std::min<size_t>(64, (a.in_stride + 255) / 256);
	launch_clear(a, n, st);
	if (a.strategy == Z_RLE) {
		hipLaunchKernelGGL((dfl_run_len_kernel<false, 15>), dim3(gx, n), dim3(256), 0, st, a);  // run-length words
		hipLaunchKernelGGL(dfl_rle_rec_kernel, dim3(gx, n), dim3(256), 0, st, a);
		hipLaunchKernelGGL(dfl_offsets2_kernel, dim3(256), dim3(256), 0, st, a, n);
		hipLaunchKernelGGL(dfl_walk_kernel, dim3(n), dim3(WALK_T), 0, st, a, n);
		if (ml9) hipLaunchKernelGGL(dfl_symbols_kernel<BLOCK_SYMS_ML9>, dim3(gx, n), dim3(256), 0, st, a);
		else hipLaunchKernelGGL(dfl_symbols_kernel<BLOCK_SYMS>, dim3(gx, n), dim3(256), 0, st, a);
	} else {
		if (ml9) hipLaunchKernelGGL(dfl_huff_symbols_kernel<BLOCK_SYMS_ML9>, dim3(gx, n), dim3(256), 0, st, a);
		else hipLaunchKernelGGL(dfl_huff_symbols_kernel<BLOCK_SYMS>, dim3(gx, n), dim3(256), 0, st, a);
	}
	hipLaunchKernelGGL(dfl_adler_kernel, dim3(n), dim3(256), 0, st, a);
	launch_tree(a, n, st);
	hipLaunchKernelGGL(dfl_layout_kernel, dim3(n), dim3(64), 0, st, a, n);
	hipLaunchKernelGGL(dfl_emit_kernel, dim3(a.max_blocks, n), dim3(256), 0, st, a);
	return hipGetLastError();
}

hipError_t launch_deflate(const DeflateArgs &a, int n, hipStream_t st, hipStream_t side, const hipEvent_t *ev)
{
	hipError_t e;
	const bool ml9 = a.hash_bits == 16;
	if ((a.hash_bits != 15 && !ml9) || a.block_syms != (uint32_t)(ml9 ? BLOCK_SYMS_ML9 : BLOCK_SYMS)) return hipErrorInvalidValue;
	if (ml9 && a.pos_mask != 0xFFFFFFFFu) return hipErrorInvalidValue;  // memLevel 9: wide records only ("Sort records")
	if ((a.out_stride & 3) || ((uintptr_t)a.out & 3)) return hipErrorInvalidValue;
	if (a.tree_waves != 0 && a.tree_waves != 1 && a.tree_waves != 16) return hipErrorInvalidValue;
	if (short_pass(a.strategy)) return launch_deflate_short(a, n, st);
	hipLaunchKernelGGL(dfl_offsets_kernel, dim3(64), dim3(256), 0, st, a, n);  // (also zeroes sort_hist and run_counts)
	const int gx = (int)std::min<size_t>(64, (a.in_stride + 255) / 256);
	if (ml9) {
		hipLaunchKernelGGL((dfl_run_len_kernel<true, 16>), dim3(gx, n), dim3(256), 0, st, a);
		hipLaunchKernelGGL((dfl_sort_pass_kernel<true, 16>), dim3(n), dim3(1024), 0, st, a);
		hipLaunchKernelGGL((dfl_sort_pass_kernel<false, 16>), dim3(n), dim3(1024), 0, st, a);
	} else {
		hipLaunchKernelGGL((dfl_run_len_kernel<true, 15>), dim3(gx, n), dim3(256), 0, st, a);       // run-length words, sort histograms, run-list counts
		hipLaunchKernelGGL((dfl_sort_pass_kernel<true, 15>), dim3(n), dim3(1024), 0, st, a);   // in -> rec_in by hash & 255
		hipLaunchKernelGGL((dfl_sort_pass_kernel<false, 15>), dim3(n), dim3(1024), 0, st, a);  // -> rec_out by hash >> 8
	}
	const bool fork = side != nullptr && ev != nullptr;
	hipStream_t s2 = fork ? side : st;
	if (fork) {
		if ((e = hipEventRecord(ev[0], st)) != hipSuccess) return e;
		if ((e = hipStreamWaitEvent(s2, ev[0], 0)) != hipSuccess) return e;
	}
	hipLaunchKernelGGL(dfl_run_lists_kernel, dim3(a.run_chunks, n), dim3(256), 0, s2, a);
	hipLaunchKernelGGL(dfl_run_info_kernel, dim3(8, n), dim3(256), 0, s2, a);
	// neither depends on anything before it: beside the match kernel, whose waves mostly wait, they are off the
	// serial path (the clear takes 30 us here and 11 us alone; the pass is shorter this way)
	launch_clear(a, n, s2);
	hipLaunchKernelGGL(dfl_offsets2_kernel, dim3(256), dim3(256), 0, s2, a, n);
	// wide records: one 256-lane block per 256 positions (more of them in flight hide the scattered accesses better than grid-stride
	// loops).  Compact records: the kernel's waves mostly wait, and with the next turn's records in flight a wave
	// that makes more turns wastes less of its life on its entry and its last flush, so a slice gets as few workgroups as still
	// fill an XCD (256 of them) with the slices it works through, xcd_slice(): DFL_MATCH_GRID of them in a large batch (33 turns
	// on a bench payload; 256 slices: 426 us against 445 / 437 / 509 / 553 with 16 / 64 / 128 / 256 and 485 with 8,
	// profiles/match_prefetch_sweeps.log), 256 for up to eight slices as before
	const int n8 = (n + 7) & ~7;  // see xcd_slice()
	const int gm_cap = a.pos_mask == COMPACT_POS_MASK ? std::max(DFL_MATCH_GRID, 256 / std::max(1, n8 / 8)) : 2048;
	const int gm = (int)std::min<size_t>(gm_cap, (a.in_stride + 255) / 256);
	if (a.max_chain < 16 || a.max_chain > 4096 || a.nice < 16 || a.nice > (uint32_t)MAX_MATCH) return hipErrorInvalidValue;  // levels 4 .. 9
	const bool ql = (a.max_chain >> 2) <= (uint32_t)LIGHT_STEPS;  // the quarter chain ends inside the light walk
	if (a.pos_mask == COMPACT_POS_MASK) {
		if (ql) hipLaunchKernelGGL((dfl_match_kernel<true, true>), dim3(gm, n8), dim3(256), 0, st, a, n);
		else hipLaunchKernelGGL((dfl_match_kernel<true, false>), dim3(gm, n8), dim3(256), 0, st, a, n);
	} else if (a.pos_mask == 0xFFFFFFFFu) {
		if (ql) hipLaunchKernelGGL((dfl_match_kernel<false, true>), dim3(gm, n8), dim3(256), 0, st, a, n);
		else hipLaunchKernelGGL((dfl_match_kernel<false, false>), dim3(gm, n8), dim3(256), 0, st, a, n);
	} else return hipErrorInvalidValue;
	if (fork) {  // both have what the other produced: the run matcher the run lists, the heavy matcher the queue of long chains
		if ((e = hipEventRecord(ev[1], st)) != hipSuccess) return e;
		if ((e = hipEventRecord(ev[2], s2)) != hipSuccess) return e;
		if ((e = hipStreamWaitEvent(s2, ev[1], 0)) != hipSuccess) return e;
		if ((e = hipStreamWaitEvent(st, ev[2], 0)) != hipSuccess) return e;
	}
	hipLaunchKernelGGL(dfl_match_heavy_kernel, dim3(gx, n8), dim3(256), 0, s2, a, n);
	hipLaunchKernelGGL(dfl_adler_kernel, dim3(n), dim3(256), 0, s2, a);
	hipLaunchKernelGGL(dfl_match_run_kernel, dim3(gx, n8), dim3(256), 0, st, a, n);
	if (fork) {
		if ((e = hipEventRecord(ev[3], s2)) != hipSuccess) return e;
		if ((e = hipStreamWaitEvent(st, ev[3], 0)) != hipSuccess) return e;
	}
	hipLaunchKernelGGL(dfl_rec_kernel, dim3(gx, n), dim3(256), 0, st, a);
	hipLaunchKernelGGL(dfl_walk_kernel, dim3(n), dim3(WALK_T), 0, st, a, n);
	if (ml9) hipLaunchKernelGGL(dfl_symbols_kernel<BLOCK_SYMS_ML9>, dim3(gx, n), dim3(256), 0, st, a);
	else hipLaunchKernelGGL(dfl_symbols_kernel<BLOCK_SYMS>, dim3(gx, n), dim3(256), 0, st, a);
	launch_tree(a, n, st);
	hipLaunchKernelGGL(dfl_layout_kernel, dim3(n), dim3(64), 0, st, a, n);
	hipLaunchKernelGGL(dfl_emit_kernel, dim3(a.max_blocks, n), dim3(256), 0, st, a);
	return hipGetLastError();
}

// exact = 1: files touch each other (archive layout), so a destination has any alignment.  The source is dword-aligned (the
// stride is a multiple of 4): aligned destination dwords are composed from two source dwords, and only the bytes before the
// first and after the last aligned dword of a file are stored one at a time.  A composed dword reads its second source dword
// only when it takes bytes from it (head != 0), and then that dword starts inside the file: nothing beyond the stride is read.
__global__ void __launch_bounds__(256) dfl_pack_exact_kernel(const uint8_t *src, size_t stride, const uint32_t *sizes,
                                                             const uint64_t *offsets, uint8_t *dst)
{
	const int s = blockIdx.y;
	const uint32_t nbytes = sizes[s];
	const uint8_t *in = src + (size_t)s * stride;
	uint8_t *out = dst + offsets[s];
	const uint32_t head = min((uint32_t)(-(uintptr_t)out & 3u), nbytes);  // bytes before the first aligned destination dword
	const uint32_t nd = (nbytes - head) >> 2;                            // aligned destination dwords
	const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
	const uint32_t *in32 = reinterpret_cast<const uint32_t *>(in);
	uint32_t *out32 = reinterpret_cast<uint32_t *>(out + head);
	const uint32_t sh = 8u * head, up = head ? 1u : 0u;
	for (uint32_t j = tid; j < nd; j += nth) {  // destination bytes head + 4j .. + 3 = source bytes of dwords j and j + 1
		const uint64_t pair = ((uint64_t)in32[j + up] << 32) | in32[j];
		out32[j] = (uint32_t)(pair >> sh);
	}
	const uint32_t tail0 = head + 4u * nd;
	if (tid < head) out[tid] = in[tid];
	if (tid < nbytes - tail0) out[tail0 + tid] = in[tail0 + tid];
}

hipError_t launch_pack(const uint8_t *src, size_t stride, const uint32_t *sizes, int n, uint64_t *offsets, uint8_t *dst,
                       int exact, hipStream_t st)
{
	hipLaunchKernelGGL(dfl_pack_offsets_kernel, dim3(1), dim3(256), 0, st, sizes, n, offsets, exact);
	if (exact) hipLaunchKernelGGL(dfl_pack_exact_kernel, dim3(32, n), dim3(256), 0, st, src, stride, sizes, offsets, dst);
	else hipLaunchKernelGGL(dfl_pack_kernel, dim3(16, n), dim3(256), 0, st, src, stride, sizes, offsets, dst);
	return hipGetLastError();
}

}  // namespace cct
