// Host model of the pipelined heap replay of dfl_tree_kernel (csrc/deflate_kernels.hip, tree_heap), checked against a
// plain sequential replay of zlib 1.2.11 build_tree (trees.c:625-668).
//
// The kernel replays trees.c's heap with several sifts in flight, one lane per sift.  This program runs the same tick
// schedule with the lanes emulated by a loop -- every lane reads, then every lane writes, as one ds_read / ds_write
// instruction of a wave does -- and compares the result with the sequential replay: the heap tail (the order tree_fix's
// overflow repair walks), dad[], freq[], depths and the final heap.  It also checks, tick by tick, that no lane reads a
// slot another lane writes in the same tick and that no two lanes write the same slot.
//
//   build:  c++ -O2 -std=c++17 -o tree_schedule_model tools/tree_schedule_model.cpp
//   run:    tree_schedule_model --builtin          every heap size 2..286 and the tie-heavy families
//           tree_schedule_model < histograms       one histogram per line: "elems f0 f1 ... f(elems-1)"
// Output: one line per case set, "ok <cases> seq_levels <n> fixed_levels <n> ticks <n> ..." or "FAIL ..." (exit 1).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr int L_CODES = 286, HEAP_SIZE = 2 * L_CODES + 1;
constexpr int HEAP_SLOTS = HEAP_SIZE + 3;  // as TreeScratch::heap
constexpr int LANES = 8;                   // sift slots in flight (the kernel's TREE_SIFTS)

struct Result {
	std::vector<int> heap_tail;  // node ids at heap[heap_max .. HEAP_SIZE-1]
	std::vector<int> dad, freq, depth;
	long levels = 0;        // sequential: child-pair reads of trees.c's loops (early exit)
	long fixed_levels = 0;  // sequential: levels the one-lane kernel ran (sift_root reads floor(log2 heap_len) child pairs)
	long heapify_levels = 0;
	long ticks = 0, heapify_ticks = 0, stall_ticks = 0;
	int max_in_flight = 0;
};

// ---- plain trees.c, node ids in the heap, smaller() on freq then depth
Result seq_build(const std::vector<int> &f0, int elems)
{
	Result r;
	std::vector<int> freq(HEAP_SIZE, 0), dad(HEAP_SIZE, 0), depth(HEAP_SIZE, 0), heap(HEAP_SIZE + 1, 0);
	for (int n = 0; n < elems; n++) freq[n] = f0[n];
	int heap_len = 0, heap_max = HEAP_SIZE, max_code = -1;
	for (int n = 0; n < elems; n++)
		if (freq[n]) heap[++heap_len] = max_code = n;
	while (heap_len < 2) {
		const int node = heap[++heap_len] = max_code < 2 ? ++max_code : 0;
		freq[node] = 1;
	}
	auto smaller = [&](int n, int m) { return freq[n] < freq[m] || (freq[n] == freq[m] && depth[n] <= depth[m]); };
	auto down = [&](int k, long &lv) {
		int v = heap[k], j = k << 1;
		while (j <= heap_len) {
			lv++;
			if (j < heap_len && smaller(heap[j + 1], heap[j])) j++;
			if (smaller(v, heap[j])) break;
			heap[k] = heap[j]; k = j; j <<= 1;
		}
		heap[k] = v;
	};
	auto fixed = [&](int hl) { long l = 0; while ((2 << l) <= hl) l++; return l; };
	for (int n = heap_len / 2; n >= 1; n--) down(n, r.heapify_levels);
	int node = elems;
	do {
		const int n = heap[1];
		heap[1] = heap[heap_len--];
		down(1, r.levels); r.fixed_levels += fixed(heap_len);
		const int m = heap[1];
		heap[--heap_max] = n; heap[--heap_max] = m;
		freq[node] = freq[n] + freq[m];
		depth[node] = (depth[n] >= depth[m] ? depth[n] : depth[m]) + 1;
		dad[n] = dad[m] = node;
		heap[1] = node++;
		down(1, r.levels); r.fixed_levels += fixed(heap_len);
	} while (heap_len >= 2);
	heap[--heap_max] = heap[1];
	for (int h = heap_max; h < HEAP_SIZE; h++) r.heap_tail.push_back(heap[h]);
	r.dad = dad; r.freq = freq; r.depth = depth;
	return r;
}

// ---- the kernel's schedule: entries freq << 15 | depth << 10 | node, smaller(a, b) is a <= (b | 1023)
struct Fail { std::string what; };

Result pipe_build(const std::vector<int> &f0, int elems)
{
	Result r;
	std::vector<uint32_t> heap(HEAP_SLOTS, 0xDEADBEEFu);
	std::vector<int> freq(HEAP_SIZE, 0), dad(HEAP_SIZE, 0);
	for (int n = 0; n < elems; n++) freq[n] = f0[n];
	int h = 0, max_code = -1;
	for (int n = 0; n < elems; n++)
		if (freq[n]) { heap[1 + h++] = ((uint32_t)freq[n] << 15) | (uint32_t)n; max_code = n; }
	while (h < 2) {
		const int node = max_code < 2 ? ++max_code : 0;
		freq[node] = 1;
		heap[++h] = (1u << 15) | (uint32_t)node;
	}
	// 1. heapify: trees.c visits every node of a depth before any node above it, and the nodes of one depth have disjoint
	// subtrees, so one round per depth sifts all of them at once (one lane each; lanes of a round advance in lockstep)
	{
		int dmax = 0;
		while ((2 << dmax) <= h / 2) dmax++;
		for (int d = dmax; d >= 0; d--) {
			const int lo = 1 << d, hi = std::min((2 << d) - 1, h / 2);
			for (int n0 = lo; n0 <= hi; n0 += 64) {
				const int cnt = std::min(64, hi - n0 + 1);
				std::vector<uint32_t> v(cnt);
				std::vector<int> k(cnt);
				std::vector<char> mv(cnt, 1);
				for (int i = 0; i < cnt; i++) { k[i] = n0 + i; v[i] = heap[k[i]]; }
				for (bool any = true; any;) {
					any = false;
					std::vector<uint32_t> x(cnt), y(cnt);
					for (int i = 0; i < cnt; i++)  // reads
						if (mv[i] && 2 * k[i] <= h) { x[i] = heap[2 * k[i]]; y[i] = heap[2 * k[i] + 1]; }
					for (int i = 0; i < cnt; i++) {  // writes
						if (!mv[i]) continue;
						const int j = 2 * k[i];
						const bool right = j < h && y[i] <= (x[i] | 1023u);
						const uint32_t e = right ? y[i] : x[i];
						const bool go = j <= h && v[i] > (e | 1023u);
						heap[k[i]] = go ? e : v[i];
						if (go) k[i] = j + right; else mv[i] = 0;
					}
					r.heapify_ticks++;
					for (int i = 0; i < cnt; i++) any |= mv[i] != 0;
				}
			}
		}
	}
	// 2. the main loop: sifts A (pqremove: heap[h] sinks from the root) and B (the new node sinks from the root) in the
	// order trees.c runs them, a new one every other tick at the earliest
	uint32_t v[LANES] = {}, k[LANES] = {}, hl[LANES] = {};
	bool moving[LANES] = {};
	int node = elems, hm = HEAP_SIZE, slot = 0;
	bool next_b = false, done = false;
	long t = 0, last_start = -2;
	uint32_t en = heap[1], newv = 0;
	for (;;) {
		int start = -1;  // 0: A, 1: B
		if (!done && t - last_start >= 2) {
			if (next_b) start = 1;
			else {
				// A takes the last slot h: only when h is outside the subtree of every moving sift's hole
				bool hazard = false;
				for (int i = 0; i < LANES; i++) {
					if (!moving[i]) continue;
					if (k[i] > (uint32_t)h) throw Fail{"hole beyond heap_len"};
					const int dd = __builtin_clz(k[i]) - __builtin_clz((uint32_t)h);
					if (((uint32_t)h >> dd) == k[i]) hazard = true;
				}
				if (hazard) r.stall_ticks++;
				else start = 0;
			}
		}
		if (start >= 0) {
			if (moving[slot]) throw Fail{"slot still busy"};
			if (start == 0) { v[slot] = heap[h]; hl[slot] = (uint32_t)--h; }
			else { v[slot] = newv; hl[slot] = (uint32_t)h; }
			k[slot] = 1; moving[slot] = true;
		}
		// one level of every moving sift: all reads, then all writes
		uint32_t x[LANES], y[LANES], w[LANES];
		int rd[2 * LANES], nrd = 0, wr[LANES], nwr = 0;
		for (int i = 0; i < LANES; i++) {
			if (!moving[i]) continue;
			const uint32_t j = 2 * k[i];
			x[i] = heap[j]; y[i] = heap[j + 1];
			if (j <= hl[i]) rd[nrd++] = (int)j;
			if (j < hl[i]) rd[nrd++] = (int)j + 1;
		}
		for (int i = 0; i < LANES; i++) {
			if (!moving[i]) continue;
			const uint32_t j = 2 * k[i];
			const bool right = j < hl[i] && y[i] <= (x[i] | 1023u);
			const uint32_t e = right ? y[i] : x[i];
			const bool go = j <= hl[i] && v[i] > (e | 1023u);
			w[i] = go ? e : v[i];
			heap[k[i]] = w[i];
			wr[nwr++] = (int)k[i];
			if (go) k[i] = j + right; else moving[i] = false;
		}
		for (int a = 0; a < nwr; a++) {
			for (int b = a + 1; b < nwr; b++) if (wr[a] == wr[b]) throw Fail{"two lanes write one slot"};
			for (int b = 0; b < nrd; b++) if (wr[a] == rd[b]) throw Fail{"a lane reads a slot written in the same tick"};
		}
		int inflight = 0;
		for (int i = 0; i < LANES; i++) inflight += moving[i];
		r.max_in_flight = std::max(r.max_in_flight, inflight + (start >= 0 && !moving[slot] ? 1 : 0));
		t++;
		if (start == 0) {  // pqremove done at the root: the two nodes are known, the new node is built off the chain
			const uint32_t em = w[slot];
			const int n = (int)(en & 1023u), m = (int)(em & 1023u);
			heap[--hm] = en; heap[--hm] = em;
			const uint32_t f = (en >> 15) + (em >> 15);
			const uint32_t dn = (en >> 10) & 31u, dm = (em >> 10) & 31u;
			const uint32_t d = (dn >= dm ? dn : dm) + 1;
			freq[node] = (int)f;
			dad[n] = dad[m] = node;
			newv = (f << 15) | (d << 10) | (uint32_t)node;
			next_b = true; last_start = t - 1; slot = (slot + 1) % LANES;
		} else if (start == 1) {
			en = w[slot];
			node++;
			next_b = false; last_start = t - 1; slot = (slot + 1) % LANES;
			if (h < 2) done = true;
		}
		bool any = false;
		for (int i = 0; i < LANES; i++) any |= moving[i];
		if (done && !any) break;
	}
	heap[--hm] = en;
	r.ticks = t;
	for (int i = hm; i < HEAP_SIZE; i++) r.heap_tail.push_back((int)(heap[i] & 1023u));
	r.dad = dad; r.freq = freq;
	r.depth.assign(HEAP_SIZE, 0);
	for (int i = hm; i < HEAP_SIZE; i++) r.depth[heap[i] & 1023u] = (int)((heap[i] >> 10) & 31u);
	return r;
}

struct Totals { long cases = 0, levels = 0, fixed = 0, hlevels = 0, ticks = 0, hticks = 0, stalls = 0; int inflight = 0; };

bool check(const std::vector<int> &f, int elems, Totals &T, const char *what)
{
	const Result s = seq_build(f, elems);
	Result p;
	try { p = pipe_build(f, elems); } catch (const Fail &e) {
		std::printf("FAIL %s case %ld: %s\n", what, T.cases, e.what.c_str());
		return false;
	}
	const char *bad = nullptr;
	if (s.heap_tail != p.heap_tail) bad = "heap tail";
	else if (s.dad != p.dad) bad = "dad";
	else if (s.freq != p.freq) bad = "freq";
	else
		for (int n : s.heap_tail) if (s.depth[n] != p.depth[n]) bad = "depth";
	if (bad) {
		std::printf("FAIL %s case %ld: %s differs (elems %d)\n", what, T.cases, bad, elems);
		return false;
	}
	T.cases++; T.levels += s.levels; T.fixed += s.fixed_levels; T.hlevels += s.heapify_levels;
	T.ticks += p.ticks; T.hticks += p.heapify_ticks; T.stalls += p.stall_ticks;
	T.inflight = std::max(T.inflight, p.max_in_flight);
	return true;
}

void report(const char *what, const Totals &T)
{
	const double c = T.cases ? (double)T.cases : 1.0;
	std::printf("ok %s cases %ld  per tree: seq_levels %.1f fixed_levels %.1f heapify_levels %.1f | ticks %.1f "
	            "heapify_ticks %.1f stall_ticks %.1f max_in_flight %d | fixed/ticks %.2f\n",
	            what, T.cases, T.levels / c, T.fixed / c, T.hlevels / c, T.ticks / c, T.hticks / c, T.stalls / c, T.inflight,
	            (double)(T.fixed + T.hlevels) / (double)(T.ticks + T.hticks));
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % n); }

// nz non-zero symbols spread over `elems` (positions random, values from gen), total kept <= 16384 as in a block
template <class G> std::vector<int> family(int elems, int nz, G gen)
{
	std::vector<int> f(elems, 0);
	std::vector<int> pos(elems);
	for (int i = 0; i < elems; i++) pos[i] = i;
	for (int i = elems - 1; i > 0; i--) std::swap(pos[i], pos[rnd((uint32_t)i + 1)]);
	long tot = 0;
	for (int i = 0; i < nz; i++) { f[pos[i]] = gen(i); tot += f[pos[i]]; }
	while (tot > 16384) {
		tot = 0;
		for (int i = 0; i < elems; i++) { if (f[i] > 1) f[i] = (f[i] + 1) / 2; tot += f[i]; }
	}
	return f;
}

}  // namespace

int main(int argc, char **argv)
{
	bool ok = true;
	if (argc > 1 && !std::strcmp(argv[1], "--builtin")) {
		const int elems = L_CODES;
		Totals sizes, ones, two, geo, pairs, rnd_t, small;
		for (int nz = 2; nz <= L_CODES; nz++) {
			for (int rep = 0; rep < 3; rep++) {
				ok &= check(family(elems, nz, [](int) { return 1 + (int)rnd(200); }), elems, sizes, "sizes");
				ok &= check(family(elems, nz, [](int) { return 1; }), elems, ones, "all_ones");
				ok &= check(family(elems, nz, [](int) { return rnd(2) ? 3 : 7; }), elems, two, "two_values");
				ok &= check(family(elems, nz, [](int i) { return 1 << std::min(i / 3, 13); }), elems, geo, "geometric");
				ok &= check(family(elems, nz, [](int i) { return 1 + i / 2; }), elems, pairs, "equal_pairs");
				ok &= check(family(elems, nz, [](int) { return 1 + (int)rnd(1 + rnd(4000)); }), elems, rnd_t, "random");
			}
		}
		for (int elems2 : {30, 19})  // distance and bit-length alphabets, including one or no used symbol
			for (int nz = 0; nz <= elems2; nz++)
				for (int rep = 0; rep < 4; rep++)
					ok &= check(family(elems2, nz, [](int) { return 1 + (int)rnd(rnd(2) ? 3 : 500); }), elems2, small, "small");
		if (ok) {
			report("sizes", sizes); report("all_ones", ones); report("two_values", two);
			report("geometric", geo); report("equal_pairs", pairs); report("random", rnd_t); report("small", small);
		}
		return ok ? 0 : 1;
	}
	// histograms from stdin
	Totals T;
	char line[1 << 16];
	while (std::fgets(line, sizeof line, stdin)) {
		char *p = line, *e;
		const long elems = std::strtol(p, &e, 10);
		if (e == p) continue;
		p = e;
		std::vector<int> f;
		for (long i = 0; i < elems; i++) { f.push_back((int)std::strtol(p, &e, 10)); p = e; }
		ok &= check(f, (int)elems, T, "stdin");
	}
	if (ok) report("stdin", T);
	return ok ? 0 : 1;
}
