// Host side of libcompact_hip.so: device context, traversal-table cache, workspaces, the
// DEFLATE/INFLATE stage (system libz on a host thread team -- the same library the reference
// reaches through CPython's zlib module, core.py:340,421) and the extern "C" entry points
// declared in include/compact_hip.h.
#include <dlfcn.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/compact_hip.h"
#include "cct_internal.h"
#include "host.h"
#include "handoff.h"

namespace cct {
bool gilbert_table(int width, int height, int32_t *out);

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	return code;
}

std::mutex g_mu;

namespace {

struct ShapeTables {  // everything that depends on (width, height) only; lives in HBM
	int32_t *d_lut = nullptr;  // traversal order O[N]
	bool tiled = false;        // traversal = aligned 64x64 tiles -> encode_tiles_kernel applies
	int n_tiles = 0, n_orient = 0;
	uint32_t *d_org = nullptr;
	uint8_t *d_orient = nullptr;
	uint16_t *d_pat = nullptr;
	// decode_kernel's block path: every 16 traversal positions are an aligned 4x4 square of the raster (dec_block_words)
	bool dec_blocks = false;
	uint32_t *d_blk = nullptr;
	// streaming kernel (encode_stream.hip): every tile is a 16x16 grid of 4x4-pixel traversal blocks
	bool stream = false;
	uint32_t *d_ptab = nullptr;       // n_orient * 128 * 4
	uint32_t *d_otab = nullptr;       // 4 * 16
	uint32_t *d_ttab = nullptr;       // 16 * 4
	uint32_t *d_htab = nullptr;       // n_orient * 32 * 2: the look-ahead quadrant of a tile
	StreamTiles tiles;                // host copy: travels in the kernel arguments
};

// What an encode call still uses after it has given its slot to the next call ("queue ahead", encode_batch_impl): the next
// call records and copies into the slot's other set meanwhile.  Two per slot; handoff.h says who owns which, and until when.
struct HandoffSet {
	EventPair stage, pass;        // timing: around the transform+pack stage, around the device DEFLATE pass
	hipEvent_t landed = nullptr;  // sizes and status have reached `landing`
	DevBuf landing;               // pinned: a call's sizes / status / statistics (a copy to pageable memory blocks the host until it has happened)
	DevBuf packed;                // the packed archive of a pass: it leaves the device on the copy stream, after the slot has been released
	hipEvent_t ev_packed = nullptr, ev_copied = nullptr;  // created with the slot's copy stream (pack_enqueue)
	HandoffSet() { landing.pinned_host = true; }
	int create()  // ensure_ctx: no steady-state call creates an event
	{
		for (hipEvent_t *e : {&stage.e0, &stage.e1, &pass.e0, &pass.e1}) HIP_TRY(hipEventCreate(e));
		HIP_TRY(hipEventCreateWithFlags(&landed, hipEventDisableTiming));
		return CCT_OK;
	}
	void release()  // cct_shutdown, every stream drained
	{
		stage.release(); pass.release(); landing.release(); packed.release();
		for (hipEvent_t *e : {&landed, &ev_packed, &ev_copied}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
	}
};

// Everything one encode batch in flight owns: stream, workspaces, the captured DEFLATE graph.  There are two of them.
// Several kernels of the DEFLATE pass are latency-bound and leave most of the chip idle (the Huffman tree kernel runs one
// serial heap replay per block for over a millisecond; the match kernel waits on scattered loads), so a second batch on a
// stream of its own fills the gaps: two callers get two slots and their kernel chains interleave on the device.
struct EncSlot {
	std::mutex *mu = nullptr;      // slot 0: g_mu (it shares the main stream with the plumbing calls), slot 1: its own
	hipStream_t stream = nullptr;  // slot 0: the main stream
	// the ~25 launches of one DEFLATE pass, captured once per argument set and replayed as a graph: fewer host
	// calls and no dispatch gaps between the kernels when a decode shares the queue processor
	struct ZGraph { std::vector<uint8_t> key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; uint64_t last_use = 0; };
	std::vector<ZGraph> z_graphs;  // a batch deflated in several passes has one argument set per pass (round 2 kept ONE graph and
	uint64_t z_clock = 0;          // captured it again for every pass of such a batch: 5 ms per step at 512 x 1024^2)
	// packed archives leave the device on their own stream from the packed buffer of a hand-off set, after the slot has
	// been released: the next encode call may start its kernels while this one's files are still on the wire
	hipStream_t stream_copy = nullptr;
	HandoffSet sets[2];
	// encode workspaces
	DevBuf e_role, e_lidx, e_lmask, e_lcur, e_images, e_payload, e_sizes, e_status, e_stats;
	DevBuf e_pairrec, e_hand;  // streaming kernel: meshed-pair records, hand-off words and tickets
	DevBuf h_stage;  // pinned host staging (payloads)
	DevBuf z_ws[DFL_REGIONS];  // workspace of the device DEFLATE pass, one buffer per region of deflate_workspace.h
	DevBuf z_out, z_outsizes, z_in, z_insizes, z_packed, z_packoffs;  // its input and output, and the packed files
	DevBuf png_img, png_out, png_sizes;  // PNG writer: rasters from the host, files, their sizes (cct_png_encode_batch, cct_png_encode8_batch)
	// match records are valid by tag (deflate_kernels.hip MatchRec): the device counter (region DFL_R_GEN) has run z_gen_passes
	// times since the buffer z_mr_cleared (region DFL_R_MATCH at that time) was last zeroed together with it
	const void *z_mr_cleared = nullptr;
	size_t z_mr_cleared_cap = 0;
	unsigned z_gen_passes = 0;
	hipStream_t stream_side = nullptr;  // side branch of the DEFLATE pass (launch_deflate)
	hipEvent_t ev_fork[4] = {nullptr, nullptr, nullptr, nullptr};
	EventPair ev_zlib;  // around the DEFLATE pass of cct_zlib_compress_batch*
	DevBuf *all_bufs[48];
	int n_bufs = 0;
	EncSlot()
	{
		DevBuf *b[] = {&e_role, &e_lidx, &e_lmask, &e_lcur, &e_images, &e_payload, &e_sizes, &e_status, &e_stats, &e_pairrec,
		               &e_hand, &h_stage, &z_out, &z_outsizes, &z_in, &z_insizes, &z_packed, &z_packoffs,
		               &png_img, &png_out, &png_sizes};
		for (DevBuf *p : b) all_bufs[n_bufs++] = p;
		for (DevBuf &w : z_ws) all_bufs[n_bufs++] = &w;  // cct_shutdown releases them with the rest
		h_stage.pinned_host = true;
	}
	EncSlot(const EncSlot &) = delete;
	EncSlot &operator=(const EncSlot &) = delete;
};
constexpr int N_ENC_SLOTS = 2;

// The same for a decode batch in flight (cct_decode_batch, cct_zlib_decompress_batch): stream, workspaces, events.  With two of
// them the archive upload of one batch runs under the INFLATE and decode kernels of the other (what bounds a decode-only
// caller: BASELINE configs[4]).
struct DecSlot {
	hipStream_t stream = nullptr;  // slot 0: Context::stream_dec
	DevBuf d_role, d_slot, d_jord, d_jval, d_payload, d_sizes, d_status, d_images, d_pcache;
	DevBuf d_arch, d_archoffs, d_zstatus;
	DevBuf d_png_z, d_png_tab, d_png_bpp;  // PNG reader: gathered zlib streams, chunk table, bytes per sample (cct_png_read_batch)
	DevBuf dh_stage;  // pinned host staging of inflated payloads (host INFLATE path)
	hipEvent_t ev_d0 = nullptr, ev_d1 = nullptr, ev_k_dec0 = nullptr, ev_k_dec1 = nullptr;
	hipEvent_t ev_ws = nullptr;  // recorded after a launch on ANOTHER stream that uses this slot's workspaces (cct_decode_payload_dev)
	DevBuf *all_bufs[16];
	int n_bufs = 0;
	DecSlot()
	{
		DevBuf *b[] = {&d_role, &d_slot, &d_jord, &d_jval, &d_payload, &d_sizes, &d_status, &d_images, &d_pcache, &d_arch, &d_archoffs,
		               &d_zstatus, &dh_stage, &d_png_z, &d_png_tab, &d_png_bpp};
		for (DevBuf *p : b) all_bufs[n_bufs++] = p;
		dh_stage.pinned_host = true;
	}
	void release()  // cct_shutdown, the stream drained
	{
		for (int i = 0; i < n_bufs; i++) all_bufs[i]->release();
		for (hipEvent_t *e : {&ev_d0, &ev_d1, &ev_k_dec0, &ev_k_dec1, &ev_ws}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
	}
	DecSlot(const DecSlot &) = delete;
	DecSlot &operator=(const DecSlot &) = delete;
};
constexpr int N_DEC_SLOTS = DEC_SLOTS;

struct Context {
	bool ready = false;
	pid_t pid = 0;
	int device = -1;
	hipStream_t stream = nullptr;  // main stream: plumbing calls, cct_encode_payload_dev, encode slot 0
	int use_graph = 1;
	int deflate_fork = 1;   // independent kernels of the DEFLATE pass on a side branch (launch_deflate)
	int queue_ahead = 1;    // an encode call hands its slot on before it waits for the sizes (encode_batch_impl)
	int decode_yields = 1;  // decode kernels issued next to an encode wait for the next transform+pack stage to end (cct_decode_batch)
	int tree_waves = 0;     // option "tree_waves": waves per workgroup of dfl_tree_kernel, 1 or 16; 0 = chosen per pass (deflate_kernels.hip launch_tree)
	int compact_recs = 1;  // sort records that carry the first five string bytes (slices below 4 MiB; deflate_kernels.hip "Sort records")
	int enc_slots = 1;  // option "encode_slots": encode batches on the device at a time.  Default 1: on two of the three boxes
	                    // measured a second batch in flight cost more (each kernel slows down next to another batch's
	                    // DEFLATE pass) than it filled (bench.py reports both settings: stages.other_encode_slot_setting)
	hipStream_t stream_dec = nullptr;  // decode runs on its own stream so it can overlap an encode in flight
	std::map<std::pair<int, int>, ShapeTables> luts;  // (width,height) -> device tables
	int use_tiles = 1;  // option "tile_path": 1 default choice among the tile paths (the streaming kernel wherever it applies), 4 the
	                    // streaming kernel (encode_stream.hip), 2 the one-workgroup-per-slice tile kernel, 0 the generic LUT-gather
	                    // kernel (3, the four-kernel pipeline of round 2, is removed and refused)
	int stream_tpg = STREAM_TPG;  // tuning option "stream_tpg": tiles per workgroup of the streaming kernel (1, 2, 4)
	int last_path = -1; // read-only option "last_encode_path": which stage (i) implementation the last encode used (0 generic, 2 tile kernel, 3 streaming kernel,
	                    // 4 generic kernel with a run-time block size; 1, the removed pipeline, is not reused)
	int runtime_bs = 0;  // option "runtime_block_size": 1 sends every block size through the run-time block size kernels (encode_kernel<0>,
	                     // decode_kernel<0>), which otherwise run the sizes that are not powers of two only; for cross-checks and measurements
	int last_dec_path = -1;  // read-only option "last_decode_path": 0 a decode_kernel compiled for the block size, 1 the run-time block size kernel
	int last_dec_block_path = -1;  // read-only option "last_decode_block_path": 1 the last decode launch placed whole 4x4 blocks (decode_kernel<16, true, true>)
	int dbg_skip = 0;   // option "debug_skip", tuning build only (tuning.h): phase-ablation mask (outputs invalid when set)
	int tuning_build = TUNING;  // read-only option "tuning_build", tuning build only: how a tool asks which library it loaded
	int device_deflate = 1;  // option "device_deflate": 0 = DEFLATE stage on the host thread team (libz)
	int device_inflate = 1;  // option "device_inflate": 1 = INFLATE on the device (inflate_kernels.hip, speculative lane-parallel
	                         // decode), 0 = libz on the host thread team (same bytes; bounded by the host CPUs the process may use)
	int zlib_threads = 0;
	int wg_threads = 1024;
	int dec_slots = N_DEC_SLOTS;  // option "decode_slots"
	int inflate_lanes = 0;  // option "inflate_lanes": 256 / 512 lanes per stream in the INFLATE kernel, 0 = 512 unless an encode call is
	                        // in flight (next to an encode batch the narrower workgroup is the faster one, see inflate_kernels.hip)
	int last_inflate_lanes = 0;  // read-only option "last_inflate_lanes"
	int png_unfilter_waves = PNG_UNFILTER_WAVES;  // option "png_unfilter_waves": waves per image of png_unfilter_kernel (1, 2, 4, 8)
};
std::atomic<int> g_encodes_in_flight{0};
// gate between the decode and the encode stream (sched_kernels.hip): device counters and what has been issued so far
uint32_t *g_gate = nullptr;
std::atomic<uint32_t> g_gate_passes_issued{0};
struct EncodeInFlight {
	EncodeInFlight() { g_encodes_in_flight.fetch_add(1, std::memory_order_relaxed); }
	~EncodeInFlight() { g_encodes_in_flight.fetch_sub(1, std::memory_order_relaxed); }
};

bool trace_on()  // CCT_TRACE (tuning.h): host timings of every batch call on stderr
{
	return tuning_env("CCT_TRACE", 0) != 0;
}

double now_ms()
{
	using namespace std::chrono;
	return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

Context g_ctx;
}  // namespace
QuiesceLock g_quiesce;
thread_local int tl_api_depth = 0;
namespace {
int inflate_lanes_now()
{
	const int lanes = g_ctx.inflate_lanes ? g_ctx.inflate_lanes : (g_encodes_in_flight.load(std::memory_order_relaxed) > 0 ? 256 : 512);
	g_ctx.last_inflate_lanes = lanes;
	return lanes;
}
EncSlot *g_enc = new EncSlot[N_ENC_SLOTS];
DecSlot *g_dec = new DecSlot[N_DEC_SLOTS];
void reset_ctx()
{
	g_ctx = Context();
	delete[] g_enc; g_enc = new EncSlot[N_ENC_SLOTS];
	delete[] g_dec; g_dec = new DecSlot[N_DEC_SLOTS];
}
// timings of the calling thread's most recent batch call (cct_last_timings): per thread, so that an encode and a
// decode driven from two threads do not overwrite each other's numbers
thread_local float tl_enc_kernel_ms = 0, tl_dec_kernel_ms = 0, tl_d2h_ms = 0, tl_deflate_ms = 0, tl_inflate_ms = 0, tl_h2d_ms = 0;
std::mutex g_mu1;     // encode slot 1
HandoffRing g_handoff[N_ENC_SLOTS];  // who owns which of EncSlot::sets; like the slot mutexes they outlive reset_ctx()
std::mutex g_mu_dec[N_DEC_SLOTS];  // the decode slots; like g_mu / g_mu1 they outlive reset_ctx(), which replaces the slot objects
std::mutex g_mu_lut;  // the per-shape table cache (taken after g_mu by encode, alone by decode)

int default_device()
{
	const char *lr = getenv("LOCAL_RANK");
	return lr ? atoi(lr) : 0;
}

}  // namespace

int ensure_ctx(int device)
{
	if (g_ctx.ready && g_ctx.pid != getpid()) {
		// A child forked AFTER the parent initialised the device inherits a HIP runtime it cannot use (ROCm does not
		// support that state, and re-creating the context on top of it is not safe either).  Callers that fan work out over
		// processes (scripts/evaluate.py:107) must fork before the first device call: each child then initialises its own.
		return fail(CCT_E_DEVICE, "this process was forked after the library had initialised the GPU in its parent (pid %d): "
		                          "fork workers before the first cct_* device call", (int)g_ctx.pid);
	}
	if (g_ctx.ready) {
		if (device >= 0 && device != g_ctx.device)
			return fail(CCT_E_ARG, "library already bound to device %d", g_ctx.device);
		HIP_TRY(hipSetDevice(g_ctx.device));
		return CCT_OK;
	}
	// The runtime spreads a process's streams over GPU_MAX_HW_QUEUES hardware queues (default 4).  The library keeps up to eight
	// streams busy (two encode slots with copy and side streams, two decode slots, the size gather), and two streams on one queue
	// run one after the other: with a stream more than before, the packed-archive copy and the next DEFLATE pass shared a queue
	// and a 1024^2 pass started 3 ms late (BASELINE configs[3]: 14.9 K instead of 17 K MPixels/s); with another assignment the
	// side branch of a pass shared one with the decode (configs[1]: DEFLATE 4.1 instead of 3.6 ms).  Eight queues, unless the
	// user has set the variable; it is read when the runtime initialises, i.e. by the first HIP call of the process below.
	setenv("GPU_MAX_HW_QUEUES", "8", 0);
	int count = 0;
	hipError_t e = hipGetDeviceCount(&count);
	if (e != hipSuccess || count <= 0)
		return fail(CCT_E_DEVICE, "no HIP device available (%s); libcompact_hip has no CPU fallback",
		            e == hipSuccess ? "device count 0" : hipGetErrorString(e));
	const int dev = device >= 0 ? device : default_device();
	if (dev >= count) return fail(CCT_E_DEVICE, "device %d requested but only %d visible", dev, count);
	HIP_TRY(hipSetDevice(dev));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, dev));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return fail(CCT_E_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code only", dev, prop.gcnArchName);
	HIP_TRY(hipStreamCreateWithFlags(&g_ctx.stream, hipStreamNonBlocking));
	HIP_TRY(hipStreamCreateWithFlags(&g_ctx.stream_dec, hipStreamNonBlocking));
	for (int k = 0; k < N_ENC_SLOTS; k++) {
		EncSlot &E = g_enc[k];
		E.mu = k == 0 ? &g_mu : &g_mu1;
		if (k == 0) E.stream = g_ctx.stream;
		else HIP_TRY(hipStreamCreateWithFlags(&E.stream, hipStreamNonBlocking));
		for (HandoffSet &S : E.sets)
			if (int rc = S.create()) return rc;
		for (int q = 0; q < 4; q++) HIP_TRY(hipEventCreateWithFlags(&E.ev_fork[q], hipEventDisableTiming));
	}
	for (int k = 0; k < N_DEC_SLOTS; k++) {
		DecSlot &D = g_dec[k];
		if (k == 0) D.stream = g_ctx.stream_dec;
		else HIP_TRY(hipStreamCreateWithFlags(&D.stream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreate(&D.ev_d0));
		HIP_TRY(hipEventCreate(&D.ev_d1));
		HIP_TRY(hipEventCreate(&D.ev_k_dec0));
		HIP_TRY(hipEventCreate(&D.ev_k_dec1));
		HIP_TRY(hipEventCreateWithFlags(&D.ev_ws, hipEventDisableTiming));
	}
	HIP_TRY(deflate_init_tables());  // __constant__ tables of the DEFLATE kernels, shared by both encode slots
	HIP_TRY(hipMalloc(&g_gate, 256));
	HIP_TRY(hipMemset(g_gate, 0, 256));
	g_gate_passes_issued = 0;
	g_ctx.device = dev;
	g_ctx.pid = getpid();
	if (g_ctx.zlib_threads <= 0) {
		// host team size: the CPUs this process may actually use.  Under a cgroup CPU quota (cpu.max) more
		// runnable threads than about twice the quota only get the whole process throttled.
		unsigned hc = std::thread::hardware_concurrency();
		int nt = hc ? (int)hc : 1;
		if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
			long long quota = 0, period = 0;
			if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0)
				nt = std::min(nt, (int)std::max<long long>(1, 2 * ((quota + period - 1) / period)));
			fclose(f);
		}
		g_ctx.zlib_threads = nt;
	}
	g_ctx.ready = true;
	return CCT_OK;
}

hipStream_t main_stream() { return g_ctx.stream; }
int bound_device() { return g_ctx.device; }
bool forked_after_init() { return g_ctx.ready && g_ctx.pid != getpid(); }

namespace {

// Tables of the streaming kernel.  Inside every 64x64 tile the traversal must walk aligned 4x4-pixel blocks (16
// positions each), and every block must be walked quadrant by quadrant (2x2 pixels, 4 positions each) with quarter 0
// = top-left or bottom-right quadrant, quarter 2 = the other one, quarter 1 = bottom-left or top-right, quarter 3 = the
// other one.  The generalized Hilbert curve on power-of-two squares does; anything else keeps the older kernels.
void build_stream_tables(const std::vector<int32_t> &O, int width, const std::vector<uint32_t> &org,
                         const std::vector<uint8_t> &orient, ShapeTables &t)
{
	t.stream = false;
	const int nt = (int)org.size();
	const int no = t.n_orient;
	std::vector<uint16_t> rtab((size_t)no * 256, 0xFFFF);
	std::vector<uint32_t> tile_last(no, 0);
	std::vector<std::vector<int>> bpat;  // block orientations: raster index (row*4+col) of the 16 positions
	for (int ti = 0; ti < nt; ti++) {
		const int32_t *k = O.data() + (size_t)ti * 4096;
		const int to = orient[ti];
		for (int b = 0; b < 256; b++) {
			int lo = k[b * 16];
			for (int i = 1; i < 16; i++) lo = std::min(lo, k[b * 16 + i]);
			const int d0 = lo - (int)org[ti];
			const int by4 = d0 / width, bx4 = d0 % width;
			if (by4 % 4 || bx4 % 4 || by4 >= 64 || bx4 >= 64) return;
			std::vector<int> pat(16);
			for (int i = 0; i < 16; i++) {
				const int d = k[b * 16 + i] - lo, dy = d / width, dx = d % width;
				if (dx >= 4 || dy >= 4) return;
				pat[i] = dy * 4 + dx;
			}
			int bo = -1;
			for (size_t q = 0; q < bpat.size(); q++) if (bpat[q] == pat) { bo = (int)q; break; }
			if (bo < 0) { if (bpat.size() == 4) return; bpat.push_back(pat); bo = (int)bpat.size() - 1; }
			const uint16_t ent = (uint16_t)(b | (bo << 8));
			uint16_t &slot = rtab[(size_t)to * 256 + (by4 / 4) * 16 + bx4 / 4];
			if (slot != 0xFFFF && slot != ent) return;  // tiles of one orientation must agree
			slot = ent;
		}
		tile_last[to] = (uint32_t)(k[4095] - (int)org[ti]);
	}
	for (uint16_t e : rtab) if (e == 0xFFFF) return;
	// one entry per block pair of a tile
	std::vector<uint32_t> ptab((size_t)no * 128 * 4, 0);
	{
		std::vector<int> done(no, 0);
		for (int ti = 0; ti < nt; ti++) {
			const int to = orient[ti];
			if (done[to]) continue;
			done[to] = 1;
			const int32_t *k = O.data() + (size_t)ti * 4096;
			for (int lane = 0; lane < 128; lane++) {
				const int by = lane >> 3, bxp = lane & 7;
				uint32_t *e = ptab.data() + ((size_t)to * 128 + lane) * 4;
				e[0] = (uint32_t)rtab[(size_t)to * 256 + by * 16 + 2 * bxp] | (uint32_t)rtab[(size_t)to * 256 + by * 16 + 2 * bxp + 1] << 16;
				for (int h = 0; h < 2; h++) {
					const int kb = (int)((e[0] >> (16 * h)) & 0xFF);
					e[1 + h] = kb == 0 ? 0xFFFFFFFFu : (uint32_t)(k[kb * 16 - 1] - (int)org[ti]);
				}
			}
		}
	}
	// half tiles: the block pairs whose blocks lie in the first / second 128 traversal blocks
	for (int to = 0; to < no; to++)
		for (int half = 0; half < 2; half++) {
			uint32_t reg[64];  // raster offset inside the tile of every such pair's 8x4-pixel region, raster order
			int cnt = 0;
			for (int lane = 0; lane < 128; lane++) {
				const uint32_t *e = ptab.data() + ((size_t)to * 128 + lane) * 4;
				const int ka = (int)(e[0] & 0xFF), kb = (int)((e[0] >> 16) & 0xFF);
				if ((ka >> 7) != (kb >> 7)) return;  // a pair of blocks straddles the halves: not the structure assumed
				if ((ka >> 7) != half) continue;
				if (cnt == 64) return;
				reg[cnt++] = (uint32_t)((lane >> 3) * 4 * width + (lane & 7) * 8);
			}
			if (cnt != 64) return;
			// the half must be a 64x32 (block rows r0..r0+7) or a 32x64 (block-pair columns c0..c0+3) rectangle
			bool rect = false;
			for (int vertical = 0; vertical < 2 && !rect; vertical++)
				for (int first = 0; first < 16 && !rect; first += vertical ? 4 : 8) {
					bool ok = true;
					for (int l = 0; l < 64 && ok; l++) {
						const uint32_t want = vertical ? (uint32_t)((l >> 2) * 4 * width + (first + (l & 3)) * 8)
						                               : (uint32_t)((first + (l >> 3)) * 4 * width + (l & 7) * 8);
						ok = reg[l] == want;
					}
					rect = ok;
				}
			if (!rect) return;
		}
	if (nt > 256) return;
	for (int ti = 0; ti < nt; ti++) {
		if (org[ti] >= (1u << 24)) return;
		t.tiles.orgo[ti] = org[ti] | ((uint32_t)orient[ti] << 24);
	}
	for (int to = 0; to < no; to++) t.tiles.last[to] = tile_last[to];
	std::vector<uint32_t> otab(64, 0);
	for (size_t bo = 0; bo < bpat.size(); bo++) {
		const std::vector<int> &pat = bpat[bo];
		int quad[4];
		for (int q = 0; q < 4; q++) {
			const int r = pat[4 * q] / 4, c = pat[4 * q] % 4;
			quad[q] = (r >> 1) * 2 + (c >> 1);  // 0 TL, 1 TR, 2 BL, 3 BR
			for (int i = 1; i < 4; i++)
				if (((pat[4 * q + i] / 4) >> 1) * 2 + ((pat[4 * q + i] % 4) >> 1) != quad[q]) return;
		}
		if (!((quad[0] == 0 && quad[2] == 3) || (quad[0] == 3 && quad[2] == 0))) return;
		if (!((quad[1] == 2 && quad[3] == 1) || (quad[1] == 1 && quad[3] == 2))) return;
		uint32_t *ot = otab.data() + bo * 16;
		for (int j = 0; j < 8; j++) {
			uint32_t sel = 0;
			for (int h = 0; h < 2; h++) {
				const int r = pat[2 * j + h] / 4, c = pat[2 * j + h] % 4;
				const uint32_t byte0 = (uint32_t)((r & 1) * 4 + (c & 1) * 2);  // v_perm source: top dword bytes 0-3, bottom 4-7
				sel |= (byte0 | ((byte0 + 1) << 8)) << (16 * h);
			}
			ot[j] = sel;
		}
		ot[8] = (quad[0] == 3 ? 1u : 0u) | (quad[1] == 1 ? 2u : 0u);
	}
	// token bytes of a 4-pixel group by its two-byte mask: v_perm selectors over {X: bytes 4-7, P: bytes 0-3}
	std::vector<uint32_t> ttab(64, 0);
	for (int f = 0; f < 16; f++) {
		uint8_t seq[8];
		int n = 0;
		for (int px = 0; px < 4; px++) { if (f >> px & 1) seq[n++] = (uint8_t)(4 + px); seq[n++] = (uint8_t)px; }
		for (int i = n; i < 8; i++) seq[i] = 0x0C;  // constant 0x00
		ttab[f * 4 + 0] = seq[0] | seq[1] << 8 | seq[2] << 16 | (uint32_t)seq[3] << 24;
		ttab[f * 4 + 1] = seq[4] | seq[5] << 8 | seq[6] << 16 | (uint32_t)seq[7] << 24;
		ttab[f * 4 + 2] = (uint32_t)n;
		uint32_t keep = 0x7F7F7F7Fu;  // bits of the deltas' low bytes that reach the stream: 7 of a short token, 8 of a full token's second byte
		for (int px = 0; px < 4; px++) if (f >> px & 1) keep |= 0x80u << (8 * px);
		ttab[f * 4 + 3] = keep;
	}
	// the first 64 traversal blocks of a tile (the look-ahead of the previous tile's mesh search): a 32x32-pixel quadrant, 8
	// block rows of 4 block pairs.  Entry (row * 4 + pair) of htab is the pair's ptab word; the quadrant's origin inside the
	// tile travels in the kernel arguments (tiles.qorg), so the rows of the look-ahead are requested without a table lookup
	std::vector<uint32_t> htab((size_t)no * 32 * 2, 0);
	for (int to = 0; to < no; to++) {
		int cnt = 0, r0 = 16, c0 = 8;
		for (int lane = 0; lane < 128; lane++) {
			const uint32_t *e = ptab.data() + ((size_t)to * 128 + lane) * 4;
			const int ka = (int)(e[0] & 0xFF), kb = (int)((e[0] >> 16) & 0xFF);
			if ((ka < 64) != (kb < 64)) return;
			if (ka >= 64) continue;
			r0 = std::min(r0, lane >> 3); c0 = std::min(c0, lane & 7);
			cnt++;
		}
		if (cnt != 32 || r0 > 8 || c0 > 4) return;
		for (int lane = 0; lane < 128; lane++) {
			const uint32_t *e = ptab.data() + ((size_t)to * 128 + lane) * 4;
			if ((int)(e[0] & 0xFF) >= 64) continue;
			const int r = (lane >> 3) - r0, c = (lane & 7) - c0;
			if (r < 0 || r >= 8 || c < 0 || c >= 4) return;  // not an 8 x 4 rectangle of block pairs
			htab[((size_t)to * 32 + r * 4 + c) * 2] = e[0];
			htab[((size_t)to * 32 + r * 4 + c) * 2 + 1] = (uint32_t)((lane >> 3) * 4 * width + (lane & 7) * 8);
		}
		t.tiles.qorg[to] = (uint32_t)(r0 * 4 * width + c0 * 8);
	}
	if (hipMalloc(&t.d_ptab, ptab.size() * 4) != hipSuccess) return;
	if (hipMalloc(&t.d_htab, htab.size() * 4) != hipSuccess) return;
	if (hipMemcpy(t.d_htab, htab.data(), htab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return;
	if (hipMalloc(&t.d_otab, otab.size() * 4) != hipSuccess) return;
	if (hipMalloc(&t.d_ttab, ttab.size() * 4) != hipSuccess) return;
	if (hipMemcpy(t.d_ptab, ptab.data(), ptab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return;
	if (hipMemcpy(t.d_otab, otab.data(), otab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return;
	if (hipMemcpy(t.d_ttab, ttab.data(), ttab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return;
	t.stream = true;
}

// decode_kernel's block path (block size 16): is every aligned run of 16 traversal positions of a tile an aligned 4x4 square
// of the raster, visited in one of at most DEC_BLK_ORDERS orders?  If so a block is four raster rows of four pixels, and its
// placement is the tile origin plus two table entries.  The words, in the order decode_kernel stages them (dec_block_words):
//   n_orient * 256   per pattern and block: raster offset dy * width + dx of its top-left pixel inside the tile | order << 16
//   DEC_BLK_ORDERS * 2   per order: the traversal step that visits cell dy * 4 + dx, a nibble each, low word first
//   DEC_BLK_ORDERS * 8   per order: the raster offset dy * width + dx of traversal step t, 16 bits each
// A shape that fails the test keeps dec_blocks false and decodes through the traversal table; that is a property of the
// shape.  A device error while the tables are put in place is returned (and nothing is left allocated): get_tables fails
// with it, so a shape never takes the slower path for the life of the context because of one.
hipError_t build_block_tables(const std::vector<std::vector<uint16_t>> &raws, int width, ShapeTables &t)
{
	t.dec_blocks = false;
	if (width > 1024) return hipSuccess;  // 16-bit offsets inside a tile
	const size_t no = raws.size();
	std::vector<uint32_t> words(dec_block_words((int)no), 0);
	std::vector<uint64_t> orders;  // cell of step t, a nibble each
	for (size_t o = 0; o < no; o++)
		for (int b = 0; b < 256; b++) {
			const uint16_t *k = raws[o].data() + b * 16;
			int y0 = 64, x0 = 64;
			for (int i = 0; i < 16; i++) { y0 = std::min(y0, k[i] >> 6); x0 = std::min(x0, k[i] & 63); }
			if (y0 % 4 != 0 || x0 % 4 != 0) return hipSuccess;
			uint64_t fwd = 0;
			uint32_t seen = 0;
			for (int i = 0; i < 16; i++) {
				const int dy = (k[i] >> 6) - y0, dx = (k[i] & 63) - x0;
				if (dy >= 4 || dx >= 4) return hipSuccess;  // not an aligned 4x4 square
				seen |= 1u << (dy * 4 + dx);
				fwd |= (uint64_t)(dy * 4 + dx) << (4 * i);
			}
			if (seen != 0xFFFFu) return hipSuccess;
			size_t which = 0;
			while (which < orders.size() && orders[which] != fwd) which++;
			if (which == orders.size()) {
				if (which == DEC_BLK_ORDERS) return hipSuccess;
				orders.push_back(fwd);
			}
			words[o * 256 + b] = (uint32_t)(y0 * width + x0) | ((uint32_t)which << 16);
		}
	uint32_t *inv = words.data() + no * 256, *off = inv + DEC_BLK_ORDERS * 2;
	for (size_t q = 0; q < orders.size(); q++)
		for (int i = 0; i < 16; i++) {
			const uint32_t cell = (uint32_t)(orders[q] >> (4 * i)) & 15u;
			inv[q * 2 + (cell >> 3)] |= (uint32_t)i << (4 * (cell & 7u));
			off[q * 8 + (i >> 1)] |= ((cell >> 2) * (uint32_t)width + (cell & 3u)) << (16 * (i & 1));
		}
	hipError_t e = hipMalloc(&t.d_blk, words.size() * 4);
	if (e != hipSuccess) { t.d_blk = nullptr; return e; }
	e = hipMemcpy(t.d_blk, words.data(), words.size() * 4, hipMemcpyHostToDevice);
	if (e != hipSuccess) { (void)hipFree(t.d_blk); t.d_blk = nullptr; return e; }
	t.dec_blocks = true;
	return hipSuccess;
}

// Does the traversal decompose into aligned 64x64 tiles (4096 consecutive positions each)?  If so
// build what encode_tiles_kernel needs: per tile its origin and which pattern it follows, and per
// distinct pattern the LDS byte offset (row-XOR-swizzled raster image) of every position.
// raws: per pattern dy * 64 + dx of every position of a tile, for build_block_tables
void build_tile_tables(const std::vector<int32_t> &O, int width, ShapeTables &t, std::vector<std::vector<uint16_t>> &raws)
{
	t.tiled = false;
	const size_t N = O.size();
	if (N == 0 || N % 8192 != 0 || width % 8 != 0) return;
	const int nt = (int)(N / 4096);
	if (nt > TILE_MAX_TILES) return;
	std::vector<uint32_t> org(nt);
	std::vector<uint8_t> orient(nt);
	std::vector<std::vector<uint16_t>> pats;
	std::vector<uint16_t> cur(4096), raw(4096);
	for (int ti = 0; ti < nt; ti++) {
		const int32_t *k = O.data() + (size_t)ti * 4096;
		int32_t lo = k[0];
		for (int i = 1; i < 4096; i++) lo = std::min(lo, k[i]);
		if ((lo % width) % 8 != 0) return;
		for (int i = 0; i < 4096; i++) {
			const int32_t d = k[i] - lo;
			const int dy = d / width, dx = d % width;
			if (dx >= 64 || dy >= 64) return;  // not an aligned 64x64 square
			cur[i] = (uint16_t)(dy * 128 + (((dx >> 3) ^ (dy & 7)) << 4) + (dx & 7) * 2);
			raw[i] = (uint16_t)(dy * 64 + dx);
		}
		int which = -1;
		for (size_t p = 0; p < pats.size(); p++)
			if (pats[p] == cur) { which = (int)p; break; }
		if (which < 0) {
			if ((int)pats.size() == TILE_MAX_ORIENT) return;
			pats.push_back(cur);
			raws.push_back(raw);
			which = (int)pats.size() - 1;
		}
		org[ti] = (uint32_t)lo;
		orient[ti] = (uint8_t)which;
	}
	std::vector<uint16_t> flat;
	for (auto &p : pats) flat.insert(flat.end(), p.begin(), p.end());
	if (hipMalloc(&t.d_org, nt * sizeof(uint32_t)) != hipSuccess) return;
	if (hipMalloc(&t.d_orient, nt) != hipSuccess) return;
	if (hipMalloc(&t.d_pat, flat.size() * sizeof(uint16_t)) != hipSuccess) return;
	if (hipMemcpy(t.d_org, org.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return;
	if (hipMemcpy(t.d_orient, orient.data(), nt, hipMemcpyHostToDevice) != hipSuccess) return;
	if (hipMemcpy(t.d_pat, flat.data(), flat.size() * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess) return;
	t.n_tiles = nt;
	t.n_orient = (int)pats.size();
	t.tiled = true;
	build_stream_tables(O, width, org, orient, t);
}

int get_tables(int width, int height, const ShapeTables **out)
{
	const auto key = std::make_pair(width, height);
	{
		std::lock_guard<std::mutex> lkl(g_mu_lut);
		auto it = g_ctx.luts.find(key);
		if (it != g_ctx.luts.end()) { *out = &it->second; return CCT_OK; }
	}
	// a new shape: the traversal is generated on the host with no lock held; the device allocations and the synchronous
	// copies of the tables run with nothing else of the library in flight (host.h), and g_mu_lut is taken INSIDE the
	// exclusive section (the other order would invert against a thread that holds g_mu_lut and asks for the section)
	const size_t N = (size_t)width * height;
	std::vector<int32_t> host(N ? N : 1);
	if (!gilbert_table(width, height, host.data())) return fail(CCT_E_SHAPE, "traversal generation failed for %dx%d", width, height);
	host.resize(N);
	return exclusive_section([&]() -> int {
		std::lock_guard<std::mutex> lkl(g_mu_lut);
		auto it = g_ctx.luts.find(key);
		if (it != g_ctx.luts.end()) { *out = &it->second; return CCT_OK; }  // another thread built it meanwhile
		ShapeTables t;
		HIP_TRY(hipMalloc(&t.d_lut, (N ? N : 1) * sizeof(int32_t)));
		HIP_TRY(hipMemcpy(t.d_lut, host.data(), N * sizeof(int32_t), hipMemcpyHostToDevice));
		std::vector<std::vector<uint16_t>> raws;
		build_tile_tables(host, width, t, raws);
		if (t.tiled) HIP_TRY(build_block_tables(raws, width, t));
		auto ins = g_ctx.luts.emplace(key, t);
		*out = &ins.first->second;
		return CCT_OK;
	});
}

int get_lut(int width, int height, const int32_t **out)
{
	const ShapeTables *t;
	int rc = get_tables(width, height, &t);
	if (rc) return rc;
	*out = t->d_lut;
	return CCT_OK;
}

bool bs_ok(int bs) { return bs >= 3 && bs <= 64; }

int check_shape(int n, int width, int height, int bs)
{
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	if (width <= 0 || height <= 0 || width > 65535 || height > 65535)
		return fail(CCT_E_ARG, "shape %dx%d outside the 16-bit header fields", width, height);
	if (!bs_ok(bs)) return fail(CCT_E_ARG, "block_size %d not supported by the HIP path (3 to 64)", bs);
	const int64_t N = (int64_t)width * height;
	if (N % bs != 0) return fail(CCT_E_SHAPE, "cannot reshape array of size %lld into blocks of %d", (long long)N, bs);
	if (N >= (int64_t)1 << 30) return fail(CCT_E_ARG, "slices of 2^30 pixels or more are not supported");
	return CCT_OK;
}

// Persistent host thread team: fn(i) for i in [0, n).  Spawning 256 threads per call costs more than the
// INFLATE work they do, so workers are kept (and re-created in a forked child, where they do not exist).
class HostTeam {
public:
	template <class F>
	void run(int n, int threads, F fn)
	{
		if (n <= 0) return;
		const int nt = std::max(1, std::min(threads, n));
		if (nt == 1) { for (int i = 0; i < n; i++) fn(i); return; }
		std::unique_lock<std::mutex> lk(m_);
		if (pid_ != getpid()) {  // forked child: the parent's workers are not here
			nworkers_ = 0;
			pid_ = getpid();
		}
		while (nworkers_ < nt - 1) { std::thread([this] { loop(); }).detach(); nworkers_++; }  // daemon workers
		job_ = [&fn](int i) { fn(i); };
		n_ = n; next_.store(0); pending_ = std::min(nt - 1, nworkers_); want_ = pending_; gen_++;
		cv_.notify_all();
		lk.unlock();
		for (int i; (i = next_.fetch_add(1)) < n;) fn(i);  // the caller works too
		lk.lock();
		done_.wait(lk, [this] { return pending_ == 0; });
		job_ = nullptr;
	}
private:
	void loop()
	{
		uint64_t seen = 0;
		std::unique_lock<std::mutex> lk(m_);
		for (;;) {
			cv_.wait(lk, [&] { return gen_ != seen && want_ > 0; });
			seen = gen_;
			want_--;
			auto job = job_;
			const int n = n_;
			lk.unlock();
			for (int i; (i = next_.fetch_add(1)) < n;) job(i);
			lk.lock();
			if (--pending_ == 0) done_.notify_all();
		}
	}
	std::mutex m_;
	std::condition_variable cv_, done_;
	int nworkers_ = 0;
	std::function<void(int)> job_;
	std::atomic<int> next_{0};
	int n_ = 0, pending_ = 0, want_ = 0;
	uint64_t gen_ = 0;
	pid_t pid_ = getpid();
};
// never destroyed: detached workers may still wait on the condition variables at process exit
HostTeam &g_team_enc = *new HostTeam, &g_team_dec = *new HostTeam;  // encode- and decode-side host phases may overlap

template <class F>
void parallel_for(int n, int threads, F fn, HostTeam &team = g_team_enc)
{
	team.run(n, threads, fn);
}

int encode_payload_locked(EncSlot &E, hipStream_t st, const uint16_t *d_images, int n, int width, int height, int bs, uint32_t flags,
                          int eof, uint8_t *d_payload, size_t stride, uint32_t *d_sizes, uint32_t *d_status,
                          cct_slice_stats *d_stats, uint8_t *d_roles)
{
	const int N = width * height, NB = N / bs;
	if (stride < cct_payload_stride(width, height, bs)) return fail(CCT_E_CAP, "payload stride %zu too small", stride);
	if (n == 0) return CCT_OK;
	EncArgs a{};
	a.images = d_images;
	a.lut = nullptr;
	if (flags & CCT_FLAG_FRACTAL) { int rc = get_lut(width, height, &a.lut); if (rc) return rc; }
	a.N = N; a.NB = NB; a.eof = eof; a.flags = flags;
	a.payload = d_payload; a.stride = stride; a.sizes = d_sizes; a.status = d_status;
	a.stats = reinterpret_cast<uint32_t *>(d_stats); a.roles_out = d_roles;
	a.dbg_skip = (uint32_t)g_ctx.dbg_skip;
	bool role_in_lds = true;
	(void)enc_lds_bytes(NB, &role_in_lds);
	const size_t per = (size_t)n * NB;
	int rc;
	if (!role_in_lds) { if ((rc = E.e_role.ensure(per))) return rc; a.ws_role = (uint8_t *)E.e_role.p; }
	if ((rc = E.e_lidx.ensure(per * 4))) return rc;
	if ((rc = E.e_lmask.ensure(per * 8))) return rc;
	if ((rc = E.e_lcur.ensure(per))) return rc;
	a.ws_lidx = (uint32_t *)E.e_lidx.p; a.ws_lmask = (uint64_t *)E.e_lmask.p; a.ws_lcur = (uint8_t *)E.e_lcur.p;
	const ShapeTables *tb = nullptr;
	if ((flags & CCT_FLAG_FRACTAL) && bs == 16 && g_ctx.use_tiles && !g_ctx.runtime_bs) { if ((rc = get_tables(width, height, &tb))) return rc; }
	// Choice among the tile paths (option "tile_path"): 1 = default: the streaming kernel (encode_stream.hip) wherever it
	// applies; 4 forces it, 2 the one-workgroup-per-slice tile kernel of round 1, 0 the generic table-gather kernel.
	const bool stream_ok = tb && tb->tiled && tb->stream && NB <= STREAM_MAX_NB && !g_ctx.dbg_skip;
	const int tpg = g_ctx.stream_tpg;
	const int gps = tb ? (tb->n_tiles + tpg - 1) / tpg : 0;
	if (stream_ok && (g_ctx.use_tiles == 1 || g_ctx.use_tiles == 4)) {
		if ((rc = E.e_pairrec.ensure((size_t)n * (NB / 2) * STREAM_PAIR_REC))) return rc;
		if ((rc = E.e_hand.ensure(stream_ws_bytes(n, gps)))) return rc;
		StreamArgs sa{};
		sa.e = a;
		sa.tiles = tb->tiles; sa.ptab = tb->d_ptab; sa.htab = tb->d_htab; sa.otab = tb->d_otab; sa.ttab = tb->d_ttab;
		sa.n_tiles = tb->n_tiles; sa.row_pitch = width; sa.gps = gps; sa.tpg = tpg;
		{ static const int dbg = tuning_env("CCT_STREAM_DBG", 0); sa.dbg = dbg; }
		sa.hand = (uint64_t *)E.e_hand.p; sa.ticket = (uint32_t *)(sa.hand + (size_t)n * gps * 4);
		sa.spill_mask = (uint64_t *)E.e_lmask.p; sa.spill_idx = (uint16_t *)E.e_lidx.p; sa.pairrec = (uint8_t *)E.e_pairrec.p;
		g_ctx.last_path = 3;
		// two memsets and one kernel: launched plainly.  Replayed as a graph the three nodes took 0.20 ms in the bench against 0.15
		// (profiles/r03_graph_ab.log): a graph pays between its nodes what it saves on the host, and there is nothing to save here
		HIP_TRY(launch_encode_stream(sa, n, st));
		return CCT_OK;
	}
	if (tb && tb->tiled) {
		bool tile_role_in_lds = true;
		(void)enc_tiles_lds_bytes(NB, &tile_role_in_lds);
		if (!tile_role_in_lds) { if ((rc = E.e_role.ensure(per))) return rc; a.ws_role = (uint8_t *)E.e_role.p; }
		else a.ws_role = nullptr;
		TileEncArgs ta{};
		ta.e = a;
		ta.tile_org = tb->d_org; ta.tile_orient = tb->d_orient; ta.patterns = tb->d_pat;
		ta.n_orient = tb->n_orient; ta.n_tiles = tb->n_tiles; ta.row_pitch = width;
		HIP_TRY(launch_encode_tiles(ta, n, st));
		g_ctx.last_path = 2;
		return CCT_OK;
	}
	const bool run_time = bs_run_time(bs, g_ctx.runtime_bs != 0);
	HIP_TRY(launch_encode(a, n, bs, g_ctx.wg_threads, st, run_time));
	g_ctx.last_path = run_time ? 4 : 0;
	return CCT_OK;
}

// Payload bytes one DEFLATE pass takes (its workspaces, deflate_workspace.h, need 44 bytes per payload byte: 47 GB at this bound, of 288).  2^28
// in round 1; at 1024x1024 that made passes of 127 slices, and the kernels that give a slice one workgroup (both sort
// passes, the run list, the block walk) left half of the 256 CUs idle.
constexpr size_t DEFLATE_PASS_BYTES = (size_t)1 << 30;

// DEFLATE (zlib stream of `level`, `strategy` and `mem_level`: 4 .. 9 with strategies 0, 1, 4, 1 .. 9 with 2, 3; memLevel 8 or 9)
// of n device-resident byte strings on the device; output slice i = 13 header bytes + zlib stream at d_out + i*out_stride
// (E.z_out), sizes in E.z_outsizes.
int deflate_locked(EncSlot &E, const uint8_t *d_in, size_t in_stride, const uint32_t *d_in_sizes, int n, const uint8_t header13[13],
                   size_t out_stride, int level, int strategy, int mem_level = 8)
{
	if (in_stride % 256 != 0 || out_stride % 4 != 0) return fail(CCT_E_ARG, "deflate strides must be multiples of 256 / 4");
	DeflateArgs a{};
	if (!deflate_strategy_args(level, strategy, a))
		return fail(CCT_E_ARG, "zlib level %d with strategy %d is not on the device", level, strategy);
	if (!deflate_mem_level_args(mem_level, a)) return fail(CCT_E_ARG, "zlib memLevel %d: 8 and 9 are on the device", mem_level);
	const size_t EB = (size_t)n * in_stride;
	if (EB >= ((size_t)1 << 32)) return fail(CCT_E_ARG, "deflate batch of %zu bytes exceeds the 4 GiB sort limit; split the batch", EB);
	// the regions this pass needs, each a buffer that grows on its own (deflate_workspace.h: why they are not one arena); a short
	// pass (Z_HUFFMAN_ONLY / Z_RLE) neither grows nor clears the workspaces of the hash chains
	const DflShape shape = dfl_shape(n, in_stride, a.block_syms);
	int rc;
	void *base[DFL_REGIONS];
	for (int r = 0; r < DFL_REGIONS; r++) {
		if (dfl_region_needed(r, strategy) && (rc = E.z_ws[r].ensure(dfl_region_bytes(r, shape)))) return rc;
		base[r] = E.z_ws[r].p;
	}
	if ((rc = E.z_out.ensure((size_t)n * out_stride))) return rc;
	if ((rc = E.z_outsizes.ensure((size_t)n * 4))) return rc;
	// (cutting the batch into slice ranges that run concurrently on streams of their own was tried and removed: the
	// cross-stream dependencies cost more than the overlap returned, here as in the transform+pack stage)
	const bool use_fork = g_ctx.deflate_fork != 0;
	if (use_fork && !E.stream_side) {
		// created on first use (see GPU_MAX_HW_QUEUES in ensure_ctx: streams are not free)
		const int crc = exclusive_section([&]() -> int { HIP_TRY(hipStreamCreateWithFlags(&E.stream_side, hipStreamNonBlocking)); return CCT_OK; });
		if (crc) return crc;
	}
	a.in = d_in; a.in_stride = in_stride; a.in_sizes = d_in_sizes;
	dfl_bind(a, base, shape);
	a.tree_waves = (uint32_t)g_ctx.tree_waves;  // 0: launch_tree and the kernel choose (part of the graph key below)
	// compact sort records hold a 15-bit hash: memLevel 8 only (deflate_kernels.hip "Sort records").  A compact record for the
	// 16-bit hash would need a 20-bit position field.  memLevel 9 serves the PNG writer, and on filtered PNG rows compact records
	// do not pay even at memLevel 8 (61.7 against 61.0 ms per 256 slices at level 6)
	a.pos_mask = (g_ctx.compact_recs && mem_level == 8 && in_stride < ((size_t)1 << 22)) ? (1u << 22) - 1u : 0xFFFFFFFFu;
	// the tag of a pass must not meet a record of 16383 passes ago: clear records and counter well before it comes round (and
	// whenever the buffer is new); a pass that failed on the way may have left the two counts a few apart, hence the margin
	// (a short pass neither reads match records nor advances the tag: it does not count)
	const DevBuf &mr = E.z_ws[DFL_R_MATCH];
	if (dfl_uses_chains(strategy)) {
		if (E.z_mr_cleared != mr.p || E.z_mr_cleared_cap != mr.cap || E.z_gen_passes >= 16000u) {
			HIP_TRY(hipMemsetAsync(mr.p, 0, mr.cap, E.stream));
			HIP_TRY(hipMemsetAsync(E.z_ws[DFL_R_GEN].p, 0, 256, E.stream));
			E.z_mr_cleared = mr.p; E.z_mr_cleared_cap = mr.cap; E.z_gen_passes = 0;
		}
		E.z_gen_passes++;
	}
	a.out = (uint8_t *)E.z_out.p; a.out_stride = out_stride; a.out_sizes = (uint32_t *)E.z_outsizes.p;
	memcpy(a.header13, header13, 13);
	if (g_ctx.use_graph) {
		// whole batch on the main stream, as a graph keyed by everything the launches depend on
		std::vector<uint8_t> key(sizeof(DeflateArgs) + 2 * sizeof(int));
		memcpy(key.data(), &a, sizeof(DeflateArgs));
		memcpy(key.data() + sizeof(DeflateArgs), &n, sizeof(int));
		const int fork_key = use_fork ? 1 : 0;
		memcpy(key.data() + sizeof(DeflateArgs) + sizeof(int), &fork_key, sizeof(int));
		EncSlot::ZGraph *zg = nullptr;
		for (auto &g : E.z_graphs) if (g.key == key) zg = &g;
		if (!zg) {
			const int crc = exclusive_section([&]() -> int {  // nothing else of the library runs during a capture (host.h)
				if (E.z_graphs.size() >= 4) {  // forget the least recently used argument set
					size_t old = 0;
					for (size_t i = 1; i < E.z_graphs.size(); i++) if (E.z_graphs[i].last_use < E.z_graphs[old].last_use) old = i;
					if (E.z_graphs[old].exec) (void)hipGraphExecDestroy(E.z_graphs[old].exec);
					if (E.z_graphs[old].graph) (void)hipGraphDestroy(E.z_graphs[old].graph);
					E.z_graphs.erase(E.z_graphs.begin() + (long)old);
				}
				EncSlot::ZGraph g;
				HIP_TRY(hipStreamBeginCapture(E.stream, hipStreamCaptureModeThreadLocal));
				hipError_t le = launch_deflate(a, n, E.stream, use_fork ? E.stream_side : nullptr, E.ev_fork);
				hipError_t ce = hipStreamEndCapture(E.stream, &g.graph);
				if (le != hipSuccess) { if (g.graph) (void)hipGraphDestroy(g.graph); return fail(CCT_E_DEVICE, "DEFLATE capture: %s", hipGetErrorString(le)); }
				HIP_TRY(ce);
				const hipError_t ie = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
				if (ie != hipSuccess) { (void)hipGraphDestroy(g.graph); return fail(CCT_E_DEVICE, "hipGraphInstantiate failed: %s", hipGetErrorString(ie)); }
				g.key = key;
				E.z_graphs.push_back(std::move(g));
				return CCT_OK;
			});
			if (crc) return crc;
			zg = &E.z_graphs.back();
		}
		zg->last_use = ++E.z_clock;
		HIP_TRY(hipGraphLaunch(zg->exec, E.stream));
		return CCT_OK;
	}
	HIP_TRY(launch_deflate(a, n, E.stream, use_fork ? E.stream_side : nullptr, E.ev_fork));
	return CCT_OK;
}

int decode_payload_locked(DecSlot &D, const uint8_t *d_payload, size_t stride, const uint32_t *d_sizes, int n, int width,
                          int height, int bs, int fractal, uint16_t *d_images, uint32_t *d_status, hipStream_t st)
{
	const int N = width * height, NB = N / bs;
	if (stride % 16 != 0) return fail(CCT_E_ARG, "payload stride must be a multiple of 16");
	if (n == 0) return CCT_OK;
	DecArgs a{};
	a.payload = d_payload; a.stride = stride; a.sizes = d_sizes;
	a.lut = nullptr;
	a.n_tiles = 0; a.n_orient = 0; a.width = width;
	if (fractal) {
		const ShapeTables *tb;
		int rc0 = get_tables(width, height, &tb);
		if (rc0) return rc0;
		a.lut = tb->d_lut;
		if (tb->tiled && tb->dec_blocks && g_ctx.use_tiles && !g_ctx.runtime_bs) {
			a.tile_org = tb->d_org; a.tile_orient = tb->d_orient; a.blk_tab = tb->d_blk;
			a.n_tiles = tb->n_tiles; a.n_orient = tb->n_orient;
		}
	}
	a.N = N; a.NB = NB; a.images = d_images; a.status = d_status;
	a.narrow_stores = ((uintptr_t)d_images & 7u) != 0;  // a slice is a multiple of 8 bytes: every slice starts as the first does
	const size_t per = (size_t)n * NB, jper = (size_t)n * ((size_t)NB / 2 + 1);
	int rc;
	if ((rc = D.d_role.ensure(per))) return rc;
	if ((rc = D.d_slot.ensure(per * 4))) return rc;
	if ((rc = D.d_jord.ensure(jper * 4))) return rc;
	if ((rc = D.d_jval.ensure(jper))) return rc;
	a.ws_role = (uint8_t *)D.d_role.p; a.ws_slot = (uint32_t *)D.d_slot.p;
	a.ws_jord = (uint32_t *)D.d_jord.p; a.ws_jval = (uint8_t *)D.d_jval.p;
	a.pcache_steps = (int)(stride / ((size_t)g_ctx.wg_threads * DEC_SEG) + 2);
	if ((rc = D.d_pcache.ensure((size_t)n * a.pcache_steps * g_ctx.wg_threads * sizeof(uint2)))) return rc;
	a.ws_pcache = (uint2 *)D.d_pcache.p;
	const bool run_time = bs_run_time(bs, g_ctx.runtime_bs != 0);
	bool block_path = false;
	HIP_TRY(launch_decode(a, n, bs, g_ctx.wg_threads, st, run_time, &block_path));
	g_ctx.last_dec_path = run_time ? 1 : 0;
	g_ctx.last_dec_block_path = block_path ? 1 : 0;
	if (st != D.stream) {
		// the kernel is still queued on the caller's stream when the slot is released: whatever takes the slot next runs on
		// D.stream and must not touch d_role / d_slot / d_jord / d_pcache before this launch is through
		HIP_TRY(hipEventRecord(D.ev_ws, st));
		HIP_TRY(hipStreamWaitEvent(D.stream, D.ev_ws, 0));
	}
	return CCT_OK;
}

}  // namespace
}  // namespace cct

using namespace cct;

extern "C" {

int cct_version(void) { return CCT_ABI_VERSION; }
const char *cct_last_error(void) { return g_err; }

int cct_init(int device)
{
	std::lock_guard<std::mutex> lk(g_mu);
	return ensure_ctx(device);
}

int cct_shutdown(void)
{
	std::lock_guard<std::mutex> lk(g_mu);
	std::lock_guard<std::mutex> lk1(g_mu1);
	std::lock_guard<std::mutex> lkd0(g_mu_dec[0]);
	std::lock_guard<std::mutex> lkd1(g_mu_dec[1]);
	if (!g_ctx.ready || g_ctx.pid != getpid()) { reset_ctx(); return CCT_OK; }
	(void)hipSetDevice(g_ctx.device);
	(void)hipStreamSynchronize(g_ctx.stream);
	(void)hipStreamSynchronize(g_ctx.stream_dec);
	for (int k = 0; k < N_ENC_SLOTS; k++) {
		EncSlot &E = g_enc[k];
		if (E.stream) (void)hipStreamSynchronize(E.stream);
		if (E.stream_copy) (void)hipStreamSynchronize(E.stream_copy);
		for (auto &g : E.z_graphs) { if (g.exec) (void)hipGraphExecDestroy(g.exec); if (g.graph) (void)hipGraphDestroy(g.graph); }
		for (int i = 0; i < E.n_bufs; i++) E.all_bufs[i]->release();
		for (HandoffSet &S : E.sets) S.release();
		for (hipEvent_t e : E.ev_fork) if (e) (void)hipEventDestroy(e);
		E.ev_zlib.release();
		if (E.stream_copy) (void)hipStreamDestroy(E.stream_copy);
		if (E.stream_side) { (void)hipStreamSynchronize(E.stream_side); (void)hipStreamDestroy(E.stream_side); }
		if (k > 0 && E.stream) (void)hipStreamDestroy(E.stream);
	}
	comm_release();
	dicom_rle_release();
	jpegll_release();
	jpegls_release();
	j2k_release();
	tiff_release();
	if (g_gate) { (void)hipFree(g_gate); g_gate = nullptr; }
	for (auto &kv : g_ctx.luts) {
		ShapeTables &t = kv.second;
		void *ptrs[] = {t.d_lut, t.d_org, t.d_orient, t.d_pat, t.d_blk, t.d_ptab, t.d_otab, t.d_ttab, t.d_htab};
		for (void *p : ptrs) if (p) (void)hipFree(p);
	}
	for (int k = 0; k < N_DEC_SLOTS; k++) {
		DecSlot &D = g_dec[k];
		if (D.stream) (void)hipStreamSynchronize(D.stream);
		D.release();
		if (k > 0 && D.stream) (void)hipStreamDestroy(D.stream);
	}
	(void)hipStreamDestroy(g_ctx.stream);
	(void)hipStreamDestroy(g_ctx.stream_dec);
	reset_ctx();
	return CCT_OK;
}

int cct_device_info(char *name, size_t name_cap, int *compute_units, uint64_t *hbm_bytes)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, g_ctx.device));
	if (name && name_cap) {
		// the runtime of this image leaves hipDeviceProp_t::name empty for the MI355X: ask hipDeviceGetName, then fall back
		char dn[256] = "";
		if (prop.name[0]) snprintf(dn, sizeof dn, "%s", prop.name);
		else if (hipDeviceGetName(dn, (int)sizeof dn, g_ctx.device) != hipSuccess || !dn[0]) {
			(void)hipGetLastError();
			snprintf(dn, sizeof dn, "gfx950 device, %d CUs", prop.multiProcessorCount);
		}
		snprintf(name, name_cap, "%s (%s)", dn, prop.gcnArchName);
	}
	if (compute_units) *compute_units = prop.multiProcessorCount;
	if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
	return CCT_OK;
}

int cct_dev_alloc(void **d_ptr, size_t bytes)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	return exclusive_section([&]() -> int { HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 1)); return CCT_OK; });
}
int cct_dev_free(void *d_ptr)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	return exclusive_section([&]() -> int {  // hipFree waits for the whole device: not next to a capture (host.h)
		HIP_TRY(hipStreamSynchronize(g_ctx.stream));
		HIP_TRY(hipFree(d_ptr));
		return CCT_OK;
	});
}
int cct_host_alloc(void **h_ptr, size_t bytes)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	return exclusive_section([&]() -> int { HIP_TRY(hipHostMalloc(h_ptr, bytes ? bytes : 1, hipHostMallocDefault)); return CCT_OK; });
}
int cct_host_free(void *h_ptr)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	return exclusive_section([&]() -> int {
		HIP_TRY(hipStreamSynchronize(g_ctx.stream));
		HIP_TRY(hipHostFree(h_ptr));
		return CCT_OK;
	});
}
// is [p, p + bytes) page-locked host memory (cct_host_alloc / hipHostMalloc / hipHostRegister)?
static bool is_pinned_host(const void *p, size_t bytes)
{
	hipPointerAttribute_t at{};
	if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
	if (at.type != hipMemoryTypeHost) return false;
	hipPointerAttribute_t at2{};
	if (bytes > 1 && hipPointerGetAttributes(&at2, (const uint8_t *)p + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return false; }
	return bytes <= 1 || at2.type == hipMemoryTypeHost;
}
int cct_h2d(void *d_dst, const void *h_src, size_t bytes)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, g_ctx.stream));
	HIP_TRY(hipStreamSynchronize(g_ctx.stream));
	return CCT_OK;
}
int cct_d2h(void *h_dst, const void *d_src, size_t bytes)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, g_ctx.stream));
	HIP_TRY(hipStreamSynchronize(g_ctx.stream));
	return CCT_OK;
}
int cct_dev_memset(void *d_dst, int value, size_t bytes)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	HIP_TRY(hipMemsetAsync(d_dst, value, bytes, g_ctx.stream));
	HIP_TRY(hipStreamSynchronize(g_ctx.stream));  // complete on return: decode calls run on their own stream
	return CCT_OK;
}
int cct_sync(void)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(g_ctx.stream));
	for (int k = 1; k < N_ENC_SLOTS; k++) {  // an encode batch call is complete when it returns; this is for symmetry only
		std::lock_guard<std::mutex> lk1(*g_enc[k].mu);
		HIP_TRY(hipStreamSynchronize(g_enc[k].stream));
	}
	return CCT_OK;
}

int cct_event_create(void **ev)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	hipEvent_t e;
	HIP_TRY(hipEventCreate(&e));
	*ev = (void *)e;
	return CCT_OK;
}
int cct_event_record(void *ev)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	HIP_TRY(hipEventRecord((hipEvent_t)ev, g_ctx.stream));
	return CCT_OK;
}
int cct_event_elapsed_ms(void *ev_start, void *ev_stop, float *ms)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	HIP_TRY(hipEventSynchronize((hipEvent_t)ev_stop));
	HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)ev_start, (hipEvent_t)ev_stop));
	return CCT_OK;
}
int cct_event_destroy(void *ev)
{
	std::lock_guard<std::mutex> lk(g_mu);
	int rc = ensure_ctx();
	if (rc) return rc;
	HIP_TRY(hipEventDestroy((hipEvent_t)ev));
	return CCT_OK;
}

int cct_curve_table(int width, int height, int32_t *h_out)
{
	if (width <= 0 || height <= 0 || !h_out) return fail(CCT_E_ARG, "bad curve arguments");
	return gilbert_table(width, height, h_out) ? CCT_OK : fail(CCT_E_SHAPE, "traversal generation failed");
}

size_t cct_payload_stride(int width, int height, int block_size)
{
	if (width <= 0 || height <= 0 || block_size <= 0) return 0;
	const size_t N = (size_t)width * height, NB = N / block_size;
	// every pixel a 2-byte token, one jump byte per pair of blocks, EOF, flush padding
	const size_t need = 2 * N + NB / 2 + 1 + 16;
	return (need + 255) & ~(size_t)255;
}

size_t cct_file_bound(int width, int height, int block_size)
{
	const size_t p = cct_payload_stride(width, height, block_size);
	return deflate_out_stride(p, 8);  // .cct files are memLevel 8 streams
}

int cct_encode_payload_dev(const uint16_t *d_images, int n, int width, int height, int block_size, uint32_t flags,
                           int eof_byte, uint8_t *d_payload, size_t payload_stride, uint32_t *d_payload_sizes,
                           uint32_t *d_status, cct_slice_stats *d_stats, uint8_t *d_roles)
{
	std::lock_guard<std::mutex> lk(g_mu);
	ApiCall in_call;
	int rc = check_shape(n, width, height, block_size);
	if (rc) return rc;
	if ((rc = ensure_ctx())) return rc;
	return encode_payload_locked(g_enc[0], g_ctx.stream, d_images, n, width, height, block_size,
	                             flags & ~(CCT_FLAG_LEVEL_MASK | CCT_FLAG_STRATEGY_MASK), eof_byte, d_payload, payload_stride,
	                             d_payload_sizes, d_status, d_stats, d_roles);
}

// ---- pieces of cct_encode_batch / cct_encode_batch_packed -------------------------------------------------------------

// take a free encode slot (see EncSlot): the first caller gets slot 0, one that arrives while it is busy slot 1
static EncSlot &acquire_encode_slot(std::unique_lock<std::mutex> &lk)
{
	std::mutex *const slot_mu[N_ENC_SLOTS] = {&g_mu, &g_mu1};
	const int nslots = std::max(1, std::min(g_ctx.enc_slots, N_ENC_SLOTS));
	for (;;) {
		for (int k = 0; k < nslots; k++) {
			std::unique_lock<std::mutex> t(*slot_mu[k], std::try_to_lock);
			if (t.owns_lock()) { lk = std::move(t); return g_enc[k]; }
		}
		std::this_thread::sleep_for(std::chrono::microseconds(50));
	}
}

// CCT_FLAG_DEFLATE_STRATEGY field -> zlib strategy 0 .. 4 (a clear field is Z_DEFAULT_STRATEGY); -1 for a refused field
static int flags_deflate_strategy(uint32_t flags)
{
	const int f = (int)((flags & CCT_FLAG_STRATEGY_MASK) >> 12);
	return f <= 4 ? f : -1;
}

// CCT_FLAG_DEFLATE_LEVEL field -> zlib level (a clear field is level 9, what the reference writes); -1 for a refused field.
// Levels 1 .. 3 are deflate_fast, except under Z_HUFFMAN_ONLY / Z_RLE, which ignore the level's function
static int flags_deflate_level(uint32_t flags, int strategy)
{
	const int f = (int)((flags & CCT_FLAG_LEVEL_MASK) >> 8);
	const int lo = (strategy == 2 || strategy == 3) ? 1 : 4;
	return f == 0 ? 9 : (f >= lo && f <= 9) ? f : -1;
}

// core.py:193-210 (big-endian fields, values masked to a byte / 16 bits)
static void make_header13(uint8_t hdr13[13], const char magic[4], int width, int height, int channels, int bytes_per_channel,
                          uint32_t flags)
{
	hdr13[0] = (uint8_t)magic[0]; hdr13[1] = (uint8_t)magic[1]; hdr13[2] = (uint8_t)magic[2]; hdr13[3] = (uint8_t)magic[3];
	hdr13[4] = (uint8_t)((width >> 8) & 0xFF); hdr13[5] = (uint8_t)(width & 0xFF);
	hdr13[6] = (uint8_t)((height >> 8) & 0xFF); hdr13[7] = (uint8_t)(height & 0xFF);
	hdr13[8] = (uint8_t)(channels & 0xFF); hdr13[9] = (uint8_t)(bytes_per_channel & 0xFF);
	hdr13[10] = (flags & CCT_FLAG_FRACTAL) ? 1 : 0;
	hdr13[11] = (flags & CCT_FLAG_SEGMENTATION) ? 1 : 0;
	hdr13[12] = (flags & CCT_FLAG_DEFLATE) ? 1 : 0;
}

// One DEFLATE pass worth of files (nc of them, sizes osz[], in E.z_out at stride zstride) on their way to the caller.
struct FilesOut {
	EncSlot &E;
	int nc;
	const uint32_t *osz;     // file sizes (host)
	size_t zstride;
	size_t exact;            // sum of the sizes
	std::vector<size_t> offs;  // 16-byte aligned offsets of the files in a strided-pack buffer
};

// archive layout, page-locked destination, first half: pack the files of a pass into the packed buffer of a hand-off set the
// call owns (offsets computed on the device from the sizes, so this can be queued right behind the DEFLATE pass, before the
// host knows the sizes -- the pack used to start a launch latency after the host had read them); `cap` = what the buffer must hold
static int pack_enqueue(EncSlot &E, HandoffSet &S, int nc, size_t zstride, size_t cap)
{
	int rc;
	if (!E.stream_copy) {
		const int crc = exclusive_section([&]() -> int {
			HIP_TRY(hipStreamCreateWithFlags(&E.stream_copy, hipStreamNonBlocking));
			for (HandoffSet &s : E.sets) {
				HIP_TRY(hipEventCreateWithFlags(&s.ev_packed, hipEventDisableTiming));
				HIP_TRY(hipEventCreateWithFlags(&s.ev_copied, hipEventDisableTiming));
				HIP_TRY(hipEventRecord(s.ev_copied, E.stream_copy));
			}
			return CCT_OK;
		});
		if (crc) return crc;
	}
	if (S.packed.cap < cap) HIP_TRY(hipEventSynchronize(S.ev_copied));  // about to be reallocated
	if ((rc = S.packed.ensure(cap))) return rc;
	if ((rc = E.z_packoffs.ensure((size_t)(nc + 1) * 8))) return rc;
	HIP_TRY(hipStreamWaitEvent(E.stream, S.ev_copied, 0));  // the copy out of this buffer by the set's owner before
	HIP_TRY(launch_pack((const uint8_t *)E.z_out.p, zstride, (const uint32_t *)E.z_outsizes.p, nc,
	                    (uint64_t *)E.z_packoffs.p, (uint8_t *)S.packed.p, 1, E.stream));
	HIP_TRY(hipEventRecord(S.ev_packed, E.stream));
	return CCT_OK;
}

// second half: the packed files to the copy stream.  The caller gives the slot back before it waits for S.ev_copied -- the
// next batch's kernels start while these files travel
static int packed_to_pinned_archive_async(EncSlot &E, HandoffSet &S, size_t exact, uint8_t *h_dst)
{
	HIP_TRY(hipStreamWaitEvent(E.stream_copy, S.ev_packed, 0));
	HIP_TRY(hipMemcpyAsync(h_dst, S.packed.p, exact, hipMemcpyDeviceToHost, E.stream_copy));
	HIP_TRY(hipEventRecord(S.ev_copied, E.stream_copy));
	return CCT_OK;
}

// archive layout, any destination: exact pack on the device, one copy (through the pinned stage unless the destination is
// page-locked itself, then a threaded memcpy)
static int files_to_archive(FilesOut &f, uint8_t *h_dst, double *t_copied)
{
	EncSlot &E = f.E;
	int rc;
	const size_t cap = f.offs[f.nc] + 16;
	if ((rc = E.z_packed.ensure(cap))) return rc;
	HIP_TRY(launch_pack((const uint8_t *)E.z_out.p, f.zstride, (const uint32_t *)E.z_outsizes.p, f.nc,
	                    (uint64_t *)E.z_packoffs.p, (uint8_t *)E.z_packed.p, 1, E.stream));
	if (is_pinned_host(h_dst, f.exact)) {
		HIP_TRY(hipMemcpyAsync(h_dst, E.z_packed.p, f.exact, hipMemcpyDeviceToHost, E.stream));
		HIP_TRY(hipStreamSynchronize(E.stream));
		*t_copied = now_ms();
		return CCT_OK;
	}
	if ((rc = E.h_stage.ensure(cap))) return rc;
	HIP_TRY(hipMemcpyAsync(E.h_stage.p, E.z_packed.p, f.exact, hipMemcpyDeviceToHost, E.stream));
	HIP_TRY(hipStreamSynchronize(E.stream));
	*t_copied = now_ms();
	const int nt = std::min(g_ctx.zlib_threads, 16);
	const size_t per = (f.exact + nt - 1) / nt;
	const uint8_t *stg = (const uint8_t *)E.h_stage.p;
	const size_t exact = f.exact;
	parallel_for(nt, nt, [&](int t) {
		const size_t lo = (size_t)t * per, hi = std::min(exact, lo + per);
		if (lo < hi) memcpy(h_dst + lo, stg + lo, hi - lo);
	});
	return CCT_OK;
}

// strided layout (file i at h_out + i * out_stride): 16-byte aligned pack on the device, one copy into the pinned stage,
// threaded scatter
static int files_to_strided(FilesOut &f, uint8_t *h_first, size_t out_stride)
{
	EncSlot &E = f.E;
	int rc;
	const size_t packed_cap = f.offs[f.nc];
	if ((rc = E.z_packed.ensure(packed_cap + 16))) return rc;
	if ((rc = E.h_stage.ensure(packed_cap + 16))) return rc;
	HIP_TRY(launch_pack((const uint8_t *)E.z_out.p, f.zstride, (const uint32_t *)E.z_outsizes.p, f.nc,
	                    (uint64_t *)E.z_packoffs.p, (uint8_t *)E.z_packed.p, 0, E.stream));
	HIP_TRY(hipMemcpyAsync(E.h_stage.p, E.z_packed.p, packed_cap, hipMemcpyDeviceToHost, E.stream));
	HIP_TRY(hipStreamSynchronize(E.stream));
	const uint8_t *stg = (const uint8_t *)E.h_stage.p;
	const uint32_t *osz = f.osz;
	const std::vector<size_t> &offs = f.offs;
	parallel_for(f.nc, std::min(g_ctx.zlib_threads, 32), [&](int i) { memcpy(h_first + (size_t)i * out_stride, stg + offs[i], osz[i]); });
	return CCT_OK;
}

// DEFLATE (or none) on the host thread team: payloads come back, libz at `level` per slice (9: core.py:340), header in front
static int files_on_host(EncSlot &E, int n, size_t stride, const std::vector<uint32_t> &psz, const uint8_t hdr13[13], bool defl,
                         int level, int strategy, uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes)
{
	const double t_copy0 = now_ms();
	uint8_t *stage = (uint8_t *)E.h_stage.p;
	for (int i = 0; i < n; i++)  // bring back only the bytes each slice produced (none has overflowed its stride: the caller has looked)
		HIP_TRY(hipMemcpyAsync(stage + (size_t)i * stride, (uint8_t *)E.e_payload.p + (size_t)i * stride, psz[i],
		                       hipMemcpyDeviceToHost, E.stream));
	HIP_TRY(hipStreamSynchronize(E.stream));
	const double t_defl0 = now_ms();
	tl_d2h_ms = (float)(t_defl0 - t_copy0);
	std::atomic<int> zerr(0);
	parallel_for(n, defl ? g_ctx.zlib_threads : 1, [&](int i) {
		uint8_t *o = h_out + (size_t)i * out_stride;
		memcpy(o, hdr13, 13);
		const uint8_t *pl = stage + (size_t)i * stride;
		if (defl && strategy != Z_DEFAULT_STRATEGY) {  // zlib.compressobj(level, DEFLATED, 15, 8, strategy)
			z_stream zs{};
			int zr = deflateInit2(&zs, level, Z_DEFLATED, 15, 8, strategy);
			if (zr != Z_OK) { zerr.store(zr); h_out_sizes[i] = 0; return; }
			zs.next_in = const_cast<Bytef *>(pl); zs.avail_in = psz[i];
			zs.next_out = o + 13; zs.avail_out = (uInt)(out_stride - 13);
			zr = deflate(&zs, Z_FINISH);
			const uLong dl = zs.total_out;
			(void)deflateEnd(&zs);
			if (zr != Z_STREAM_END) { zerr.store(zr == Z_OK ? Z_BUF_ERROR : zr); h_out_sizes[i] = 0; return; }
			h_out_sizes[i] = 13 + (uint32_t)dl;
		} else if (defl) {  // zlib.compress(data, level), core.py:340 with level 9
			uLongf dl = (uLongf)(out_stride - 13);
			const int zr = compress2(o + 13, &dl, pl, psz[i], level);
			if (zr != Z_OK) { zerr.store(zr); h_out_sizes[i] = 0; return; }
			h_out_sizes[i] = 13 + (uint32_t)dl;
		} else {
			memcpy(o + 13, pl, psz[i]);
			h_out_sizes[i] = 13 + psz[i];
		}
	});
	tl_deflate_ms = (float)(now_ms() - t_defl0);
	if (zerr.load()) return fail(CCT_E_ZLIB, "compress2 failed (%d)", zerr.load());
	return CCT_OK;
}

// CCT_FLAG_DEFLATE_LEVEL / _STRATEGY fields of an encode call -> zlib level and strategy; the fields leave `flags` (the payload
// stage and the .cct header do not depend on them)
static int take_deflate_fields(uint32_t &flags, int *level, int *strategy)
{
	*strategy = flags_deflate_strategy(flags);
	if (*strategy < 0)
		return fail(CCT_E_ARG, "deflate strategy field %u: zlib strategies are 0 .. 4", (flags & CCT_FLAG_STRATEGY_MASK) >> 12);
	*level = flags_deflate_level(flags, *strategy);
	if (*level < 0) {
		if (*strategy == 2 || *strategy == 3)
			return fail(CCT_E_ARG, "deflate level field %u with strategy %d: levels 1 .. 9 only",
			            (flags & CCT_FLAG_LEVEL_MASK) >> 8, *strategy);
		return fail(CCT_E_ARG, "deflate level field %u with strategy %d: levels 4 .. 9 only (1 .. 3 are deflate_fast: not on the device)",
		            (flags & CCT_FLAG_LEVEL_MASK) >> 8, *strategy);
	}
	flags &= ~(CCT_FLAG_LEVEL_MASK | CCT_FLAG_STRATEGY_MASK);
	return CCT_OK;
}

static int encode_batch_impl(const uint16_t *images, int images_on_device, int n, int width, int height, int block_size,
                             uint32_t flags, int eof_byte, const char magic[4], int channels, int bytes_per_channel,
                             uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes, uint32_t *h_status,
                             uint32_t *h_payload_sizes, cct_slice_stats *h_stats, uint64_t *h_packed_offsets)
{
	// h_packed_offsets != NULL: archive layout -- files back to back in h_out (capacity out_stride bytes in
	// total), h_packed_offsets[n+1]; needs the device DEFLATE path (or deflate off)
	const bool packed = h_packed_offsets != nullptr;
	const double t_call0 = now_ms();
	EncodeInFlight in_flight;  // decode calls that start meanwhile pick the INFLATE geometry that shares the device best
	int level, strategy, rc;
	if ((rc = take_deflate_fields(flags, &level, &strategy))) return rc;

	// ---- checks, context, slot, hand-off set ----
	if ((rc = check_shape(n, width, height, block_size))) return rc;
	if (!(g_ctx.ready && g_ctx.pid == getpid())) {  // first use in this process: bind the device
		std::lock_guard<std::mutex> lk0(g_mu);
		if ((rc = ensure_ctx())) return rc;
	}
	std::unique_lock<std::mutex> lk;
	EncSlot &E = acquire_encode_slot(lk);
	HandoffRing &ring = g_handoff[&E - g_enc];
	HandoffOwner own(ring);  // waits for the call two before this one; released where this call stops using the set, at the latest on return
	HandoffSet &S = E.sets[own.set()];
	ApiCall in_call;  // after the slot and the set: a thread waiting for either must not keep exclusive sections of the others waiting
	const double t_lock0 = now_ms();
	if ((rc = ensure_ctx())) return rc;
	if (n == 0) return CCT_OK;
	const size_t N = (size_t)width * height;
	const size_t stride = cct_payload_stride(width, height, block_size);
	const size_t zstride = cct_file_bound(width, height, block_size);
	const bool defl = (flags & CCT_FLAG_DEFLATE) != 0;
	if (!packed && out_stride < (defl ? zstride : 13 + stride)) return fail(CCT_E_CAP, "out_stride %zu too small", out_stride);
	if (packed && !(defl && g_ctx.device_deflate))
		return fail(CCT_E_ARG, "packed output needs deflate_compression with the device DEFLATE path");
	// With DEFLATE on the device and the whole batch in one pass the host does not need sizes or status before
	// the DEFLATE kernels are queued (they read the sizes on the device; a payload cannot outgrow its stride):
	// one host synchronisation less per batch.
	const bool one_pass = defl && g_ctx.device_deflate && (size_t)n * stride <= DEFLATE_PASS_BYTES;

	// ---- transform+pack stage enqueued: uploads, workspaces, the kernels between their events, sizes / status / statistics back ----
	const uint16_t *d_img = images;
	if (!images_on_device) {
		if ((rc = E.e_images.ensure((size_t)n * N * 2))) return rc;
		HIP_TRY(hipMemcpyAsync(E.e_images.p, images, (size_t)n * N * 2, hipMemcpyHostToDevice, E.stream));
		d_img = (const uint16_t *)E.e_images.p;
	}
	if ((rc = E.e_payload.ensure((size_t)n * stride))) return rc;
	if ((rc = E.e_sizes.ensure((size_t)n * 4))) return rc;
	if ((rc = E.e_status.ensure((size_t)n * 4))) return rc;
	if ((rc = E.h_stage.ensure((size_t)n * stride))) return rc;
	if ((rc = E.e_stats.ensure((size_t)n * sizeof(cct_slice_stats)))) return rc;
	// Queue ahead: possible when the whole call can be queued without the host knowing a size, into an archive that is
	// page-locked over every byte the call can write.  Everything this call needs from the slot is in the stream then, so
	// the slot goes to the next call BEFORE the host waits for the sizes: that call's kernels are queued behind this one's
	// while they run, and the device no longer idles for a launch latency between one batch's pack and the next batch's
	// first kernel and again before its DEFLATE graph (0.2 ms of a 4.2 ms step, profiles/r03_bench_timeline.log).  From
	// the hand-over on the call touches its hand-off set and the copy stream only.
	const bool qa = packed && one_pass && g_ctx.queue_ahead && is_pinned_host(h_out, std::min(out_stride, (size_t)n * zstride));
	std::vector<uint32_t> psz(n);
	uint32_t *l_psz = psz.data(), *l_status = h_status, *l_osz = nullptr;  // where the device's words land: with queue ahead in pinned memory
	cct_slice_stats *l_stats = h_stats;
	if (qa) {
		if ((rc = S.landing.ensure((size_t)n * (12 + sizeof(cct_slice_stats))))) return rc;
		l_psz = (uint32_t *)S.landing.p; l_status = l_psz + n; l_osz = l_status + n;
		l_stats = (cct_slice_stats *)(l_osz + n);
	}
	// (running this stage on a stream of the highest priority while the other slot is in its DEFLATE pass was tried: the
	// kernels took as long as without, waves already resident are not displaced)
	if ((rc = S.stage.begin(E.stream))) return rc;
	rc = encode_payload_locked(E, E.stream, d_img, n, width, height, block_size, flags, eof_byte, (uint8_t *)E.e_payload.p, stride,
	                           (uint32_t *)E.e_sizes.p, (uint32_t *)E.e_status.p,
	                           h_stats ? (cct_slice_stats *)E.e_stats.p : nullptr, nullptr);
	if (rc) return rc;
	if ((rc = S.stage.end(E.stream))) return rc;
	HIP_TRY(launch_gate_bump(g_gate, E.stream));  // decode kernels waiting for this stage to be over may go (cct_decode_batch)
	if (h_stats) HIP_TRY(hipMemcpyAsync(l_stats, E.e_stats.p, (size_t)n * sizeof(cct_slice_stats), hipMemcpyDeviceToHost, E.stream));
	StreamDrain drain(E.stream);  // until the first synchronisation below
	HIP_TRY(hipMemcpyAsync(l_psz, E.e_sizes.p, (size_t)n * 4, hipMemcpyDeviceToHost, E.stream));
	HIP_TRY(hipMemcpyAsync(l_status, E.e_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, E.stream));
	tl_enc_kernel_ms = 0;
	if (!one_pass) {
		HIP_TRY(hipStreamSynchronize(E.stream));
		drain.disarm();
		if ((rc = S.stage.add_ms(tl_enc_kernel_ms))) return rc;
		for (int i = 0; i < n; i++)
			if (h_status[i] & CCT_ST_CAP) return fail(CCT_E_CAP, "slice %d overflowed its payload stride", i);
	}
	uint8_t hdr13[13];
	make_header13(hdr13, magic, width, height, channels, bytes_per_channel, flags);

	// ---- DEFLATE (or none) on the host thread team ----
	if (!(defl && g_ctx.device_deflate)) {
		rc = files_on_host(E, n, stride, psz, hdr13, defl, level, strategy, h_out, out_stride, h_out_sizes);
		if (h_payload_sizes) memcpy(h_payload_sizes, psz.data(), (size_t)n * 4);
		return rc;
	}

	// ---- DEFLATE on the device: zlib.compress(data, level) (core.py:340, level 9) restated in deflate_kernels.hip ----
	// bounded workspaces: at most DEFLATE_PASS_BYTES of payload per pass, in passes of equal size (several DEFLATE
	// kernels give a slice one workgroup: a short last pass would leave most of the chip idle)
	const int chunk_max = (int)std::max<size_t>(1, DEFLATE_PASS_BYTES / stride);
	const int n_passes = (n + chunk_max - 1) / chunk_max;
	const int chunk = (n + n_passes - 1) / n_passes;
	tl_deflate_ms = 0; tl_d2h_ms = 0;
	std::optional<StreamDrain> copies;  // on the copy stream, from the first copy into the caller's archive on: an error return must not leave one in flight
	for (int c0 = 0, pass = 0; c0 < n; c0 += chunk, pass++) {
		const int nc = std::min(chunk, n - c0);
		const bool last = c0 + nc >= n;
		uint32_t *osz = h_out_sizes + c0;
		// the pass enqueued, with queue ahead the pack as well (the common pipelined case)
		if ((rc = S.pass.begin(E.stream))) return rc;
		rc = deflate_locked(E, (const uint8_t *)E.e_payload.p + (size_t)c0 * stride, stride,
		                    (const uint32_t *)E.e_sizes.p + c0, nc, hdr13, zstride, level, strategy);
		if (rc) return rc;
		if ((rc = S.pass.end(E.stream))) return rc;
		HIP_TRY(launch_gate_bump(g_gate + 1, E.stream));
		g_gate_passes_issued.fetch_add(1, std::memory_order_relaxed);  // (only once the bump is in the stream: a count that is ahead of the device for good makes every later gate wait run to its timeout)
		if (qa && (rc = pack_enqueue(E, S, nc, zstride, (size_t)nc * zstride + 16))) return rc;
		HIP_TRY(hipMemcpyAsync(qa ? l_osz : osz, E.z_outsizes.p, (size_t)nc * 4, hipMemcpyDeviceToHost, E.stream));
		// handed on, or synchronised
		if (qa) {
			HIP_TRY(hipEventRecord(S.landed, E.stream));
			lk.unlock();
			HIP_TRY(hipEventSynchronize(S.landed));
			memcpy(psz.data(), l_psz, (size_t)n * 4); memcpy(h_status, l_status, (size_t)n * 4); memcpy(osz, l_osz, (size_t)nc * 4);
			if (h_stats) memcpy(h_stats, l_stats, (size_t)n * sizeof(cct_slice_stats));
		} else HIP_TRY(hipStreamSynchronize(E.stream));
		drain.disarm();  // nothing queued targets this frame any more (later chunks copy into caller memory and synchronise at once)
		float t_dev_deflate_ms = 0;
		if ((rc = S.pass.add_ms(t_dev_deflate_ms))) return rc;
		if (one_pass) {
			if ((rc = S.stage.add_ms(tl_enc_kernel_ms))) return rc;
			for (int i = 0; i < n; i++)
				if (h_status[i] & CCT_ST_CAP) return fail(CCT_E_CAP, "slice %d overflowed its payload stride", i);
		}
		tl_deflate_ms += t_dev_deflate_ms;
		// delivered: strided, into a page-locked archive, or into any archive
		const double t_c0 = now_ms();
		FilesOut f{E, nc, osz, zstride, 0, std::vector<size_t>(nc + 1, 0)};
		for (int i = 0; i < nc; i++) { f.exact += osz[i]; f.offs[i + 1] = f.offs[i] + (((size_t)osz[i] + 15) & ~(size_t)15); }
		if (!qa && (rc = E.z_packoffs.ensure((size_t)(nc + 1) * 8))) return rc;
		if (!packed) {
			if ((rc = files_to_strided(f, h_out + (size_t)c0 * out_stride, out_stride))) return rc;
			tl_d2h_ms += (float)(now_ms() - t_c0);
			continue;
		}
		if (c0 == 0) h_packed_offsets[0] = 0;
		const uint64_t at = h_packed_offsets[c0];
		if (at + f.exact > out_stride) return fail(CCT_E_CAP, "packed output needs %zu bytes", (size_t)(at + f.exact));
		for (int i = 0; i < nc; i++) h_packed_offsets[c0 + i + 1] = h_packed_offsets[c0 + i] + osz[i];
		if (!is_pinned_host(h_out + at, f.exact) && !qa) {  // (queue ahead has checked the whole archive)
			double t_c1 = t_c0;
			if ((rc = files_to_archive(f, h_out + at, &t_c1))) return rc;
			tl_d2h_ms += (float)(now_ms() - t_c0);
			if (trace_on())
				fprintf(stderr, "[cct] encode n=%d: deflate %.2f ms, pack+d2h %.2f ms, host scatter %.2f ms (%zu bytes)\n", nc,
				        t_dev_deflate_ms, t_c1 - t_c0, now_ms() - t_c1, f.exact);
			continue;
		}
		// page-locked archive: the files of this pass leave on the copy stream while the next pass (or, after the last one,
		// the next batch) already runs its kernels.  A call of several passes keeps the slot and alternates the two packed
		// buffers: every second pass borrows the other set's, waiting for a call queued ahead of this one that still owns it.
		std::optional<HandoffOwner> borrowed;
		if (pass & 1) borrowed.emplace(ring, own.set() ^ 1u);
		HandoffSet &P = E.sets[own.set() ^ (pass & 1u)];
		if (!qa && (rc = pack_enqueue(E, P, nc, zstride, f.offs[nc] + 16))) return rc;  // (the pack kernel works in 16-byte units)
		if (!copies) copies.emplace(E.stream_copy);
		if ((rc = packed_to_pinned_archive_async(E, P, f.exact, h_out + at))) return rc;
		// the copy out of the buffer is queued, durations and landing words are read: the call after next may have the set
		if (borrowed) borrowed->release(); else if (last) own.release();
		tl_d2h_ms += (float)(now_ms() - t_c0);
		if (!last) continue;
		if (h_payload_sizes) memcpy(h_payload_sizes, psz.data(), (size_t)n * 4);
		const double t_unlock = now_ms();
		if (lk.owns_lock()) lk.unlock();  // the slot is free for the next batch; only the copy stream still works for this one
		HIP_TRY(hipEventSynchronize(P.ev_copied));
		copies->disarm();
		if (trace_on())
			fprintf(stderr, "[cct] encode n=%d: waited for a slot %.2f ms, held it %.2f ms (kernel %.2f, deflate %.2f), tail %.2f ms, t=%.2f\n", nc,
			        t_lock0 - t_call0, t_unlock - t_lock0, tl_enc_kernel_ms, t_dev_deflate_ms, now_ms() - t_unlock, t_lock0);
		tl_d2h_ms += (float)(now_ms() - t_c0);  // (no lock: a float for cct_last_timings)
		return CCT_OK;
	}
	if (h_payload_sizes) memcpy(h_payload_sizes, psz.data(), (size_t)n * 4);
	return CCT_OK;
}

int cct_encode_batch(const uint16_t *images, int images_on_device, int n, int width, int height, int block_size,
                     uint32_t flags, int eof_byte, const char magic[4], int channels, int bytes_per_channel,
                     uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes, uint32_t *h_status,
                     uint32_t *h_payload_sizes, cct_slice_stats *h_stats)
{
	return encode_batch_impl(images, images_on_device, n, width, height, block_size, flags, eof_byte, magic, channels,
	                         bytes_per_channel, h_out, out_stride, h_out_sizes, h_status, h_payload_sizes, h_stats, nullptr);
}

int cct_encode_batch_packed(const uint16_t *images, int images_on_device, int n, int width, int height, int block_size,
                            uint32_t flags, int eof_byte, const char magic[4], int channels, int bytes_per_channel,
                            uint8_t *h_archive, size_t archive_cap, uint64_t *h_offsets, uint32_t *h_out_sizes,
                            uint32_t *h_status, uint32_t *h_payload_sizes, cct_slice_stats *h_stats)
{
	if (!h_offsets) return fail(CCT_E_ARG, "h_offsets is required");
	return encode_batch_impl(images, images_on_device, n, width, height, block_size, flags, eof_byte, magic, channels,
	                         bytes_per_channel, h_archive, archive_cap, h_out_sizes, h_status, h_payload_sizes, h_stats, h_offsets);
}

static int zlib_compress_batch_impl(const uint8_t *h_in, const uint64_t *h_offsets, int n, int level, int strategy, int mem_level,
                                    uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes)
{
	std::lock_guard<std::mutex> lk(g_mu);
	ApiCall in_call;
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	int rc = ensure_ctx();
	if (rc) return rc;
	if (n == 0) return CCT_OK;
	EncSlot &E = g_enc[0];
	size_t longest = 0;
	for (int i = 0; i < n; i++) longest = std::max(longest, (size_t)(h_offsets[i + 1] - h_offsets[i]));
	const size_t in_stride = deflate_in_stride(longest), zstride = deflate_out_stride(in_stride, mem_level);
	if (out_stride < zstride - 13) return fail(CCT_E_CAP, "out_stride %zu too small (need %zu)", out_stride, zstride - 13);
	if ((rc = E.z_in.ensure((size_t)n * in_stride))) return rc;
	if ((rc = E.z_insizes.ensure((size_t)n * 4))) return rc;
	std::vector<uint32_t> isz(n), osz(n);
	StreamDrain drain(E.stream);
	HIP_TRY(hipMemsetAsync(E.z_in.p, 0, (size_t)n * in_stride, E.stream));
	for (int i = 0; i < n; i++) {
		isz[i] = (uint32_t)(h_offsets[i + 1] - h_offsets[i]);
		if (isz[i])
			HIP_TRY(hipMemcpyAsync((uint8_t *)E.z_in.p + (size_t)i * in_stride, h_in + h_offsets[i], isz[i],
			                       hipMemcpyHostToDevice, E.stream));
	}
	HIP_TRY(hipMemcpyAsync(E.z_insizes.p, isz.data(), (size_t)n * 4, hipMemcpyHostToDevice, E.stream));
	uint8_t hdr13[13] = {0};
	if ((rc = E.ev_zlib.begin(E.stream))) return rc;  // the DEFLATE pass alone, for cct_last_timings
	rc = deflate_locked(E, (const uint8_t *)E.z_in.p, in_stride, (const uint32_t *)E.z_insizes.p, n, hdr13, zstride, level, strategy,
	                    mem_level);
	if (rc) return rc;
	if ((rc = E.ev_zlib.end(E.stream))) return rc;
	HIP_TRY(hipMemcpyAsync(osz.data(), E.z_outsizes.p, (size_t)n * 4, hipMemcpyDeviceToHost, E.stream));
	HIP_TRY(hipStreamSynchronize(E.stream));
	float ms = 0;
	if ((rc = E.ev_zlib.add_ms(ms))) return rc;
	tl_deflate_ms = ms;
	for (int i = 0; i < n; i++) h_out_sizes[i] = osz[i] - 13;
	return files_to_host(h_out, out_stride, h_out_sizes, n, E.z_out.p, zstride, 13, zstride - 13, "stream", 0, "bound", E.stream);
}

int cct_zlib_compress_batch(const uint8_t *h_in, const uint64_t *h_offsets, int n, uint8_t *h_out, size_t out_stride,
                            uint32_t *h_out_sizes)
{
	return zlib_compress_batch_impl(h_in, h_offsets, n, 9, Z_DEFAULT_STRATEGY, 8, h_out, out_stride, h_out_sizes);
}

int cct_zlib_compress_batch_level(const uint8_t *h_in, const uint64_t *h_offsets, int n, int level, uint8_t *h_out,
                                  size_t out_stride, uint32_t *h_out_sizes)
{
	if (level == -1) level = 6;  // Z_DEFAULT_COMPRESSION
	if (level >= 0 && level <= 3) return fail(CCT_E_ARG, "zlib level %d: deflate_stored / deflate_fast: not on the device", level);
	if (level < 4 || level > 9) return fail(CCT_E_ARG, "zlib level %d: levels are -1 and 4 .. 9", level);
	return zlib_compress_batch_impl(h_in, h_offsets, n, level, Z_DEFAULT_STRATEGY, 8, h_out, out_stride, h_out_sizes);
}

int cct_zlib_compress_batch_strategy(const uint8_t *h_in, const uint64_t *h_offsets, int n, int level, int strategy,
                                     uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes)
{
	return cct_zlib_compress_batch_params(h_in, h_offsets, n, level, strategy, 8, h_out, out_stride, h_out_sizes);
}

int cct_zlib_compress_batch_params(const uint8_t *h_in, const uint64_t *h_offsets, int n, int level, int strategy, int mem_level,
                                   uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes)
{
	if (mem_level != 8 && mem_level != 9) return fail(CCT_E_ARG, "zlib memLevel %d: 8 and 9 are on the device", mem_level);
	if (strategy < Z_DEFAULT_STRATEGY || strategy > Z_FIXED)
		return fail(CCT_E_ARG, "zlib strategy %d: strategies are 0 .. 4 (Z_DEFAULT_STRATEGY .. Z_FIXED)", strategy);
	if (level == -1) level = 6;  // Z_DEFAULT_COMPRESSION
	if (level == 0) return fail(CCT_E_ARG, "zlib level 0 with strategy %d: deflate_stored: not on the device", strategy);
	if (level < 0 || level > 9) return fail(CCT_E_ARG, "zlib level %d with strategy %d: levels are -1 and 1 .. 9", level, strategy);
	if (strategy != Z_HUFFMAN_ONLY && strategy != Z_RLE && level <= 3)
		return fail(CCT_E_ARG, "zlib level %d with strategy %d: deflate_fast: not on the device (levels -1 and 4 .. 9)", level, strategy);
	return zlib_compress_batch_impl(h_in, h_offsets, n, level, strategy, mem_level, h_out, out_stride, h_out_sizes);
}

// ---- PNG writer (png_kernels.hip) ---------------------------------------------------------------
// Pillow's PNG stream: zlib.compressobj(level, DEFLATED, 15, memLevel 9, Z_FILTERED) (ZipEncode.c); IDAT chunks of the
// bufsize of ImageFile._save, max(65536, 4 * cols) bytes.  One DEFLATE pass takes at most DEFLATE_PASS_BYTES of filtered rows.
constexpr int PNG_MEM_LEVEL = 9;
constexpr size_t PNG_MAX_FILTERED = DEFLATE_PASS_BYTES - 512;
// bps: bytes per sample, 2 in the 16-bit files and 1 in the 8-bit ones
static size_t png_filtered_bytes(int rows, int cols, int bps = 2) { return (size_t)rows * (1 + (size_t)bps * (size_t)cols); }
static size_t png_in_stride(size_t filtered) { return deflate_in_stride(filtered); }
static size_t png_zstride(size_t in_stride) { return deflate_out_stride(in_stride, PNG_MEM_LEVEL); }
static uint32_t png_chunk(int cols) { return (uint32_t)std::max<size_t>(65536, 4 * (size_t)cols); }
// signature + IHDR (33), the stream, 12 bytes per IDAT chunk, IEND (12)
static size_t png_file_bytes(size_t zlen, uint32_t chunk) { return 33 + zlen + 12 * ((zlen + chunk - 1) / chunk) + 12; }

// every term grows with the filtered bytes, so the bound of the 16-bit file covers the 8-bit file of the same shape
static size_t png_bound_of(size_t filtered, int cols)
{
	return (png_file_bytes(png_zstride(png_in_stride(filtered)) - 13, png_chunk(cols)) + 63) & ~(size_t)63;
}

size_t cct_png_bound(int rows, int cols)
{
	if (rows < 1 || cols < 1 || png_filtered_bytes(rows, cols) > PNG_MAX_FILTERED) return 0;
	return png_bound_of(png_filtered_bytes(rows, cols), cols);
}

// What the two writers differ in: the file's bit depth, the source rasters' bytes per pixel and the arguments of the filter kernel.
struct PngFormat {
	int depth;            // 16: png_filter_kernel with `shift`; 8: png_filter8_kernel with src_bits and the window
	int shift;
	int src_bits, lo, hi;
};

static int png_encode_impl(const void *images, int images_on_device, int n, int rows, int cols, const PngFormat &fmt, int level,
                           uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes);

int cct_png_encode_batch(const uint16_t *images, int images_on_device, int n, int rows, int cols, int shift, int level,
                         uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes)
{
	if (level == -1) level = 6;  // Pillow's compress_level default (Z_DEFAULT_COMPRESSION)
	if (level >= 0 && level <= 3) return fail(CCT_E_ARG, "PNG compress_level %d: deflate_stored / deflate_fast: not on the device", level);
	if (level < 4 || level > 9) return fail(CCT_E_ARG, "PNG compress_level %d: levels are -1 and 4 .. 9", level);
	if (shift < 0 || shift > 15) return fail(CCT_E_ARG, "PNG sample shift %d: 0 .. 15", shift);
	if (rows < 1 || cols < 1) return fail(CCT_E_ARG, "PNG shape %d x %d: rows and cols must be >= 1", rows, cols);
	if (png_filtered_bytes(rows, cols) > PNG_MAX_FILTERED)
		return fail(CCT_E_ARG, "PNG shape %d x %d: %zu filtered bytes exceed one DEFLATE pass (%zu)", rows, cols,
		            png_filtered_bytes(rows, cols), PNG_MAX_FILTERED);
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	if (!images && n > 0) return fail(CCT_E_ARG, "images is required");
	const size_t bound = cct_png_bound(rows, cols);
	if (out_stride < bound) return fail(CCT_E_CAP, "out_stride %zu too small (need cct_png_bound = %zu)", out_stride, bound);
	const PngFormat fmt{16, shift, 16, 0, 0};
	return png_encode_impl(images, images_on_device, n, rows, cols, fmt, level, h_out, out_stride, h_out_sizes);
}

int cct_png_encode8_batch(const void *images, int images_on_device, int n, int rows, int cols, int src_bits, int lo, int hi,
                          int level, uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes)
{
	if (level == -1) level = 6;
	if (level >= 0 && level <= 3) return fail(CCT_E_ARG, "PNG compress_level %d: deflate_stored / deflate_fast: not on the device", level);
	if (level < 4 || level > 9) return fail(CCT_E_ARG, "PNG compress_level %d: levels are -1 and 4 .. 9", level);
	if (src_bits != 8 && src_bits != 16) return fail(CCT_E_ARG, "PNG source of %d bits: 8 or 16", src_bits);
	if (lo < 0 || hi > 65535 || lo >= hi) return fail(CCT_E_ARG, "PNG window (%d, %d): 0 <= lo < hi <= 65535", lo, hi);
	if (src_bits == 8 && (lo != 0 || hi != 255)) return fail(CCT_E_ARG, "PNG window (%d, %d) of an 8-bit source: (0, 255)", lo, hi);
	if (rows < 1 || cols < 1) return fail(CCT_E_ARG, "PNG shape %d x %d: rows and cols must be >= 1", rows, cols);
	if (png_filtered_bytes(rows, cols, 1) > PNG_MAX_FILTERED)
		return fail(CCT_E_ARG, "PNG shape %d x %d: %zu filtered bytes exceed one DEFLATE pass (%zu)", rows, cols,
		            png_filtered_bytes(rows, cols, 1), PNG_MAX_FILTERED);
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	if (!images && n > 0) return fail(CCT_E_ARG, "images is required");
	// a shape only the 8-bit file fits in one pass has no cct_png_bound: its own bound then
	const size_t bound16 = cct_png_bound(rows, cols), bound = bound16 ? bound16 : png_bound_of(png_filtered_bytes(rows, cols, 1), cols);
	if (out_stride < bound)
		return fail(CCT_E_CAP, "out_stride %zu too small (need %s = %zu)", out_stride, bound16 ? "cct_png_bound" : "the 8-bit bound", bound);
	const PngFormat fmt{8, 0, src_bits, lo, hi};
	return png_encode_impl(images, images_on_device, n, rows, cols, fmt, level, h_out, out_stride, h_out_sizes);
}

static int png_encode_impl(const void *images, int images_on_device, int n, int rows, int cols, const PngFormat &fmt, int level,
                           uint8_t *h_out, size_t out_stride, uint32_t *h_out_sizes)
{
	std::lock_guard<std::mutex> lk(g_mu);
	ApiCall in_call;
	int rc = ensure_ctx();
	if (rc) return rc;
	if (n == 0) return CCT_OK;
	EncSlot &E = g_enc[0];
	const size_t F = png_filtered_bytes(rows, cols, fmt.depth / 8), in_stride = png_in_stride(F), zstride = png_zstride(in_stride);
	const size_t img_bytes = (size_t)rows * cols * (size_t)(fmt.src_bits / 8);
	const uint32_t chunk = png_chunk(cols);
	const size_t pstride = png_file_bytes(zstride - 13, chunk);
	const uint32_t max_chunks = (uint32_t)((zstride - 13 + chunk - 1) / chunk);
	const int per_pass = (int)std::max<size_t>(1, DEFLATE_PASS_BYTES / in_stride);
	PngPackArgs pk{};
	pk.chunk = chunk;
	{  // IHDR: width, height, depth, color type 0 (grayscale), compression 0, filter 0, interlace 0
		uint8_t *h = pk.ihdr;
		const uint8_t fixed[8] = {0, 0, 0, 13, 'I', 'H', 'D', 'R'};
		memcpy(h, fixed, 8);
		const uint32_t w = (uint32_t)cols, ht = (uint32_t)rows;
		const uint8_t data[13] = {(uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w,
		                          (uint8_t)(ht >> 24), (uint8_t)(ht >> 16), (uint8_t)(ht >> 8), (uint8_t)ht, (uint8_t)fmt.depth, 0, 0, 0, 0};
		memcpy(h + 8, data, 13);
		const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), h + 4, 17);
		h[21] = (uint8_t)(crc >> 24); h[22] = (uint8_t)(crc >> 16); h[23] = (uint8_t)(crc >> 8); h[24] = (uint8_t)crc;
	}
	StreamDrain drain(E.stream);
	std::vector<uint32_t> sizes;
	std::vector<uint8_t> host_rows, host_z;
	for (int c0 = 0; c0 < n; c0 += per_pass) {
		const int nc = std::min(per_pass, n - c0);
		if ((rc = E.z_in.ensure((size_t)nc * in_stride))) return rc;
		if ((rc = E.z_insizes.ensure((size_t)nc * 4))) return rc;
		if ((rc = E.png_out.ensure((size_t)nc * pstride))) return rc;
		if ((rc = E.png_sizes.ensure((size_t)nc * 4))) return rc;
		const void *d_img;
		if ((rc = rasters_to_device(images, images_on_device, c0, nc, img_bytes, E.png_img, E.stream, &d_img))) return rc;
		sizes.assign((size_t)nc, (uint32_t)F);
		HIP_TRY(hipMemcpyAsync(E.z_insizes.p, sizes.data(), (size_t)nc * 4, hipMemcpyHostToDevice, E.stream));
		if (fmt.depth == 16)
			HIP_TRY(launch_png_filter((const uint16_t *)d_img, nc, rows, cols, fmt.shift, (uint8_t *)E.z_in.p, in_stride, E.stream));
		else
			HIP_TRY(launch_png_filter8(d_img, fmt.src_bits, nc, rows, cols, fmt.lo, fmt.hi, (uint8_t *)E.z_in.p, in_stride, E.stream));
		if (g_ctx.device_deflate) {
			const uint8_t hdr13[13] = {0};
			rc = deflate_locked(E, (const uint8_t *)E.z_in.p, in_stride, (const uint32_t *)E.z_insizes.p, nc, hdr13, zstride, level,
			                    Z_FILTERED, PNG_MEM_LEVEL);
			if (rc) return rc;
		} else {  // host libz: the filtered rows come back, the streams go out to the pack kernel in the device pass's layout
			if ((rc = E.z_out.ensure((size_t)nc * zstride))) return rc;
			if ((rc = E.z_outsizes.ensure((size_t)nc * 4))) return rc;
			host_rows.resize((size_t)nc * in_stride);
			host_z.resize((size_t)nc * zstride);
			HIP_TRY(hipMemcpyAsync(host_rows.data(), E.z_in.p, (size_t)nc * in_stride, hipMemcpyDeviceToHost, E.stream));
			HIP_TRY(hipStreamSynchronize(E.stream));
			std::atomic<int> zerr(0);
			parallel_for(nc, g_ctx.zlib_threads, [&](int i) {
				z_stream zs{};
				int zr = deflateInit2(&zs, level, Z_DEFLATED, 15, PNG_MEM_LEVEL, Z_FILTERED);
				if (zr != Z_OK) { zerr.store(zr); sizes[i] = 13; return; }
				zs.next_in = host_rows.data() + (size_t)i * in_stride; zs.avail_in = (uInt)F;
				zs.next_out = host_z.data() + (size_t)i * zstride + 13; zs.avail_out = (uInt)(zstride - 13);
				zr = deflate(&zs, Z_FINISH);
				sizes[i] = 13 + (uint32_t)zs.total_out;
				(void)deflateEnd(&zs);
				if (zr != Z_STREAM_END) { zerr.store(zr == Z_OK ? Z_BUF_ERROR : zr); sizes[i] = 13; }
			});
			if (zerr.load()) return fail(CCT_E_ZLIB, "deflate failed (%d)", zerr.load());
			HIP_TRY(hipMemcpyAsync(E.z_out.p, host_z.data(), (size_t)nc * zstride, hipMemcpyHostToDevice, E.stream));
			HIP_TRY(hipMemcpyAsync(E.z_outsizes.p, sizes.data(), (size_t)nc * 4, hipMemcpyHostToDevice, E.stream));
		}
		pk.src = (const uint8_t *)E.z_out.p; pk.src_stride = zstride; pk.src_skip = 13; pk.src_sizes = (const uint32_t *)E.z_outsizes.p;
		pk.out = (uint8_t *)E.png_out.p; pk.out_stride = pstride; pk.out_sizes = (uint32_t *)E.png_sizes.p;
		HIP_TRY(launch_png_pack(pk, nc, max_chunks, E.stream));
		HIP_TRY(hipMemcpyAsync(h_out_sizes + c0, E.png_sizes.p, (size_t)nc * 4, hipMemcpyDeviceToHost, E.stream));
		HIP_TRY(hipStreamSynchronize(E.stream));
		if ((rc = files_to_host(h_out + (size_t)c0 * out_stride, out_stride, h_out_sizes + c0, nc, E.png_out.p, pstride, 0, pstride, "PNG", c0,
		                        "stride", E.stream)))
			return rc;
	}
	return CCT_OK;
}

// launch_inflate's arguments: streams in `in` at the offsets of D.d_archoffs, each `skip` bytes in; the outputs are the slot's
static InflateArgs inflate_args(DecSlot &D, const DevBuf &in, size_t in_total, uint32_t skip, size_t out_stride)
{
	InflateArgs ia{};
	ia.in = (const uint8_t *)in.p; ia.in_total = in_total;
	ia.offsets = (const uint64_t *)D.d_archoffs.p; ia.skip = skip;
	ia.out = (uint8_t *)D.d_payload.p; ia.out_stride = out_stride;
	ia.out_sizes = (uint32_t *)D.d_sizes.p; ia.status = (uint32_t *)D.d_zstatus.p;
	return ia;
}

// The INFLATE kernel reads ahead of a stream's end: the last 48 bytes of the padded archive (pad + 16 bytes) are zero
static hipError_t zero_read_ahead(void *arch, size_t pad, hipStream_t st) { return hipMemsetAsync((uint8_t *)arch + (pad > 32 ? pad - 32 : 0), 0, pad > 32 ? 48 : pad + 16, st); }

}  // extern "C"

// On the first call of a process the device is bound BEFORE the slot and the shared lock are taken.  A thread must never wait
// for g_mu while it counts as a call in flight: a first encode holds g_mu through HIP initialisation and then asks
// for an exclusive section, which waits for every call in flight to leave.  Then the slot, the ApiCall, the thread's device.
int cct::lease_decode_slot(DecLease &l)
{
	if (!(g_ctx.ready && g_ctx.pid == getpid())) {
		std::lock_guard<std::mutex> lk(g_mu);
		if (int rc = ensure_ctx()) return rc;
	}
	const int nslots = std::max(1, std::min(g_ctx.dec_slots, N_DEC_SLOTS));
	for (;;) {  // wait for a free decode slot (see DecSlot)
		for (int k = 0; k < nslots && !l.lk.owns_lock(); k++) {
			l.lk = std::unique_lock<std::mutex>(g_mu_dec[k], std::try_to_lock);
			l.slot = k;
		}
		if (l.lk.owns_lock()) break;
		std::this_thread::sleep_for(std::chrono::microseconds(50));
	}
	l.in_call.emplace();
	l.stream = g_dec[l.slot].stream;
	HIP_TRY(hipSetDevice(g_ctx.device));
	return CCT_OK;
}

void cct::set_last_kernel_ms(bool encode, float ms) { (encode ? tl_enc_kernel_ms : tl_dec_kernel_ms) = ms; }

int cct::deflate_on_main(const uint8_t *d_in, size_t in_stride, const uint32_t *d_in_sizes, int n, size_t out_stride, int level,
                         const uint8_t **d_out, const uint32_t **d_out_sizes)
{
	EncSlot &E = g_enc[0];
	const uint8_t hdr13[13] = {0};
	if (int rc = deflate_locked(E, d_in, in_stride, d_in_sizes, n, hdr13, out_stride, level, Z_DEFAULT_STRATEGY, 8)) return rc;
	*d_out = (const uint8_t *)E.z_out.p;
	*d_out_sizes = (const uint32_t *)E.z_outsizes.p;
	return CCT_OK;
}

int cct::inflate_lanes_for_call() { return inflate_lanes_now(); }

extern "C" {

int cct_zlib_decompress_batch(const uint8_t *h_in, const uint64_t *h_offsets, int n, uint8_t *h_out, size_t out_stride,
                              uint32_t *h_out_sizes, uint32_t *h_status)
{
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	if (out_stride == 0 || (out_stride & 15)) return fail(CCT_E_ARG, "out_stride must be a positive multiple of 16");
	DecLease lease;
	int rc = lease_decode_slot(lease);
	if (rc || n == 0) return rc;
	DecSlot &D = g_dec[lease.slot];
	const uint64_t a0 = h_offsets[0], a1 = h_offsets[n];
	const size_t abytes = (size_t)(a1 - a0), apad = (abytes + 31) & ~(size_t)15;
	if ((rc = D.d_arch.ensure(apad + 16))) return rc;
	if ((rc = D.d_archoffs.ensure((size_t)(n + 1) * 8))) return rc;
	if ((rc = D.d_zstatus.ensure((size_t)n * 4))) return rc;
	if ((rc = D.d_sizes.ensure((size_t)n * 4))) return rc;
	if ((rc = D.d_payload.ensure((size_t)n * out_stride))) return rc;
	std::vector<uint64_t> rel(n + 1);
	std::vector<uint32_t> zst(n), osz(n);
	for (int i = 0; i <= n; i++) rel[i] = h_offsets[i] - a0;
	hipStream_t st = D.stream;
	StreamDrain drain(st);
	HIP_TRY(zero_read_ahead(D.d_arch.p, apad, st));
	if (abytes) HIP_TRY(hipMemcpyAsync(D.d_arch.p, h_in + a0, abytes, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(D.d_archoffs.p, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(launch_inflate(inflate_args(D, D.d_arch, apad, 0, out_stride), n, st, inflate_lanes_now()));
	HIP_TRY(hipMemcpyAsync(zst.data(), D.d_zstatus.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(osz.data(), D.d_sizes.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	int first = CCT_OK;
	for (int i = 0; i < n; i++) {
		h_status[i] = (zst[i] & CCT_ST_ZLIB) ? CCT_E_ZLIB : (zst[i] & CCT_ST_STREAM) ? CCT_E_CAP : CCT_OK;
		h_out_sizes[i] = h_status[i] == CCT_OK ? osz[i] : 0;
		if (h_status[i] != CCT_OK && first == CCT_OK) {
			first = (int)h_status[i];
			fail(first, "stream %d: %s", i, first == CCT_E_ZLIB ? "invalid DEFLATE stream" : "output larger than out_stride");
		}
	}
	rc = files_to_host(h_out, out_stride, h_out_sizes, n, D.d_payload.p, out_stride, 0, out_stride, "stream", 0, "stride", st);  // a refused stream has size 0
	return rc ? rc : first;
}

// ---- PNG reader (png_read_kernels.hip) ---------------------------------------------------------------
static uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// signature + IHDR of one file: CCT_OK or CCT_E_PNG (no message: the callers add the file's index)
static int png_parse_ihdr(const uint8_t *f, size_t len, int *rows, int *cols, int *depth)
{
	static const uint8_t head[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
	if (len < 33 || memcmp(f, head, 16) != 0) return CCT_E_PNG;
	const uint32_t w = be32(f + 16), h = be32(f + 20);
	const int d = f[24];
	if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) return CCT_E_PNG;
	if ((d != 8 && d != 16) || f[25] != 0 || f[26] != 0 || f[27] != 0 || f[28] != 0) return CCT_E_PNG;
	*rows = (int)h; *cols = (int)w; *depth = d;
	return CCT_OK;
}

int cct_png_info(const uint8_t *h_file, size_t len, int *rows, int *cols, int *bit_depth)
{
	if (!h_file || !rows || !cols || !bit_depth) return fail(CCT_E_ARG, "null argument");
	if (png_parse_ihdr(h_file, len, rows, cols, bit_depth))
		return fail(CCT_E_PNG, "not a PNG this reader takes (8- or 16-bit grayscale, not interlaced)");
	return CCT_OK;
}

// The chunk heads of one file -> entries of the chunk table (cct_internal.h PngChunk has the bounds argument).  `base`: the
// file's offset in the pass's upload; *zoff: the running size of the gathered streams.  Returns the file's status; a refused
// file leaves no entries behind.
static int png_walk_file(const uint8_t *f, size_t len, uint64_t base, uint32_t index, int rows, int cols, int *depth,
                         std::vector<PngChunk> &tab, uint64_t *zoff)
{
	int fr, fc;
	if (png_parse_ihdr(f, len, &fr, &fc, depth)) return CCT_E_PNG;
	const size_t tab0 = tab.size();
	const uint64_t z0 = *zoff;
	auto refuse = [&](int code) { tab.resize(tab0); *zoff = z0; return code; };
	tab.push_back(PngChunk{base + 12, 0, 13, index});
	size_t p = 33;
	bool idat = false, idat_over = false, iend = false;
	while (p < len && !iend) {
		if (len - p < 12) return refuse(CCT_E_PNG);  // no room for length, type and CRC
		const uint32_t L = be32(f + p);
		if (L > 0x7FFFFFFFu || (size_t)L > len - p - 12) return refuse(CCT_E_PNG);  // runs past the file
		const uint8_t *t = f + p + 4;
		for (int k = 0; k < 4; k++)
			if (!((t[k] >= 'A' && t[k] <= 'Z') || (t[k] >= 'a' && t[k] <= 'z'))) return refuse(CCT_E_PNG);
		if (!memcmp(t, "IDAT", 4)) {
			if (idat_over) return refuse(CCT_E_PNG);  // IDAT chunks must be consecutive
			idat = true;
			tab.push_back(PngChunk{base + p + 4, *zoff, L, index | PNG_CHUNK_IDAT});
			*zoff += L;
		} else {
			if (idat) idat_over = true;
			if (!memcmp(t, "IEND", 4)) {
				if (L != 0) return refuse(CCT_E_PNG);
				iend = true;
			} else if (!(t[0] & 0x20)) {
				return refuse(CCT_E_PNG);  // a critical chunk this reader does not know (PLTE, a second IHDR, ...)
			}
			tab.push_back(PngChunk{base + p + 4, 0, L, index});
		}
		p += 12 + (size_t)L;
	}
	if (!iend || p != len || !idat) return refuse(CCT_E_PNG);
	if (fr != rows || fc != cols) return refuse(CCT_E_MIXED);
	return CCT_OK;
}

static const char *png_status_text(int code)
{
	return code == CCT_E_PNG     ? "not a PNG this reader takes"
	       : code == CCT_E_MIXED ? "IHDR size differs from the batch shape"
	       : code == CCT_E_CRC   ? "chunk CRC-32 mismatch"
	       : code == CCT_E_ZLIB  ? "invalid DEFLATE stream"
	                             : "stream is not rows * (1 + row bytes) long, or a filter type above 4";
}

// The INFLATE kernel stores no byte beyond its output stride, and when the flush that crosses the stride is the stream's last one
// it then reports the stream as invalid (the Adler-32 of bytes it did not sum cannot match) instead of as too long.  So a file
// the kernel calls invalid is told apart here, on the error path only: libz inflates its IDAT data into a scratch buffer, and a
// stream that libz takes to its end with another length than `want` is CCT_E_STREAM, not CCT_E_ZLIB.  files: the pass's upload.
static bool png_valid_stream_of_wrong_length(const uint8_t *files, const std::vector<PngChunk> &tab, uint32_t index, uint64_t want)
{
	z_stream zs{};
	if (inflateInit(&zs) != Z_OK) return false;
	std::vector<uint8_t> scratch(65536);
	uint64_t total = 0;
	int zr = Z_OK;
	for (const PngChunk &c : tab) {
		if (c.file != (index | PNG_CHUNK_IDAT) || zr != Z_OK) continue;
		zs.next_in = const_cast<Bytef *>(files + c.src + 4);
		zs.avail_in = c.len;
		while (zs.avail_in && zr == Z_OK) {
			zs.next_out = scratch.data();
			zs.avail_out = (uInt)scratch.size();
			zr = inflate(&zs, Z_NO_FLUSH);
			total += scratch.size() - zs.avail_out;
		}
	}
	(void)inflateEnd(&zs);
	return zr == Z_STREAM_END && total != want;
}

// files c0 .. c0 + nc of the batch
static int png_read_pass(DecSlot &D, const uint8_t *h_files, const uint64_t *h_offsets, int c0, int nc, int rows, int cols,
                         int shift, uint16_t *d_img, uint32_t *h_status, float ms[3])
{
	int rc;
	if ((rc = check_offsets(h_offsets + c0, nc, "file"))) return rc;
	const uint64_t a0 = h_offsets[c0], a1 = h_offsets[c0 + nc];
	std::vector<PngChunk> tab;
	std::vector<uint64_t> zoffs((size_t)nc + 1, 0);
	std::vector<uint32_t> fst((size_t)nc, 0), zst((size_t)nc, 0), osz((size_t)nc, 0);
	std::vector<uint8_t> bpp((size_t)nc, 2);
	uint64_t zoff = 0;
	int max_bpp = 0;
	for (int i = 0; i < nc; i++) {
		const uint64_t f0 = h_offsets[c0 + i], f1 = h_offsets[c0 + i + 1];
		int depth = 16;
		h_status[i] = (uint32_t)png_walk_file(h_files + f0, (size_t)(f1 - f0), f0 - a0, (uint32_t)i, rows, cols, &depth, tab, &zoff);
		zoffs[(size_t)i + 1] = zoff;
		if (h_status[i] != CCT_OK) { fst[i] = PNG_ST_SKIP; continue; }
		bpp[i] = (uint8_t)(depth / 8);
		max_bpp = std::max(max_bpp, depth / 8);
	}
	if (max_bpp == 0) return CCT_OK;  // every file refused by the walk: nothing for the device
	const size_t stride = (((size_t)rows * (1 + (size_t)cols * max_bpp) + 15) & ~(size_t)15) + 16;
	const size_t abytes = (size_t)(a1 - a0), zpad = ((size_t)zoff + 31) & ~(size_t)15;
	if ((rc = D.d_arch.ensure(abytes + 16))) return rc;
	if ((rc = D.d_png_z.ensure(zpad + 16))) return rc;
	if ((rc = D.d_png_tab.ensure(tab.size() * sizeof(PngChunk)))) return rc;
	if ((rc = D.d_png_bpp.ensure((size_t)nc))) return rc;
	if ((rc = D.d_archoffs.ensure(((size_t)nc + 1) * 8))) return rc;
	if ((rc = D.d_zstatus.ensure((size_t)nc * 4))) return rc;
	if ((rc = D.d_status.ensure((size_t)nc * 4))) return rc;
	if ((rc = D.d_sizes.ensure((size_t)nc * 4))) return rc;
	if ((rc = D.d_payload.ensure((size_t)nc * stride))) return rc;
	hipStream_t st = D.stream;
	StreamDrain drain(st);
	HIP_TRY(hipMemcpyAsync(D.d_arch.p, h_files + a0, abytes, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(D.d_png_tab.p, tab.data(), tab.size() * sizeof(PngChunk), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(D.d_png_bpp.p, bpp.data(), (size_t)nc, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(D.d_archoffs.p, zoffs.data(), ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(D.d_status.p, fst.data(), (size_t)nc * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(zero_read_ahead(D.d_png_z.p, zpad, st));
	PngUnpackArgs ua{};
	ua.files = (const uint8_t *)D.d_arch.p; ua.chunks = (const PngChunk *)D.d_png_tab.p;
	ua.streams = (uint8_t *)D.d_png_z.p; ua.status = (uint32_t *)D.d_status.p;
	HIP_TRY(hipEventRecord(D.ev_d0, st));
	HIP_TRY(launch_png_unpack(ua, (uint32_t)tab.size(), st));
	HIP_TRY(hipEventRecord(D.ev_d1, st));
	HIP_TRY(launch_inflate(inflate_args(D, D.d_png_z, zpad, 0, stride), nc, st, inflate_lanes_now()));
	HIP_TRY(hipEventRecord(D.ev_k_dec0, st));
	PngUnfilterArgs fa{};
	fa.rows = (uint8_t *)D.d_payload.p; fa.rows_stride = stride;
	fa.row_sizes = (const uint32_t *)D.d_sizes.p; fa.zstatus = (const uint32_t *)D.d_zstatus.p;
	fa.status = (uint32_t *)D.d_status.p; fa.bpp = (const uint8_t *)D.d_png_bpp.p;
	fa.nrows = rows; fa.cols = cols; fa.shift = shift;
	fa.images = d_img;
	HIP_TRY(launch_png_unfilter(fa, nc, g_ctx.png_unfilter_waves, st));
	HIP_TRY(hipEventRecord(D.ev_k_dec1, st));
	HIP_TRY(hipMemcpyAsync(fst.data(), D.d_status.p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(zst.data(), D.d_zstatus.p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(osz.data(), D.d_sizes.p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	float t[3] = {0, 0, 0};
	HIP_TRY(hipEventElapsedTime(&t[0], D.ev_d0, D.ev_d1));
	HIP_TRY(hipEventElapsedTime(&t[1], D.ev_d1, D.ev_k_dec0));
	HIP_TRY(hipEventElapsedTime(&t[2], D.ev_k_dec0, D.ev_k_dec1));
	for (int k = 0; k < 3; k++) ms[k] += t[k];
	for (int i = 0; i < nc; i++) {
		if (h_status[i] != CCT_OK) continue;
		const uint32_t want = (uint32_t)((size_t)rows * (1 + (size_t)cols * bpp[i]));
		if (fst[i] & PNG_ST_CRC) h_status[i] = CCT_E_CRC;
		else if (zst[i] & CCT_ST_ZLIB) h_status[i] = png_valid_stream_of_wrong_length(h_files + a0, tab, (uint32_t)i, want) ? CCT_E_STREAM : CCT_E_ZLIB;
		else if ((zst[i] & CCT_ST_STREAM) || osz[i] != want || (fst[i] & PNG_ST_FILTER)) h_status[i] = CCT_E_STREAM;
	}
	return CCT_OK;
}

int cct_png_read_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int rows, int cols, int shift,
                       uint16_t *images, int images_on_device, size_t images_cap_px, uint32_t *h_status)
{
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	if (shift < 0 || shift > 15) return fail(CCT_E_ARG, "PNG sample shift %d: 0 .. 15", shift);
	if (rows < 1 || cols < 1) return fail(CCT_E_ARG, "PNG shape %d x %d: rows and cols must be >= 1", rows, cols);
	if (png_filtered_bytes(rows, cols) > PNG_MAX_FILTERED)
		return fail(CCT_E_ARG, "PNG shape %d x %d: %zu filtered bytes exceed the reader's limit (%zu)", rows, cols,
		            png_filtered_bytes(rows, cols), PNG_MAX_FILTERED);
	if (n > 0 && (!h_files || !h_offsets || !images || !h_status)) return fail(CCT_E_ARG, "null argument");
	const size_t N = (size_t)rows * cols;
	if (images_cap_px / N < (size_t)n) return fail(CCT_E_CAP, "output holds %zu pixels, need %zu", images_cap_px, (size_t)n * N);
	if (n == 0) return CCT_OK;
	DecLease lease;
	int rc = lease_decode_slot(lease);
	if (rc) return rc;
	DecSlot &D = g_dec[lease.slot];
	// a pass holds the inflated rows of its files: at most DEFLATE_PASS_BYTES of them, as the writer's passes do
	const size_t stride16 = ((png_filtered_bytes(rows, cols) + 15) & ~(size_t)15) + 16;
	const int per_pass = (int)std::max<size_t>(1, DEFLATE_PASS_BYTES / stride16);
	if (!images_on_device && (rc = D.d_images.ensure((size_t)std::min(n, per_pass) * N * 2))) return rc;
	float ms[3] = {0, 0, 0};
	for (int c0 = 0; c0 < n; c0 += per_pass) {
		const int nc = std::min(per_pass, n - c0);
		uint16_t *d_img = images_on_device ? images + (size_t)c0 * N : (uint16_t *)D.d_images.p;
		if ((rc = png_read_pass(D, h_files, h_offsets, c0, nc, rows, cols, shift, d_img, h_status + c0, ms))) return rc;
		if (!images_on_device) {
			HIP_TRY(hipMemcpyAsync(images + (size_t)c0 * N, d_img, (size_t)nc * N * 2, hipMemcpyDeviceToHost, D.stream));
			HIP_TRY(hipStreamSynchronize(D.stream));
		}
	}
	tl_h2d_ms = ms[0]; tl_inflate_ms = ms[1]; tl_dec_kernel_ms = ms[2];
	for (int i = 0; i < n; i++)
		if (h_status[i] != CCT_OK) return fail((int)h_status[i], "file %d: %s", i, png_status_text((int)h_status[i]));
	return CCT_OK;
}

int cct_read_header(const uint8_t *h_file, size_t len, const char magic[4], cct_header *out)
{
	if (!h_file || !out) return fail(CCT_E_ARG, "null argument");
	if (len < 13) return fail(CCT_E_STREAM, "file shorter than the 13-byte header");
	if (memcmp(h_file, magic, 4) != 0) return fail(CCT_E_MAGIC, "Image does not contain valid header");
	out->width = (h_file[4] << 8) | h_file[5];
	out->height = (h_file[6] << 8) | h_file[7];
	out->channels = h_file[8];
	out->bytes_per_channel = h_file[9];
	out->fractal = h_file[10] != 0;
	out->segmentation = h_file[11] != 0;
	out->deflate = h_file[12] != 0;
	return CCT_OK;
}

int cct_decode_payload_dev(const uint8_t *d_payload, size_t payload_stride, const uint32_t *d_payload_sizes, int n,
                           int width, int height, int block_size, int fractal, uint16_t *d_images, uint32_t *d_status)
{
	std::lock_guard<std::mutex> lkd(g_mu_dec[0]);  // the workspaces of decode slot 0
	std::lock_guard<std::mutex> lk(g_mu);
	ApiCall in_call;
	int rc = check_shape(n, width, height, block_size);
	if (rc) return rc;
	if ((rc = ensure_ctx())) return rc;
	return decode_payload_locked(g_dec[0], d_payload, payload_stride, d_payload_sizes, n, width, height, block_size, fractal,
	                             d_images, d_status, g_ctx.stream);
}

int cct_decode_batch(const uint8_t *h_files, const uint64_t *h_offsets, int n, int block_size, const char magic[4],
                     uint16_t *images, int images_on_device, size_t images_cap_px, uint32_t *h_status)
{
	if (n < 0) return fail(CCT_E_ARG, "negative batch size");
	if (n == 0) return CCT_OK;
	DecLease lease;
	int rc = lease_decode_slot(lease);
	if (rc) return rc;
	DecSlot &D = g_dec[lease.slot];
	cct_header h0;
	if ((rc = cct_read_header(h_files + h_offsets[0], (size_t)(h_offsets[1] - h_offsets[0]), magic, &h0))) return rc;
	for (int i = 1; i < n; i++) {
		cct_header h;
		if ((rc = cct_read_header(h_files + h_offsets[i], (size_t)(h_offsets[i + 1] - h_offsets[i]), magic, &h))) return rc;
		if (h.width != h0.width || h.height != h0.height || h.fractal != h0.fractal || h.deflate != h0.deflate)
			return fail(CCT_E_MIXED, "file %d differs from file 0 in shape or flags", i);
	}
	if (h0.width == 0 || h0.height == 0) return fail(CCT_E_SHAPE, "empty image");
	if ((rc = check_shape(n, h0.width, h0.height, block_size))) return rc;
	const size_t N = (size_t)h0.width * h0.height;
	if (images_cap_px / N < (size_t)n) return fail(CCT_E_CAP, "output holds %zu pixels, need %zu", images_cap_px, (size_t)n * N);
	const size_t stride = cct_payload_stride(h0.width, h0.height, block_size);
	int zthreads = 1;
	{  // the slot's own buffers; no device lock, encodes and the other decode slot may be in flight
		HIP_TRY(hipSetDevice(g_ctx.device));
		if ((rc = D.dh_stage.ensure((size_t)n * stride))) return rc;
		if ((rc = D.d_payload.ensure((size_t)n * stride))) return rc;
		if ((rc = D.d_sizes.ensure((size_t)n * 4))) return rc;
		if ((rc = D.d_status.ensure((size_t)n * 4))) return rc;
		if (!images_on_device && (rc = D.d_images.ensure((size_t)n * N * 2))) return rc;
		zthreads = g_ctx.zlib_threads;
	}
	uint8_t *stage = (uint8_t *)D.dh_stage.p;
	std::vector<uint32_t> psz(n);
	for (int i = 0; i < n; i++) h_status[i] = CCT_OK;
	const bool dev_inflate = h0.deflate && g_ctx.device_inflate;
	std::vector<uint32_t> dst(n), zst(n, 0);
	std::vector<uint64_t> rel(dev_inflate ? n + 1 : 0);
	StreamDrain drain(D.stream);  // copies into the vectors above / the caller's images must land before any return
	if (dev_inflate) {
		// INFLATE on the device (inflate_kernels.hip): the archive goes up as it is, payloads never touch the host
		const uint64_t a0 = h_offsets[0], a1 = h_offsets[n];
		const size_t abytes = (size_t)(a1 - a0), apad = (abytes + 31) & ~(size_t)15;
		HIP_TRY(hipSetDevice(g_ctx.device));
		if ((rc = D.d_arch.ensure(apad + 16))) return rc;
		if ((rc = D.d_archoffs.ensure((size_t)(n + 1) * 8))) return rc;
		if ((rc = D.d_zstatus.ensure((size_t)n * 4))) return rc;
		for (int i = 0; i <= n; i++) rel[i] = h_offsets[i] - a0;
		hipStream_t st = D.stream;
		const double t_inf0 = now_ms();
		HIP_TRY(hipMemcpyAsync(D.d_arch.p, h_files + a0, abytes, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(D.d_archoffs.p, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
		const InflateArgs ia = inflate_args(D, D.d_arch, apad, 13, stride);
		// A decode issued while an encode batch is on the device is part of a pipeline (the bench: the decode of step k next to
		// the encode of step k+1, with slack): its kernels are released when the next transform+pack stage has ended, so that
		// they run next to that batch's sort and match kernels and not next to a tree or transform+pack kernel
		// (sched_kernels.hip has the measurements).  The archive upload above does not wait.  Option "decode_yields" = 0
		// launches at once.
		if (g_ctx.decode_yields && g_encodes_in_flight.load(std::memory_order_relaxed) > 0)
			HIP_TRY(launch_gate_wait(g_gate, g_gate_passes_issued.load(std::memory_order_relaxed), 600u, 20000u, st));
		HIP_TRY(hipEventRecord(D.ev_d0, st));
		HIP_TRY(launch_inflate(ia, n, st, inflate_lanes_now()));
		HIP_TRY(hipEventRecord(D.ev_d1, st));
		uint16_t *d_img = images_on_device ? images : (uint16_t *)D.d_images.p;
		hipEvent_t ev_k = D.ev_k_dec0, ev_k1 = D.ev_k_dec1;
		HIP_TRY(hipEventRecord(ev_k, st));
		rc = decode_payload_locked(D, (const uint8_t *)D.d_payload.p, stride, (const uint32_t *)D.d_sizes.p, n, h0.width,
		                           h0.height, block_size, h0.fractal, d_img, (uint32_t *)D.d_status.p, st);
		if (rc) return rc;
		HIP_TRY(hipEventRecord(ev_k1, st));
		HIP_TRY(hipMemcpyAsync(dst.data(), D.d_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(zst.data(), D.d_zstatus.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
		if (!images_on_device)
			HIP_TRY(hipMemcpyAsync(images, d_img, (size_t)n * N * 2, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(hipEventElapsedTime(&tl_inflate_ms, D.ev_d0, D.ev_d1));
		HIP_TRY(hipEventElapsedTime(&tl_dec_kernel_ms, ev_k, ev_k1));
		(void)t_inf0;
	} else {
	// INFLATE stage: zlib.decompress(file_bytes[13:]), core.py:421 -- host threads, no device lock held
	const double t_inf0 = now_ms();
	static std::mutex mu_team;  // one host team for the decode side: two slots take turns on this path
	std::unique_lock<std::mutex> lk_team(mu_team);
	g_team_dec.run(n, h0.deflate ? zthreads : 1, [&](int i) {
		const uint8_t *body = h_files + h_offsets[i] + 13;
		const size_t blen = (size_t)(h_offsets[i + 1] - h_offsets[i]) - 13;
		uint8_t *dst = stage + (size_t)i * stride;
		if (h0.deflate) {
			uLongf dl = (uLongf)stride;
			const int zr = uncompress(dst, &dl, body, (uLong)blen);
			if (zr == Z_BUF_ERROR) { h_status[i] = CCT_E_STREAM; psz[i] = 0; }  // longer than any valid stream
			else if (zr != Z_OK) { h_status[i] = CCT_E_ZLIB; psz[i] = 0; }
			else psz[i] = (uint32_t)dl;
		} else {
			if (blen > stride) { h_status[i] = CCT_E_STREAM; psz[i] = 0; }
			else { memcpy(dst, body, blen); psz[i] = (uint32_t)blen; }
		}
	});
	lk_team.unlock();
	const float t_inflate = (float)(now_ms() - t_inf0);
	{  // device phase on the decode stream (no device lock: the HIP runtime is thread-safe)
		hipStream_t st = D.stream;
		tl_inflate_ms = t_inflate;
		// one strided copy of the used part of every staged payload (a copy per slice costs more in launches
		// than in bytes)
		size_t used = 16;
		for (int i = 0; i < n; i++) used = std::max(used, (size_t)((psz[i] + 15u) & ~15u));
		used = std::min(used, stride);
		const double t_h0 = now_ms();
		HIP_TRY(hipMemcpy2DAsync(D.d_payload.p, stride, stage, stride, used, (size_t)n, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(D.d_sizes.p, psz.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
		uint16_t *d_img = images_on_device ? images : (uint16_t *)D.d_images.p;
		HIP_TRY(hipEventRecord(D.ev_d0, st));
		rc = decode_payload_locked(D, (const uint8_t *)D.d_payload.p, stride, (const uint32_t *)D.d_sizes.p, n, h0.width,
		                           h0.height, block_size, h0.fractal, d_img, (uint32_t *)D.d_status.p, st);
		if (rc) return rc;
		HIP_TRY(hipEventRecord(D.ev_d1, st));
		HIP_TRY(hipMemcpyAsync(dst.data(), D.d_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
		if (!images_on_device)
			HIP_TRY(hipMemcpyAsync(images, d_img, (size_t)n * N * 2, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(hipEventElapsedTime(&tl_dec_kernel_ms, D.ev_d0, D.ev_d1));
		if (trace_on())
			fprintf(stderr, "[cct] decode n=%d: inflate %.2f ms, h2d+kernel+sync %.2f ms (kernel %.2f), used %zu of stride %zu\n", n,
			        t_inflate, now_ms() - t_h0, tl_dec_kernel_ms, used, stride);
	}
	}
	int first = CCT_OK;
	for (int i = 0; i < n; i++) {
		if (h_status[i] == CCT_OK) {
			if (zst[i] & CCT_ST_ZLIB) h_status[i] = CCT_E_ZLIB;
			else if ((zst[i] | dst[i]) & CCT_ST_STREAM) h_status[i] = CCT_E_STREAM;
			else if (dst[i] & CCT_ST_OVERFLOW) h_status[i] = CCT_E_OVERFLOW;
		}
		if (h_status[i] != CCT_OK && first == CCT_OK) {
			first = (int)h_status[i];
			fail(first, "file %d: %s", i,
			     first == CCT_E_ZLIB ? "invalid DEFLATE stream"
			     : first == CCT_E_OVERFLOW ? "int too big to convert (pixel left the 16-bit range)"
			                               : "truncated or malformed token stream");
		}
	}
	return first;
}

int cct_last_timings(float *out6)
{
	// no lock: this only reads a few floats, and taking the device lock here would park the caller behind a
	// whole batch that another thread is encoding
	out6[0] = tl_enc_kernel_ms; out6[1] = tl_d2h_ms; out6[2] = tl_deflate_ms;
	out6[3] = tl_inflate_ms; out6[4] = tl_dec_kernel_ms; out6[5] = tl_h2d_ms;
	return CCT_OK;
}

}  // extern "C"

namespace {
// One table for cct_set_option and cct_get_option.  `rule` validates or clamps a value on its way in (it may refuse with a
// message); read-only keys have none.  Tuning-only keys are unknown to a release build (tuning.h).
struct Option {
	const char *name;
	int Context::*member;
	int (*rule)(int &value);
	bool read_only, tuning_only;
};
int rule_any(int &) { return CCT_OK; }
int rule_bool(int &v) { v = v ? 1 : 0; return CCT_OK; }
const Option OPTIONS[] = {
	{"zlib_threads", &Context::zlib_threads, [](int &v) { return v < 1 ? fail(CCT_E_ARG, "zlib_threads < 1") : CCT_OK; }},
	{"tile_path", &Context::use_tiles, [](int &v) {
		if (v == 3) return fail(CCT_E_ARG, "tile_path 3 (the four-kernel pipeline) has been removed");
		v = (v >= 0 && v <= 4) ? v : 1; return (int)CCT_OK; }},
	{"stream_tpg", &Context::stream_tpg, [](int &v) { v = (v == 1 || v == 2 || v == 4) ? v : STREAM_TPG; return (int)CCT_OK; }},
	{"runtime_block_size", &Context::runtime_bs, rule_bool},
	{"device_deflate", &Context::device_deflate, rule_bool},
	{"device_inflate", &Context::device_inflate, rule_bool},
	{"deflate_graph", &Context::use_graph, rule_bool},
	{"deflate_compact_records", &Context::compact_recs, rule_bool},
	{"decode_yields", &Context::decode_yields, rule_bool},
	{"queue_ahead", &Context::queue_ahead, rule_bool},
	{"deflate_fork", &Context::deflate_fork, rule_bool},
	{"tree_waves", &Context::tree_waves, [](int &v) {
		return v != 0 && v != 1 && v != 16 ? fail(CCT_E_ARG, "tree_waves must be 0 (automatic), 1 or 16") : CCT_OK; }},
	{"encode_slots", &Context::enc_slots, [](int &v) { v = std::max(1, std::min(v, N_ENC_SLOTS)); return (int)CCT_OK; }},
	{"decode_slots", &Context::dec_slots, [](int &v) { v = std::max(1, std::min(v, N_DEC_SLOTS)); return (int)CCT_OK; }},
	{"inflate_lanes", &Context::inflate_lanes, [](int &v) {
		return v != 0 && v != 256 && v != 512 ? fail(CCT_E_ARG, "inflate_lanes must be 0 (automatic), 256 or 512") : CCT_OK; }},
	{"png_unfilter_waves", &Context::png_unfilter_waves, [](int &v) {
		return v != 1 && v != 2 && v != 4 && v != 8 ? fail(CCT_E_ARG, "png_unfilter_waves must be 1, 2, 4 or 8") : CCT_OK; }},
	{"wg_threads", &Context::wg_threads, [](int &v) {
		return v != 256 && v != 512 && v != 1024 ? fail(CCT_E_ARG, "wg_threads must be 256, 512 or 1024") : CCT_OK; }},
	{"last_encode_path", &Context::last_path, nullptr, true},
	{"last_decode_path", &Context::last_dec_path, nullptr, true},
	{"last_decode_block_path", &Context::last_dec_block_path, nullptr, true},
	{"last_inflate_lanes", &Context::last_inflate_lanes, nullptr, true},
	{"debug_skip", &Context::dbg_skip, rule_any, false, true},
	{"tuning_build", &Context::tuning_build, nullptr, true, true},
};
const Option *find_option(const char *key)
{
	for (const Option &o : OPTIONS)
		if (!strcmp(key, o.name) && (TUNING || !o.tuning_only)) return &o;
	fail(CCT_E_ARG, "unknown option %s", key);
	return nullptr;
}
}  // namespace

extern "C" {

int cct_set_option(const char *key, int value)
{
	std::lock_guard<std::mutex> lk(g_mu);
	const Option *o = find_option(key);
	if (!o) return CCT_E_ARG;
	if (o->read_only) return fail(CCT_E_ARG, "unknown option %s", key);
	if (int rc = o->rule(value)) return rc;
	g_ctx.*o->member = value;
	return CCT_OK;
}
int cct_get_option(const char *key, int *value)
{
	std::lock_guard<std::mutex> lk(g_mu);
	const Option *o = find_option(key);
	if (!o) return CCT_E_ARG;
	*value = g_ctx.*o->member;
	return CCT_OK;
}

}  // extern "C"
