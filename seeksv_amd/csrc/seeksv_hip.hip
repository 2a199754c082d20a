// seeksv_hip.hip - context, memory management and the C ABI (include/seeksv_hip.h) over the gfx950 kernels.
// One context = one GPU = one HIP stream.  No CPU fallback: every entry point needs a live device.
#include "seeksv_hip.h"

#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <dlfcn.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <deque>
#include <functional>
#include <memory>
#include <vector>

#include "batch_columns.h"
#include "bamdec_kernels.h"
#include "realign_kernels.h"
#include "realign_sorted_kernels.h"
#include "realign_gap_kernels.h"
#include "realign_alts_kernels.h"
#include "realign_split_kernels.h"
#include "realign_rows_kernels.h"
#include "clip_kernels.h"
#include "table3_kernels.h"
#include "tile_sort.h"
#include "common.h"
#include "cpus.h"
#include "getsv_kernels.h"
#include "radix_sort.h"
#include "readthrough_kernels.h"
#include "splitread_kernels.h"
#include "samdec_kernels.h"
#include "splitread_sa_kernels.h"
#include "alnpack_kernels.h"
#include "probe_kernels.h"
#include "dup_kernels.h"
#include "sort_kernels.h"
#include "pairdup_kernels.h"
#include "region_kernels.h"
#include "scan.h"

using namespace ssv;

namespace {

thread_local std::string g_create_error; // (per thread: ssv_last_error(NULL) is asked by the thread whose call failed; rank and reader threads run side by side)

// timed kernel groups (ssv_prof_*)
enum ProfId { P_H2D, P_CLIP_SCAN, P_CLIP_PLACE, P_CLIP_GATHER, P_SORT, P_CLUSTER_BINS, P_CLUSTER_PACK, P_TABLE_D2H, P_ISIZE, P_GETSV_SCAN, P_GETSV_CAND, P_DEPTH_FINISH, P_BAM_INFLATE, P_BAM_RECORDS, P_BAM_DECODE, P_REALIGN_INDEX, P_REALIGN_QUERY, P_BAM_UPLOAD, P_BAM_RESOLVE, P_RT_SCAN, P_RT_FINISH, P_REALIGN_GAP, P_REALIGN_ALTS, P_REALIGN_ROWS, P_SOMATIC_PROBE, P_DUP_SELECT, P_DUP_MARK, P_DUP_RETAIN, P_SORT_KEYS, P_SORT_RADIX, P_SORT_GATHER, P_PAIRDUP_ENDS, P_PAIRDUP_JOIN, P_PAIRDUP_MARK, P_REGION_SELECT, P_REGION_GATHER, P_SPLITREAD_SA_AUX, P_SPLITREAD_SA_SCAN, P_SPLITREAD_SA_FINISH, P_SPLITREAD_SCAN, P_SPLITREAD_FINISH, P_COUNT };
const char *const kProfNames[P_COUNT] = {"h2d", "clip_scan", "clip_place", "clip_gather", "event_sort", "cluster_bins", "cluster_pack", "table_d2h", "isize_stats", "getsv_scan", "getsv_cand", "depth_finish", "bam_inflate", "bam_records", "bam_decode", "realign_index", "realign_query", "bam_upload", "bam_resolve", "rt_scan", "rt_finish", "realign_gap", "realign_alts", "realign_rows", "somatic_probe", "dup_select", "dup_mark", "dup_retain", "sort_keys", "sort_radix", "sort_gather", "pairdup_ends", "pairdup_join", "pairdup_mark", "region_select", "region_gather", "splitread_sa_aux", "splitread_sa_scan", "splitread_sa_finish", "splitread_scan", "splitread_finish"};
const char kProfNameList[] = "h2d\nclip_scan\nclip_place\nclip_gather\nevent_sort\ncluster_bins\ncluster_pack\ntable_d2h\nisize_stats\ngetsv_scan\ngetsv_cand\ndepth_finish\nbam_inflate\nbam_records\nbam_decode\nrealign_index\nrealign_query\nbam_upload\nbam_resolve\nrt_scan\nrt_finish\nrealign_gap\nrealign_alts\nrealign_rows\nsomatic_probe\ndup_select\ndup_mark\ndup_retain\nsort_keys\nsort_radix\nsort_gather\npairdup_ends\npairdup_join\npairdup_mark\nregion_select\nregion_gather\nsplitread_sa_aux\nsplitread_sa_scan\nsplitread_sa_finish\nsplitread_scan\nsplitread_finish";

hipError_t pinned_delete(void *p);

// grow-only buffer that owns its memory: freed when the buffer goes (move-only); Free's return code is only looked at through release()
template <hipError_t (*Free)(void *)> struct Buf {
	void *p = nullptr;
	size_t cap = 0;
	Buf() = default;
	Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
	Buf &operator=(Buf &&o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
	~Buf() { reset(); }
	hipError_t release() { const hipError_t e = p ? Free(p) : hipSuccess; p = nullptr; cap = 0; return e; }
	void reset() { (void)release(); }
};
using DBuf = Buf<hipFree>;       // device memory
using HBuf = Buf<pinned_delete>; // pinned host memory (ensure_host)
static_assert(!std::is_copy_constructible_v<DBuf> && !std::is_copy_constructible_v<HBuf> && std::is_nothrow_move_constructible_v<DBuf>, "buffers have one owner");

// Device memory that is handed out in pieces and never moves (clip events hold addresses into it): a list of chunks with a cursor,
// rewound at the start of every getclip pass.
struct Arena {
	std::vector<DBuf> chunks;
	size_t cur = 0, used = 0;
};

struct ProfRec {
	int id;
	hipEvent_t a, b;
	int64_t units;
};

} // namespace

// A few host threads that stay around (the compact table's columns are rebuilt on them once per table: starting 64 threads costs more than
// the work they do).  run(n, fn) calls fn(0..n-1), fn(0) on the caller's thread, and returns when all are done.
struct HostPool {
	std::vector<std::thread> th;
	std::mutex mu;
	std::condition_variable cv_go, cv_done;
	const std::function<void(int)> *fn = nullptr;
	uint64_t generation = 0;
	int n_jobs = 0, n_left = 0;
	bool quit = false;
	void worker(int id)
	{
		uint64_t seen = 0;
		for (;;) {
			const std::function<void(int)> *f;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv_go.wait(lk, [&] { return quit || generation != seen; });
				if (quit) return;
				seen = generation;
				if (id >= n_jobs) continue;
				f = fn;
			}
			(*f)(id);
			std::unique_lock<std::mutex> lk(mu);
			if (--n_left == 0) cv_done.notify_all();
		}
	}
	void run(int n, const std::function<void(int)> &f)
	{
		if (n <= 1) { f(0); return; }
		while ((int)th.size() < n - 1) { const int id = (int)th.size() + 1; th.emplace_back([this, id] { worker(id); }); }
		{
			std::unique_lock<std::mutex> lk(mu);
			fn = &f; n_jobs = n; n_left = n - 1; ++generation;
		}
		cv_go.notify_all();
		f(0);
		std::unique_lock<std::mutex> lk(mu);
		cv_done.wait(lk, [&] { return n_left == 0; });
	}
	~HostPool()
	{
		{ std::unique_lock<std::mutex> lk(mu); quit = true; }
		cv_go.notify_all();
		for (auto &t : th) t.join();
	}
};

// ---- copies over the host link on an SDMA engine WE name ----
// hipMemcpyAsync lets the runtime pick the engine, and an MI355X has sixteen of which only four sit beside the PCIe root (tools/sdma_engine_probe.cpp: a 0.55 GB device-to-host copy takes
// 9.72 ms on engines 0-3, 43 ms on 4-7, 55-60 ms on 8-11, 72-78 ms on 12-15; host-to-device 9.65 / 10.9 / 13.7-15.2 / 18-19.5 ms).  On some boxes of the pool the runtime's choice (or the way
// it splits a large copy over several engines) made the SAME cluster table cross PCIe in 9.7 or in 12-18 ms from one copy to the next, and the compressed chunks of a BAM at 36-46 GB/s instead
// of 57 (round 6, profiles/r06_host_link.txt).  The two copies this path lives on - the cluster table to the host, a BAM's compressed chunks to the device - therefore go to the runtime's
// layer below HIP (hsa_amd_memory_async_copy_on_engine, found with dlsym: no link-time dependency) on the engine hsa_amd_memory_get_preferred_copy_engine names for the direction, with an HSA
// signal for the end.  Anything missing - the library, a symbol, the agents, a preferred engine - and the copy is hipMemcpyAsync's as before.  SSV_LINK_COPY=hip: that form always.
struct LinkCopy {
	bool ok = false;
	hsa_agent_t gpu{}, cpu{};
	uint32_t eng_to_host = 0, eng_to_device = 0; // the engine in use per direction, one bit each (hsa_amd_sdma_engine_id_t)
	// An engine is not ours alone: the kernel driver wipes freed device memory on one of them - for seconds behind a free of tens of GB, ours or that of the process before us -, and a
	// copy that shares it runs at half the link's rate (tools/free_wipe_probe.cpp, tools/sdma_engine_probe.cpp: engine 1 at 18.4 ms while 0, 2, 3 took 9.7).  So every large copy is
	// timed (the runtime's async-copy timestamps) and a direction moves on to the next of its candidate engines when a copy came in well below the best rate seen.
	struct Dir { std::vector<uint32_t> cand; std::vector<double> rate; size_t cur = 0; } to_host, to_device; // rate: GB/s of the candidate's last timed copy (0: not tried yet)
	double ticks_per_s = 0;
	decltype(&hsa_amd_profiling_get_async_copy_time) copy_time = nullptr;
	decltype(&hsa_signal_create) signal_create = nullptr;
	decltype(&hsa_signal_destroy) signal_destroy = nullptr;
	decltype(&hsa_signal_store_relaxed) signal_store = nullptr;
	decltype(&hsa_signal_wait_scacquire) signal_wait = nullptr;
	decltype(&hsa_signal_load_relaxed) signal_load = nullptr;
	decltype(&hsa_amd_memory_async_copy_on_engine) copy_on_engine = nullptr;
};

// a stage's state lives in the stage's file, behind a pointer here: the three oldest stages' from ssv_ctx_create on (their entry points look at it
// in every state), the others' from their first *_begin
struct ssv_clip_state;   // clip_api.inc
struct ssv_isize_state;  // isize_api.inc
struct ssv_getsv_state;  // getsv_api.inc
struct ssv_bamdec_state; // bamdec_api.inc
struct ssv_realign_state; // realign_api.inc
struct ssv_rt_state;     // readthrough_api.inc
struct ssv_samdec_state; // samdec_api.inc
struct ssv_alnpack_state; // alnpack_api.inc
struct ssv_probe_state;  // probe_api.inc
struct ssv_dup_state;    // dup_api.inc
struct ssv_sort_state;   // sort_api.inc
struct ssv_pairdup_state; // pairdup_api.inc
struct ssv_region_state;  // region_api.inc

struct ssv_ctx { // (created and deleted below the stage files only: the state structs are complete there)
	int device = 0;
	hipStream_t st = nullptr;
	std::string err;

	// ssv_batch_retain's memory: batches are cut out of arenas (a few large allocations instead of one per batch - with 320 batches of a whole-genome file kept,
	// `seeksv run` spent 0.9 s in allocations that grew slower with every one; an arena is given back when its last batch is released)
	struct RetainArena { uint8_t *base = nullptr; size_t cap = 0, used = 0; int64_t live = 0; std::vector<size_t> slabs; }; // slabs: where the arena's live batches begin
	std::vector<RetainArena> arenas;
	// arenas whose last batch was released: kept for the next ssv_batch_retain instead of handed back (round 6: a hipMalloc of 4 GB behind the release of tens of GB
	// took 0.6-1.7 s - the driver clears freed memory before it hands it out again -, once in every third run of bench.py's file leg); handed back when any
	// allocation of the context fails for lack of memory (dev_malloc), and with the context
	struct SpareArena { uint8_t *base; size_t cap; };
	std::vector<SpareArena> spare_arenas;
	// ... and the arena behind the one in use is allocated AHEAD, on a thread of its own, when the newest one is first cut into: a fresh process has no spares, and
	// its allocations may wait for memory that the process before it gave back (`seeksv run` behind `seeksv getsv`: 0.4-0.7 s of such waits inside getclip's
	// scan phase in two runs of three) - behind the decode of the batches that fill the current arena nobody waits for them
	struct ArenaAhead { std::thread th; bool pending = false; uint8_t *base = nullptr; size_t cap = 0; } ahead;

	// staging of host batches, and the record lines built for batches that come without them
	// host batches are copied into one of three staging sets: 0 and 1 take the batches announced with ssv_batch_prefetch (copied on st_h2d while
	// the kernels of the batch before run on st), 2 the ones that come unannounced (copied on st itself)
	struct StageSet { DBuf col[COL_COUNT], rec; hipEvent_t ready = nullptr; } ss[3];
	struct Prefetched { ssv_batch_t b; int set; };
	std::deque<Prefetched> pf;
	uint64_t pf_count = 0;
	hipStream_t st_h2d = nullptr;
	hipEvent_t ev_st = nullptr;

	// scratch shared by the passes
	DBuf tile_cnt, tile_off, tile_base, scan_scratch, scan_scratch64, counters, totals;
	HBuf h_counters, h_totals;
	DBuf stage; int64_t stage_cap = 0; // the scans' staging of candidates (getclip, getsv)
	DBuf ends_buf, ghist;              // cigar_ends built from the lines (getclip, getsv -F); radix histograms (getclip, getsv -F)
	HBuf h_batch;                      // ssv_batch_to_host

	hipStream_t st_copy = nullptr;
	hipEvent_t ev_packed = nullptr;
	LinkCopy link;             // the named SDMA engines of the host link (ok == false: hipMemcpyAsync)

	std::unique_ptr<ssv_clip_state> clip;
	std::unique_ptr<ssv_isize_state> isz;
	std::unique_ptr<ssv_getsv_state> getsv;
	std::unique_ptr<ssv_bamdec_state> bd;
	std::unique_ptr<ssv_realign_state> ra;
	std::unique_ptr<ssv_rt_state> rt;
	std::unique_ptr<ssv_samdec_state> sd;
	std::unique_ptr<ssv_alnpack_state> ap;
	std::unique_ptr<ssv_probe_state> probe;
	std::unique_ptr<ssv_dup_state> dup;
	std::unique_ptr<ssv_sort_state> sort;
	std::unique_ptr<ssv_pairdup_state> pairdup;
	std::unique_ptr<ssv_region_state> region;
	// the retained batches that carry rows of ssv_pairdup_retain which no ssv_pairdup_mark has used yet (slab: where the batch begins, its tid column)
	struct PairdupLive { const void *slab; int64_t n; void *rows; };
	std::vector<PairdupLive> pairdup_live;

	// ---- profiling ----
	int prof_mode = 0;
	std::vector<ProfRec> prof_recs;
	std::vector<hipEvent_t> prof_pool;
	double prof_ms[P_COUNT] = {0};
	int64_t prof_launches[P_COUNT] = {0};
	int64_t prof_units[P_COUNT] = {0};
};

namespace {

#define HIPCHECK(ctx, call)                                                                              \
	do {                                                                                                   \
		hipError_t e_ = (call);                                                                              \
		if (e_ != hipSuccess) {                                                                              \
			(ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                    \
			return e_ == hipErrorOutOfMemory ? SSV_E_NOMEM : SSV_E_HIP;                                        \
		}                                                                                                    \
	} while (0)

#define CHECK(expr)          \
	do {                       \
		int rc_ = (expr);        \
		if (rc_ != SSV_OK) return rc_; \
	} while (0)

// the arena that was asked for ahead, if any (null when there is none or its allocation failed); the caller owns it
static uint8_t *arena_ahead_take(ssv_ctx *c, size_t *cap)
{
	if (!c->ahead.pending) return nullptr;
	c->ahead.th.join();
	c->ahead.pending = false;
	uint8_t *b = c->ahead.base;
	*cap = c->ahead.cap;
	c->ahead.base = nullptr; c->ahead.cap = 0;
	return b;
}

static void arena_ahead_start(ssv_ctx *c, size_t cap)
{
	if (c->ahead.pending) return;
	c->ahead.pending = true;
	c->ahead.base = nullptr; c->ahead.cap = cap;
	const int device = c->device;
	ssv_ctx::ArenaAhead *a = &c->ahead;
	c->ahead.th = std::thread([a, device, cap] {
		void *p = nullptr;
		if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, cap) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
		a->base = static_cast<uint8_t *>(p);
	});
}

// hipMalloc; out of memory: what the context keeps in reserve (ssv_batch_retain's spare arenas, the one asked for ahead) goes back first
hipError_t dev_malloc(ssv_ctx *c, void **p, size_t bytes)
{
	hipError_t e = hipMalloc(p, bytes);
	if (e == hipErrorOutOfMemory && (!c->spare_arenas.empty() || c->ahead.pending)) {
		(void)hipGetLastError();
		(void)hipStreamSynchronize(c->st);
		size_t cap = 0;
		if (uint8_t *b = arena_ahead_take(c, &cap)) (void)hipFree(b);
		for (auto &a : c->spare_arenas) (void)hipFree(a.base);
		c->spare_arenas.clear();
		e = hipMalloc(p, bytes);
	}
	return e;
}

int ensure(ssv_ctx *c, DBuf &b, size_t bytes, bool keep = false, size_t keep_bytes = 0)
{
	if (bytes <= b.cap) return SSV_OK;
	size_t ncap = std::max(bytes, b.cap + b.cap / 2);
	ncap = (ncap + 255) & ~(size_t)255;
	DBuf nb;
	HIPCHECK(c, dev_malloc(c, &nb.p, ncap));
	nb.cap = ncap;
	if (keep && b.p && keep_bytes) {
		HIPCHECK(c, hipMemcpyAsync(nb.p, b.p, keep_bytes, hipMemcpyDeviceToDevice, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
	}
	if (b.p) {
		HIPCHECK(c, hipStreamSynchronize(c->st));
		HIPCHECK(c, b.release());
	}
	b = std::move(nb);
	return SSV_OK;
}

// Page-locked host memory.  hipHostMalloc hands out 4 KB pages: allocating, clearing and locking them runs on one thread at ~0.25 s/GB under the runtime's lock, and
// when the process ends the kernel takes every page's lock back one by one - tools/exit_cost.cpp: 4 GB of such memory cost 0.18 s to lock and 0.41-0.45 s between
// _exit and the parent's wait() returning, whatever else the process held (48 GB of device memory: 0.06 s).  That was the 0.2-0.6 s a `seeksv` command spent AFTER its
// last statement (round 6, bench.py: exit_to_reaped_s).  Buffers of 2 MB and more are therefore anonymous memory on TRANSPARENT HUGE PAGES (madvise: 2 MB pages where
// the kernel grants them - it falls back to 4 KB pages by itself), touched by a few threads, then registered with the runtime: 0.008 s to lock 4 GB, 0.001 s to leave.
// SSV_PINNED=malloc: hipHostMalloc as before (the form the tests compare with).
namespace {
struct PinnedMaps { std::mutex mu; std::unordered_map<void *, std::pair<void *, size_t>> m; }; // user pointer -> (mapping, its length)
PinnedMaps &pinned_maps() { static PinnedMaps *p = new PinnedMaps; return *p; } // (never destroyed: buffers may be freed from static destructors)
constexpr size_t HUGE_PAGE = (size_t)2 << 20;
}

// the NUMA node a GPU hangs on (sysfs numa_node of its PCI function; -1: unknown or a one-node box)
static int device_numa_node(int device)
{
	static std::mutex mu;
	static std::unordered_map<int, int> cache;
	std::lock_guard<std::mutex> lk(mu);
	auto it = cache.find(device);
	if (it != cache.end()) return it->second;
	int node = -1;
	char bdf[64] = {0};
	if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), device) == hipSuccess) {
		for (char *q = bdf; *q; ++q) *q = (char)tolower((unsigned char)*q);
		const std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/numa_node";
		if (FILE *f = fopen(path.c_str(), "r")) { if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
	} else (void)hipGetLastError();
	cache[device] = node;
	return node;
}

static void bind_near(void *p, size_t bytes, int device)
{
	const int node = device_numa_node(device);
	if (node < 0 || node >= 1024 || !p || !bytes) return;
	unsigned long mask[16] = {0};
	mask[node / (8 * sizeof(unsigned long))] |= 1ul << (node % (8 * sizeof(unsigned long)));
	(void)syscall(SYS_mbind, p, (unsigned long)bytes, 1 /* MPOL_PREFERRED */, mask, (unsigned long)(8 * sizeof(mask)), 0u); // (refused by a cpuset that does not hold the node: the pages land where they land)
}

static hipError_t pinned_new(void **out, size_t bytes, unsigned malloc_flags)
{
	static const bool plain = [] { const char *e = getenv("SSV_PINNED"); return e && !strcmp(e, "malloc"); }();
	*out = nullptr;
	if (plain || bytes < HUGE_PAGE) return hipHostMalloc(out, bytes ? bytes : 1, malloc_flags);
	const size_t n = (bytes + HUGE_PAGE - 1) & ~(HUGE_PAGE - 1), len = n + HUGE_PAGE;
	void *m = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
	if (m == MAP_FAILED) return hipHostMalloc(out, bytes, malloc_flags);
	uint8_t *a = reinterpret_cast<uint8_t *>(((uintptr_t)m + HUGE_PAGE - 1) & ~(uintptr_t)(HUGE_PAGE - 1));
	(void)madvise(a, n, MADV_HUGEPAGE);
	{ int dev = 0; if (hipGetDevice(&dev) == hipSuccess) bind_near(a, n, dev); else (void)hipGetLastError(); } // the pages on the GPU's own NUMA node, whichever CPUs touch them
	{ // first touch on a few threads (a fault clears 2 MB - or 4 KB, 512 times as often - before the runtime's call locks the pages one after the other)
		const int nt = (int)std::max<size_t>(1, std::min<size_t>({(size_t)8, n >> 25, (size_t)ssv::effective_cpus()}));
		auto touch = [a, n, nt](int t) { for (size_t o = n / HUGE_PAGE * (size_t)t / (size_t)nt * HUGE_PAGE, e = n / HUGE_PAGE * (size_t)(t + 1) / (size_t)nt * HUGE_PAGE; o < e; o += 4096) a[o] = 0; };
		std::vector<std::thread> th;
		for (int t = 1; t < nt; ++t) th.emplace_back(touch, t);
		touch(0);
		for (auto &x : th) x.join();
	}
	if (hipHostRegister(a, n, hipHostRegisterPortable) != hipSuccess) { // (a kernel or limit that refuses: the runtime's own allocator)
		(void)hipGetLastError();
		munmap(m, len);
		return hipHostMalloc(out, bytes, malloc_flags);
	}
	{ std::lock_guard<std::mutex> lk(pinned_maps().mu); pinned_maps().m[a] = std::make_pair(m, len); }
	*out = a;
	return hipSuccess;
}

hipError_t pinned_delete(void *p)
{
	if (!p) return hipSuccess;
	std::pair<void *, size_t> mapping(nullptr, 0);
	{
		std::lock_guard<std::mutex> lk(pinned_maps().mu);
		auto it = pinned_maps().m.find(p);
		if (it != pinned_maps().m.end()) { mapping = it->second; pinned_maps().m.erase(it); }
	}
	if (!mapping.first) return hipHostFree(p);
	const hipError_t e = hipHostUnregister(p);
	munmap(mapping.first, mapping.second);
	return e;
}

// find the agents and the engines (once per context; quiet on failure: the context then copies the runtime's way)
static void link_init(ssv_ctx *c)
{
	LinkCopy &L = c->link;
	const char *e = getenv("SSV_LINK_COPY");
	if (e && !strcmp(e, "hip")) return;
	void *lib = dlopen("libhsa-runtime64.so.1", RTLD_NOW | RTLD_GLOBAL);
	if (!lib) lib = dlopen("libhsa-runtime64.so", RTLD_NOW | RTLD_GLOBAL);
	if (!lib) return;
	auto sym = [&](const char *name) { return dlsym(lib, name); };
	auto f_init = reinterpret_cast<decltype(&hsa_init)>(sym("hsa_init"));
	auto f_iter = reinterpret_cast<decltype(&hsa_iterate_agents)>(sym("hsa_iterate_agents"));
	auto f_info = reinterpret_cast<decltype(&hsa_agent_get_info)>(sym("hsa_agent_get_info"));
	auto f_pref = reinterpret_cast<decltype(&hsa_amd_memory_get_preferred_copy_engine)>(sym("hsa_amd_memory_get_preferred_copy_engine"));
	auto f_stat = reinterpret_cast<decltype(&hsa_amd_memory_copy_engine_status)>(sym("hsa_amd_memory_copy_engine_status"));
	L.signal_create = reinterpret_cast<decltype(L.signal_create)>(sym("hsa_signal_create"));
	L.signal_destroy = reinterpret_cast<decltype(L.signal_destroy)>(sym("hsa_signal_destroy"));
	L.signal_store = reinterpret_cast<decltype(L.signal_store)>(sym("hsa_signal_store_relaxed"));
	L.signal_wait = reinterpret_cast<decltype(L.signal_wait)>(sym("hsa_signal_wait_scacquire"));
	L.signal_load = reinterpret_cast<decltype(L.signal_load)>(sym("hsa_signal_load_relaxed"));
	L.copy_on_engine = reinterpret_cast<decltype(L.copy_on_engine)>(sym("hsa_amd_memory_async_copy_on_engine"));
	if (!f_init || !f_iter || !f_info || !f_pref || !f_stat || !L.signal_create || !L.signal_destroy || !L.signal_store || !L.signal_wait || !L.signal_load || !L.copy_on_engine) return;
	if (f_init() != HSA_STATUS_SUCCESS) return; // (reference counted: HIP holds the runtime up already)
	// the GPU agent with this device's PCI address, and a CPU agent
	char bdf[64] = {0};
	if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), c->device) != hipSuccess) { (void)hipGetLastError(); return; }
	unsigned dom = 0, bus = 0, dev = 0, fn = 0;
	if (sscanf(bdf, "%x:%x:%x.%x", &dom, &bus, &dev, &fn) != 4) return;
	struct Find { decltype(f_info) info; uint32_t want_bdf, want_dom; hsa_agent_t gpu, cpu; bool have_gpu, have_cpu; } F{f_info, (bus << 8) | (dev << 3) | fn, dom, {}, {}, false, false};
	f_iter([](hsa_agent_t a, void *p) -> hsa_status_t {
		Find &F = *static_cast<Find *>(p);
		hsa_device_type_t t;
		if (F.info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
		if (t == HSA_DEVICE_TYPE_CPU && !F.have_cpu) { F.cpu = a; F.have_cpu = true; }
		if (t == HSA_DEVICE_TYPE_GPU && !F.have_gpu) {
			uint32_t b = 0, d = 0;
			if (F.info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &b) == HSA_STATUS_SUCCESS && F.info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &d) == HSA_STATUS_SUCCESS && b == F.want_bdf && d == F.want_dom) {
				F.gpu = a; F.have_gpu = true;
			}
		}
		return HSA_STATUS_SUCCESS;
	}, &F);
	if (!F.have_gpu || !F.have_cpu) return;
	// candidates per direction: the engines the runtime prefers for it, then the others among the four lowest it reports (the ones beside the PCIe root on this chip; an older
	// runtime - the one a PyTorch wheel carries - names no preference at all)
	auto candidates = [&](hsa_agent_t dst, hsa_agent_t src, LinkCopy::Dir &D) {
		uint32_t pref = 0, avail = 0;
		if (f_pref(dst, src, &pref) != HSA_STATUS_SUCCESS) pref = 0;
		if (f_stat(dst, src, &avail) != HSA_STATUS_SUCCESS) avail = 0;
		for (int pass = 0; pass < 2; ++pass)
			for (uint32_t b = 0; b < 16; ++b) {
				const uint32_t bit = 1u << b;
				const bool take = pass == 0 ? (pref & bit) != 0 : (!(pref & bit) && (avail & bit) && b < 4);
				if (take) { D.cand.push_back(bit); D.rate.push_back(0.0); }
			}
	};
	L.gpu = F.gpu; L.cpu = F.cpu;
	candidates(F.cpu, F.gpu, L.to_host);
	candidates(F.gpu, F.cpu, L.to_device);
	if (L.to_host.cand.empty() || L.to_device.cand.empty()) return;
	if (L.to_host.cand.size() > 1 && L.to_host.cand[0] == L.to_device.cand[0]) L.to_host.cur = 1; // the two directions start on engines of their own (both run at once: tables out, chunks in)
	L.eng_to_host = L.to_host.cand[L.to_host.cur]; L.eng_to_device = L.to_device.cand[L.to_device.cur];
	{ // timestamps of the copies (the runtime's own profiling of async copies): without them the engines stay where they start
		auto f_prof = reinterpret_cast<decltype(&hsa_amd_profiling_async_copy_enable)>(sym("hsa_amd_profiling_async_copy_enable"));
		auto f_sys = reinterpret_cast<decltype(&hsa_system_get_info)>(sym("hsa_system_get_info"));
		L.copy_time = reinterpret_cast<decltype(L.copy_time)>(sym("hsa_amd_profiling_get_async_copy_time"));
		uint64_t hz = 0;
		if (f_prof && f_sys && L.copy_time && f_prof(true) == HSA_STATUS_SUCCESS && f_sys(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &hz) == HSA_STATUS_SUCCESS && hz) L.ticks_per_s = (double)hz;
		else L.copy_time = nullptr;
	}
	L.ok = true;
	if (getenv("SSV_TIMING")) fprintf(stderr, "[timing] (host link: SDMA engines by name - to the host 0x%x of %zu candidates, to the device 0x%x of %zu%s)\n", L.eng_to_host, L.to_host.cand.size(), L.eng_to_device,
	                                  L.to_device.cand.size(), L.copy_time ? ", copies timed" : "");
}

// one copy on the direction's engine; `sig` loses one when it has landed.  false: not done (the caller copies the runtime's way)
static bool link_copy(ssv_ctx *c, void *dst, const void *src, size_t bytes, bool to_host, hsa_signal_t sig)
{
	const LinkCopy &L = c->link;
	if (!L.ok || !bytes) return false;
	return L.copy_on_engine(dst, to_host ? L.cpu : L.gpu, src, to_host ? L.gpu : L.cpu, bytes, 0, nullptr, sig, (hsa_amd_sdma_engine_id_t)(to_host ? L.eng_to_host : L.eng_to_device), true) == HSA_STATUS_SUCCESS;
}

// is [p, p + bytes) page-locked host memory the runtime knows (hipHostMalloc, hipHostRegister)?  Only such memory may be handed to an SDMA engine by address
static bool link_host_ok(const void *p)
{
	hipPointerAttribute_t a;
	memset(&a, 0, sizeof(a));
	if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
	return a.type == hipMemoryTypeHost;
}

static void link_wait(ssv_ctx *c, hsa_signal_t sig)
{
	while (c->link.signal_wait(sig, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED) >= 1) {}
}

// a large copy has landed (its own signal: `sig`): what rate did its engine give, and should the direction move on?
static void link_timed(ssv_ctx *c, hsa_signal_t sig, size_t bytes, bool to_host)
{
	LinkCopy &L = c->link;
	if (!L.copy_time || bytes < ((size_t)8 << 20)) return;
	hsa_amd_profiling_async_copy_time_t t{};
	if (L.copy_time(sig, &t) != HSA_STATUS_SUCCESS || t.end <= t.start) return;
	LinkCopy::Dir &D = to_host ? L.to_host : L.to_device;
	const double rate = (double)bytes / ((double)(t.end - t.start) / L.ticks_per_s) / 1e9;
	D.rate[D.cur] = rate;
	double best = 0;
	for (double r : D.rate) best = std::max(best, r);
	if (rate >= 0.85 * best && rate >= 40.0) return; // (a PCIe Gen5 x16 link gives 55-57 GB/s)
	// well below what this direction has seen (or what the link should give): an engine not tried yet, else the one whose last copy was the fastest
	size_t next = D.cur;
	for (size_t k = 0; k < D.cand.size(); ++k) if (D.rate[k] == 0.0) { next = k; break; }
	if (next == D.cur) for (size_t k = 0; k < D.cand.size(); ++k) if (D.rate[k] > D.rate[next]) next = k;
	if (next != D.cur) {
		if (getenv("SSV_TIMING")) fprintf(stderr, "[timing] (host link: %s at %.1f GB/s on engine 0x%x: on to engine 0x%x)\n", to_host ? "to the host" : "to the device", rate, D.cand[D.cur], D.cand[next]);
		D.cur = next;
		(to_host ? L.eng_to_host : L.eng_to_device) = D.cand[next];
	} else if (best > rate) D.rate[D.cur] = rate; // (everything is slow right now: stay, and let the stale best rates of the others age)
	for (size_t k = 0; k < D.cand.size(); ++k) if (k != D.cur && D.rate[k] > 0.0) D.rate[k] = std::max(rate, D.rate[k] * 0.9); // (what an engine gave a while ago counts for less and less)
}


int ensure_host(ssv_ctx *c, HBuf &b, size_t bytes)
{
	if (bytes <= b.cap) return SSV_OK;
	size_t ncap = (std::max(bytes, b.cap + b.cap / 2) + 255) & ~(size_t)255;
	HIPCHECK(c, b.release());
	HIPCHECK(c, pinned_new(&b.p, ncap, hipHostMallocDefault));
	b.cap = ncap;
	return SSV_OK;
}

// `bytes` of device memory that stay where they are until the arena is rewound
int arena_alloc(ssv_ctx *c, Arena &a, size_t bytes, void **out)
{
	bytes = (bytes + 255) & ~(size_t)255;
	while (a.cur < a.chunks.size() && a.chunks[a.cur].cap - a.used < bytes) { ++a.cur; a.used = 0; }
	if (a.cur == a.chunks.size()) {
		DBuf b;
		const size_t cap = std::max<size_t>(bytes, (size_t)64 << 20);
		HIPCHECK(c, dev_malloc(c, &b.p, cap));
		b.cap = cap;
		a.chunks.push_back(std::move(b));
		a.used = 0;
	}
	*out = reinterpret_cast<uint8_t *>(a.chunks[a.cur].p) + a.used;
	a.used += bytes;
	return SSV_OK;
}

template <typename T> T *P(DBuf &b) { return reinterpret_cast<T *>(b.p); }
template <typename T> T *P(HBuf &b) { return reinterpret_cast<T *>(b.p); }

// a buffer's size when the call sizes everything for a chunk `grow` times as large as the one at hand (ssv_bamdec_expect; 1: as it is)
inline size_t grown(size_t bytes, double grow) { return grow > 1.0 ? (size_t)((double)bytes * grow) + 64 : bytes; }

// The device buffers of the columns both decoders write (ssv_bamdec_decode, ssv_samdec_decode): one per column of the table, and seq_bytes.
struct DecodedColumns {
	DBuf col[COL_COUNT], seq_bytes;
	int reserve(ssv_ctx *c, size_t n, double grow) // the per-record columns
	{
		for (int k = 0; k < COL_COUNT; ++k) if (kBatchCols[k].len == LEN_N) CHECK(ensure(c, col[k], grown(n * kBatchCols[k].elem + 16, grow)));
		return ensure(c, seq_bytes, grown(n * 4 + 16, grow));
	}
	int reserve_variable(ssv_ctx *c, size_t cigar_total, size_t seq_total, double grow) // the operations, the bases + qualities: once layout()'s totals are known
	{
		CHECK(ensure(c, col[COL_cigar], grown(cigar_total * 4 + 64, grow)));
		return ensure(c, col[COL_seqqual], grown(seq_total + 64, grow));
	}
	DecodedCols view()
	{
		DecodedCols v;
#define X(member, ...) v.member = static_cast<decltype(v.member)>(col[COL_##member].p);
		SSV_BATCH_COLUMNS(X)
#undef X
		v.seq_bytes = P<uint32_t>(seq_bytes);
		return v;
	}
	// n_cigar -> cigar_off, seq_bytes -> seq_off; the totals go to device memory of the caller's, read back with the rest of its small block
	void layout(hipStream_t st, int64_t n, uint32_t *scratch32, uint64_t *scratch64, uint32_t *cigar_total, uint64_t *seq_total)
	{
		const DecodedCols v = view();
		exclusive_scan<uint16_t, uint32_t>(st, v.n_cigar, v.cigar_off, n, 0u, scratch32, cigar_total);
		exclusive_scan<uint32_t, uint64_t>(st, v.seq_bytes, v.seq_off, n, 0ull, scratch64, seq_total);
	}
	void fill(ssv_batch_t *out, int64_t n, int64_t cigar_total, int64_t seq_total) // the batch handed out (max_ref_span, rec, tid_runs: the caller's)
	{
		out->n = n; out->n_cigar_total = cigar_total; out->seqqual_bytes = seq_total;
		for (int k = 0; k < COL_COUNT; ++k) col_set(*out, k, col[k].p);
	}
};

// The contig lists of a decoded chunk, for both decoders (ssv_bamdec_decode, ssv_samdec_decode in its mode for sorted originals): the changes of contig among
// the records that are not UNMAP|MUNMAP (ssv_bamdec_info.tid_run_*: getclip's flush sequence) and the tid column as runs (ssv_batch_t.tid_runs).
struct TidLists {
	static constexpr uint32_t RUN_CAP = 1u << 16, RAW_RUN_CAP = 64;
	DBuf tile_last, tile_prev, runs, raw_runs;
	HBuf h_raw_runs, h_runs;
	std::vector<ssv_tid_run> tid_runs;
	int reserve(ssv_ctx *c, int64_t n, double grow)
	{
		const size_t n_tiles = (size_t)((n + BLOCK - 1) / BLOCK);
		CHECK(ensure(c, tile_last, grown(n_tiles * 4, grow))); CHECK(ensure(c, tile_prev, grown(n_tiles * 4, grow)));
		CHECK(ensure(c, runs, grown((size_t)RUN_CAP * sizeof(ssv::TidRun), grow)));
		CHECK(ensure(c, raw_runs, grown((size_t)RAW_RUN_CAP * sizeof(ssv::TidRun), grow)));
		return ensure_host(c, h_raw_runs, (size_t)RAW_RUN_CAP * sizeof(ssv::TidRun));
	}
	// the four kernels over the decoded tid / flag columns; the counts and the last contig go to device words of the caller's (zeroed by it), read back with its small block
	int launch(ssv_ctx *c, hipStream_t st, const int32_t *tid, const uint16_t *flag, int64_t n, int32_t prev_tid, uint32_t *n_runs, int32_t *last_tid, uint32_t *n_raw_runs)
	{
		const int64_t n_tiles = (n + BLOCK - 1) / BLOCK;
		hipLaunchKernelGGL(ssv::k_tid_tile_last, dim3((unsigned)n_tiles), dim3(BLOCK), 0, st, tid, flag, n, P<int32_t>(tile_last));
		hipLaunchKernelGGL(ssv::k_tid_tile_carry, dim3(1), dim3(WAVE), 0, st, P<int32_t>(tile_last), n_tiles, prev_tid, P<int32_t>(tile_prev), last_tid);
		hipLaunchKernelGGL(ssv::k_tid_runs, dim3((unsigned)n_tiles), dim3(BLOCK), 0, st, tid, flag, n, P<int32_t>(tile_prev), P<ssv::TidRun>(runs), RUN_CAP, n_runs);
		hipLaunchKernelGGL(ssv::k_tid_raw_runs, dim3((unsigned)n_tiles), dim3(BLOCK), 0, st, tid, n, P<ssv::TidRun>(raw_runs), RAW_RUN_CAP, n_raw_runs);
		HIPCHECK(c, hipMemcpyAsync(h_raw_runs.p, raw_runs.p, (size_t)RAW_RUN_CAP * sizeof(ssv::TidRun), hipMemcpyDeviceToHost, st));
		return SSV_OK;
	}
	// once the caller has read n_runs (<= RUN_CAP): the changes on their way to the host (the caller synchronises when n_runs > 0)
	int fetch(ssv_ctx *c, hipStream_t st, uint32_t n_runs)
	{
		CHECK(ensure_host(c, h_runs, (size_t)n_runs * sizeof(ssv::TidRun) + 64 + (size_t)n_runs * 8));
		if (n_runs) HIPCHECK(c, hipMemcpyAsync(h_runs.p, runs.p, (size_t)n_runs * sizeof(ssv::TidRun), hipMemcpyDeviceToHost, st));
		return SSV_OK;
	}
	// atomics gave the runs no order: sort by record index, then split into the two arrays of the info struct (behind the pairs)
	void changes(uint32_t n_runs, ssv_bamdec_info &info)
	{
		ssv::TidRun *r = P<ssv::TidRun>(h_runs);
		std::sort(r, r + n_runs, [](const ssv::TidRun &a, const ssv::TidRun &b) { return a.index < b.index; });
		uint32_t *idx = reinterpret_cast<uint32_t *>(P<uint8_t>(h_runs) + (((size_t)n_runs * sizeof(ssv::TidRun) + 63) & ~(size_t)63));
		int32_t *tv = reinterpret_cast<int32_t *>(idx + n_runs);
		for (uint32_t k = 0; k < n_runs; ++k) { idx[k] = r[k].index; tv[k] = r[k].tid; }
		info.n_tid_runs = n_runs; info.tid_run_index = idx; info.tid_run_tid = tv;
	}
	// the tid column as runs (sorted by record index); more than the list holds: not handed out
	void batch_runs(uint32_t nr, ssv_batch_t *out)
	{
		tid_runs.clear();
		if (nr < 1 || nr > RAW_RUN_CAP) return;
		const ssv::TidRun *r = P<ssv::TidRun>(h_raw_runs);
		for (uint32_t k = 0; k < nr; ++k) tid_runs.push_back(ssv_tid_run{(int64_t)r[k].index, r[k].tid, 0});
		std::sort(tid_runs.begin(), tid_runs.end(), [](const ssv_tid_run &a, const ssv_tid_run &b) { return a.first < b.first; });
		out->tid_runs = tid_runs.data(); out->n_tid_runs = (int64_t)nr;
	}
};

// The one set of rules for an ssv_names_t argument (`what`: the entry point, for the message): a batch with records needs its names, and names that are
// given say where they lie.
int check_names(ssv_ctx *c, const ssv_names_t *nm, int64_t n, const char *what)
{
	const char *bad = nullptr;
	if (n > 0 && (!nm || !nm->base || !nm->off)) bad = "a batch with records needs their names";
	else if (nm && nm->mem != SSV_MEM_HOST && nm->mem != SSV_MEM_DEVICE) bad = "bad names.mem";
	else if (nm && nm->bias < 0) bad = "names.bias below 0";
	else if (nm && nm->mem == SSV_MEM_HOST && nm->bytes < 0) bad = "names.bytes below 0";
	if (!bad) return SSV_OK;
	c->err = std::string(what) + ": " + bad;
	return SSV_E_ARG;
}

// The names of a batch of n > 0 records where the kernels read them: device names in place; host names copied into `blob` and `off` on c->st, 16 zero
// bytes behind the blob (a name without its NUL ends there).
int stage_names(ssv_ctx *c, const ssv_names_t *nm, int64_t n, DBuf &blob, DBuf &off, DevNames &out)
{
	if (nm->mem == SSV_MEM_DEVICE) { out = DevNames{nm->base, nm->off, nm->bias}; return SSV_OK; }
	CHECK(ensure(c, blob, (size_t)nm->bytes + 16)); CHECK(ensure(c, off, (size_t)n * 8 + 16));
	if (nm->bytes) HIPCHECK(c, hipMemcpyAsync(blob.p, nm->base, (size_t)nm->bytes, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemsetAsync(P<char>(blob) + nm->bytes, 0, 16, c->st));
	HIPCHECK(c, hipMemcpyAsync(off.p, nm->off, (size_t)n * 8, hipMemcpyHostToDevice, c->st));
	out = DevNames{P<char>(blob), P<uint64_t>(off), nm->bias};
	return SSV_OK;
}

struct ProfScope {
	ssv_ctx *c;
	int id;
	bool on;
	hipEvent_t a{}, b{};
	int64_t units;
	ProfScope(ssv_ctx *ctx, int id_, int64_t units_) : c(ctx), id(id_), units(units_)
	{
		on = c->prof_mode == 1 || (c->prof_mode == 2 && (id == P_CLIP_SCAN || id == P_GETSV_SCAN));
		if (!on) return;
		for (hipEvent_t *e : {&a, &b}) {
			if (!c->prof_pool.empty()) { *e = c->prof_pool.back(); c->prof_pool.pop_back(); }
			else if (hipEventCreate(e) != hipSuccess) { on = false; return; }
		}
		(void)hipEventRecord(a, c->st);
	}
	~ProfScope()
	{
		if (!on) return;
		(void)hipEventRecord(b, c->st);
		c->prof_recs.push_back({id, a, b, units});
	}
};

void prof_collect(ssv_ctx *c)
{
	if (c->prof_recs.empty()) return;
	(void)hipStreamSynchronize(c->st);
	for (ProfRec &r : c->prof_recs) {
		float ms = 0;
		if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
			c->prof_ms[r.id] += ms; c->prof_launches[r.id] += 1; c->prof_units[r.id] += r.units;
		}
		c->prof_pool.push_back(r.a); c->prof_pool.push_back(r.b);
	}
	c->prof_recs.clear();
}

// persistent streaming kernels: the grid is the number of workgroups that are resident at once (a larger grid queues the surplus
// behind the first wave of workgroups and stretches the kernel).  clip_scan: 106 SGPRs -> 6 workgroups of 256 threads per CU;
// getsv_scan: 104 VGPRs (software-pipelined loads) -> 4 per CU.  Overrides for experiments: SSV_CLIP_SCAN_BLOCKS, SSV_GETSV_SCAN_BLOCKS.
inline unsigned scan_blocks(int64_t ntiles, const char *env, int64_t dflt)
{
	const char *e = getenv(env);
	int64_t cfg = e ? atoll(e) : dflt;
	return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ntiles, std::min<int64_t>(cfg, CS_MAX_BLOCKS)));
}

inline unsigned grid_for(int64_t n, int per_block) { return (unsigned)std::max<int64_t>(1, (n + per_block - 1) / per_block); }

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool aligned64(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 63) == 0; }

// Copies of a host batch into staging set `set`, issued on `st`: with `rec` the batch ships lines + hot columns + variable parts; without,
// the classic columns (the lines are then built on the device, k_build_rec).
static int upload_host_batch(ssv_ctx *c, const ssv_batch_t *b, int set, hipStream_t st)
{
	const size_t n = (size_t)b->n;
	ssv_ctx::StageSet &S = c->ss[set];
	for (int k = 0; k < COL_COUNT; ++k) {
		const void *src = b->rec && kBatchCols[k].in_rec ? nullptr : col_get(*b, k);
		if (!src) { if (kBatchCols[k].never_empty) CHECK(ensure(c, S.col[k], 16)); continue; }
		const size_t bytes = col_bytes(*b, k);
		CHECK(ensure(c, S.col[k], bytes + 16));
		if (bytes) HIPCHECK(c, hipMemcpyAsync(S.col[k].p, src, bytes, hipMemcpyHostToDevice, st));
	}
	CHECK(ensure(c, S.rec, n * sizeof(ssv_record) + 64));
	if (b->rec && n) HIPCHECK(c, hipMemcpyAsync(S.rec.p, b->rec, n * sizeof(ssv_record), hipMemcpyHostToDevice, st));
	return SSV_OK;
}

// k_build_rec's source out of any set of column base pointers: at(COL_x) -> where column x lies
template <typename At> static SoaCols soa_cols(At at)
{
	SoaCols s;
#define X(member, ...) s.member = static_cast<decltype(s.member)>(at(COL_##member));
	SSV_BATCH_COLUMNS(X)
#undef X
	return s;
}

// the device view of a host batch staged in set `set` (a column that may be NULL is NULL here when the batch came without it)
static void staged_view(ssv_ctx *c, const ssv_batch_t *b, int set, DevBatch &d, SoaCols &s)
{
	ssv_ctx::StageSet &S = c->ss[set];
	s = soa_cols([&](int k) -> const void * { return kBatchCols[k].nullable && !col_get(*b, k) ? nullptr : S.col[k].p; });
	d.tid = s.tid; d.pos = s.pos; d.n_cigar = s.n_cigar; d.cigar = s.cigar; d.seqqual = s.seqqual; d.ends = s.cigar_ends;
	d.rec = P<ssv_record>(S.rec);
}

static int check_batch(ssv_ctx *c, const ssv_batch_t *b)
{
	if (!b || b->n < 0 || b->n >= (1ll << 31)) { c->err = "bad batch"; return SSV_E_ARG; }
	bool complete = true; // the per-record columns that must be there: all but the nullable ones, or with `rec` those it does not stand in for
	for (int k = 0; k < COL_COUNT; ++k)
		if (kBatchCols[k].len == LEN_N && !kBatchCols[k].nullable && !(b->rec && kBatchCols[k].in_rec) && !col_get(*b, k)) complete = false;
	if (b->n > 0 && !complete) { c->err = "batch with null arrays"; return SSV_E_ARG; }
	const int mem = b->mem & ~(int)SSV_MEM_PERSISTENT;
	if (mem != SSV_MEM_DEVICE && b->mem != SSV_MEM_HOST) { c->err = "bad batch.mem"; return SSV_E_ARG; }
	return SSV_OK;
}

// Make the batch visible to the kernels: device batches are used in place, host batches are copied to HBM (or were, ssv_batch_prefetch); a
// batch that comes as structure-of-arrays columns only is transposed into record lines (ssv_record) on the device.
int stage_batch(ssv_ctx *c, const ssv_batch_t *b, DevBatch &d, bool keep_announced = false)
{
	CHECK(check_batch(c, b));
	d.n = b->n; d.max_ref_span = b->max_ref_span;
	const size_t n = (size_t)b->n;
	SoaCols s{};
	ssv_record *rec_dst = nullptr;
	if ((b->mem & ~(int)SSV_MEM_PERSISTENT) == SSV_MEM_DEVICE) {
		if (!aligned16(b->tid) || !aligned16(b->pos) || !aligned16(b->n_cigar) || (b->rec && !aligned64(b->rec))) {
			c->err = "device batch arrays must be 16-byte aligned (rec: 64-byte aligned)"; return SSV_E_ARG;
		}
		if (b->cigar_ends && !aligned16(b->cigar_ends)) { c->err = "device batch arrays must be 16-byte aligned (rec: 64-byte aligned)"; return SSV_E_ARG; }
		d.tid = b->tid; d.pos = b->pos; d.n_cigar = b->n_cigar; d.cigar = b->cigar; d.seqqual = b->seqqual; d.rec = b->rec; d.ends = b->cigar_ends;
		if (d.rec || n == 0) return SSV_OK;
		s = soa_cols([&](int k) { return col_get(*b, k); });
		CHECK(ensure(c, c->ss[2].rec, n * sizeof(ssv_record) + 64));
		rec_dst = P<ssv_record>(c->ss[2].rec);
	} else {
		if (!c->pf.empty()) {
			// announced batches are consumed in the order they were announced
			const ssv_ctx::Prefetched f = c->pf.front();
			if (memcmp(&f.b, b, sizeof(*b)) != 0) { c->err = "a prefetched batch is pending: the next scan call must be given that batch"; return SSV_E_STATE; }
			if (!keep_announced) c->pf.pop_front(); // (a scan of a leading part of the batch leaves it staged for the scan of the rest)
			staged_view(c, b, f.set, d, s);
			HIPCHECK(c, hipEventSynchronize(c->ss[f.set].ready)); // the caller may recycle the host arrays once the scan call returns
		} else {
			ProfScope ps(c, P_H2D, b->n);
			CHECK(upload_host_batch(c, b, 2, c->st));
			staged_view(c, b, 2, d, s);
			HIPCHECK(c, hipStreamSynchronize(c->st)); // same promise (copies from pinned host arrays are asynchronous)
		}
		if (b->rec || n == 0) return SSV_OK;
		rec_dst = const_cast<ssv_record *>(d.rec);
	}
	k_build_rec<<<grid_for(b->n, BLOCK), BLOCK, 0, c->st>>>(s, b->n, rec_dst);
	HIPCHECK(c, hipGetLastError());
	d.rec = rec_dst;
	return SSV_OK;
}

// `need` bytes (a multiple of 256: every batch starts 256-byte aligned) for a batch that stays (RetainedSlab below, for ssv_batch_retain, ssv_dup_retain,
// ssv_pairdup_retain and ssv_batch_sort): room in the newest arena, or a new one - 256 MB first, doubling up to SSV_RETAIN_ARENA_MB (4 GB), never smaller than
// the batch.  The arena counts the slab as live; a caller that fails afterwards takes it back (retain_slab_undo).
int retain_slab(ssv_ctx *c, size_t need, ssv_ctx::RetainArena **arena_out, uint8_t **slab)
{
	ssv_ctx::RetainArena *arena = nullptr;
	if (!c->arenas.empty() && c->arenas.back().cap - c->arenas.back().used >= need) arena = &c->arenas.back();
	else {
		static const size_t arena_max = []() { const char *e = getenv("SSV_RETAIN_ARENA_MB"); return (size_t)(e ? atoll(e) : 4096) << 20; }();
		size_t cap = c->arenas.empty() ? std::min(arena_max, (size_t)256 << 20) : std::min(arena_max, c->arenas.back().cap * 2);
		if (cap < need) cap = need;
		ssv_ctx::RetainArena a;
		// a spare one that is large enough (the smallest such), else a new one
		size_t pick = c->spare_arenas.size();
		for (size_t k = 0; k < c->spare_arenas.size(); ++k)
			if (c->spare_arenas[k].cap >= need && (pick == c->spare_arenas.size() || c->spare_arenas[k].cap < c->spare_arenas[pick].cap)) pick = k;
		if (pick < c->spare_arenas.size()) { a.base = c->spare_arenas[pick].base; cap = c->spare_arenas[pick].cap; c->spare_arenas.erase(c->spare_arenas.begin() + (long)pick); }
		else {
			size_t acap = 0;
			if (uint8_t *b = arena_ahead_take(c, &acap)) { // the one asked for ahead - if this batch fits (else it waits among the spares)
				if (acap >= need) { a.base = b; cap = acap; }
				else c->spare_arenas.push_back({b, acap});
			}
			if (!a.base) HIPCHECK(c, dev_malloc(c, reinterpret_cast<void **>(&a.base), cap));
		}
		a.cap = cap;
		c->arenas.push_back(a);
		arena = &c->arenas.back();
		// the next one, while this one fills (not when spares are waiting: a context that has been through a release has its memory)
		if (c->spare_arenas.empty()) arena_ahead_start(c, std::min(arena_max, cap * 2));
	}
	*slab = arena->base + arena->used;
	arena->slabs.push_back(arena->used);
	arena->used += need; ++arena->live;
	*arena_out = arena;
	return SSV_OK;
}
inline void retain_slab_undo(ssv_ctx::RetainArena *arena, size_t need) { --arena->live; arena->used -= need; arena->slabs.pop_back(); }

// The retained form, stated once: seven parts in one slab, each 256-byte aligned - tid, pos, n_cigar, cigar_ends, the lines, the operations, the
// bases + qualities - and behind them `extra` bytes of the producer's own (ssv_pairdup_retain's rows).  The object holds the slab, and a host copy of tid_runs
// when it was given one, and gives both back when it goes - unless the batch was handed out.
struct RetainedSlab {
	size_t n, cigar_total, seq_bytes;
	size_t off[9]; // off[7]: where the extra bytes begin, off[8]: the slab's size
	ssv_ctx::RetainArena *arena = nullptr;
	uint8_t *slab = nullptr;
	ssv_tid_run *runs = nullptr;
	int64_t n_runs = 0;
	bool handed_out = false;
	RetainedSlab(size_t n_, size_t cigar_total_, size_t seq_bytes_, size_t extra = 0) : n(n_), cigar_total(cigar_total_), seq_bytes(seq_bytes_)
	{
		const size_t sz[8] = {n * 4 + 16, n * 4 + 16, n * 2 + 16, n + 16, n * sizeof(ssv_record) + 64, cigar_total * 4 + 64, seq_bytes + 64, extra};
		off[0] = 0;
		for (int k = 0; k < 8; ++k) off[k + 1] = off[k] + ((sz[k] + 255) & ~(size_t)255);
	}
	RetainedSlab(const RetainedSlab &) = delete;
	RetainedSlab &operator=(const RetainedSlab &) = delete;
	~RetainedSlab() { if (!handed_out) { if (arena) retain_slab_undo(arena, off[8]); free(runs); } }
	int take(ssv_ctx *c) { return retain_slab(c, off[8], &arena, &slab); }
	// room for a host copy of the tid column as `count` runs, which lives as long as the batch (NULL: none to be had, the error is set)
	ssv_tid_run *new_runs(ssv_ctx *c, int64_t count)
	{
		runs = static_cast<ssv_tid_run *>(malloc((size_t)count * sizeof(ssv_tid_run)));
		if (!runs) c->err = "out of host memory (tid_runs)";
		else n_runs = count;
		return runs;
	}
	int copy_runs(ssv_ctx *c, const ssv_batch_t *b) // the runs of a batch that has them
	{
		if (!b->tid_runs || b->n_tid_runs <= 0) return SSV_OK;
		if (!new_runs(c, b->n_tid_runs)) return SSV_E_NOMEM;
		memcpy(runs, b->tid_runs, (size_t)b->n_tid_runs * sizeof(ssv_tid_run));
		return SSV_OK;
	}
	template <typename T> T *part(int k) const { return reinterpret_cast<T *>(slab + off[k]); }
	RetDst dst() const { return RetDst{part<int32_t>(0), part<int32_t>(1), part<uint16_t>(2), part<uint8_t>(3), part<ssv_record>(4), part<uint32_t>(5), part<uint8_t>(6)}; }
	// the batch as its owner sees it; from here on the slab and the runs are the batch's (ssv_batch_release)
	void hand_out(ssv_batch_t *out, int32_t max_ref_span)
	{
		const RetDst d = dst();
		handed_out = true;
		memset(out, 0, sizeof(*out));
		out->n = (int64_t)n; out->mem = SSV_MEM_DEVICE | SSV_MEM_PERSISTENT; out->max_ref_span = max_ref_span;
		out->tid = d.tid; out->pos = d.pos; out->n_cigar = d.n_cigar; out->cigar_ends = d.ends; out->rec = d.rec; out->cigar = d.cigar; out->seqqual = d.seqqual;
		out->n_cigar_total = (int64_t)cigar_total; out->seqqual_bytes = (int64_t)seq_bytes;
		if (runs) { out->tid_runs = runs; out->n_tid_runs = n_runs; }
	}
};

// a staged batch that came without its cigar_ends column: built from the lines into the context's buffer
int staged_ends(ssv_ctx *c, DevBatch &d)
{
	if (d.ends || d.n == 0) return SSV_OK;
	CHECK(ensure(c, c->ends_buf, (size_t)d.n + 16));
	k_build_ends<<<grid_for(d.n, BLOCK), BLOCK, 0, c->st>>>(d, P<uint8_t>(c->ends_buf));
	HIPCHECK(c, hipGetLastError());
	d.ends = P<uint8_t>(c->ends_buf);
	return SSV_OK;
}

// A small block of device words that a call's kernels and scans leave their counts in, and its pinned host copy.  What the words mean, and how many
// bytes they take, is the stage's.
struct SmallWords {
	DBuf dev;
	HBuf host;
	size_t bytes = 0;
	int reserve(ssv_ctx *c, size_t bytes_) { bytes = bytes_; CHECK(ensure(c, dev, bytes)); return ensure_host(c, host, bytes); }
	int clear(ssv_ctx *c) { HIPCHECK(c, hipMemsetAsync(dev.p, 0, bytes, c->st)); return SSV_OK; }
	int fetch(ssv_ctx *c) // the host copy is current, and everything on the stream before it is done
	{
		HIPCHECK(c, hipMemcpyAsync(host.p, dev.p, bytes, hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
		return SSV_OK;
	}
};

// (tests) an environment variable that cuts a 64-bit hash to its low bits, so that hashes collide: the mask, and how many bits it keeps
uint64_t env_low_bits_mask(const char *name, int *bits_out = nullptr)
{
	const char *e = getenv(name);
	const int bits = e ? std::max(1, std::min(64, atoi(e))) : 64;
	if (bits_out) *bits_out = bits;
	return bits == 64 ? ~0ull : ((1ull << bits) - 1);
}

__global__ void k_max_span(DevBatch b, int *out)
{
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	int span = 0;
	if (i < b.n) {
		const RecLine r = rec_load(b.rec, i);
		const int n = r.n_cigar();
		long long s = 0;
		for (int k = 0; k < n; ++k) { uint32_t x = r.op(b.cigar, k); int op = (int)(x & 15u); if (op == C_M || op == C_D || op == C_N || op == C_EQ || op == C_X) s += x >> 4; }
		span = s > 0x7fffffff ? 0x7fffffff : (int)s;
	}
	span = wave_max(span);
	if (lane_id() == 0 && span > 0 && span > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, span); // (look first: one address, a wavefront each)
}

} // namespace


// the three oldest stages: state struct + C ABI each (the ssv_* names have C linkage from include/seeksv_hip.h)
#include "clip_api.inc"
#include "probe_api.inc"
#include "isize_api.inc"
#include "getsv_api.inc"

// =====================================================================================================================
extern "C" {

int ssv_abi_version(void) { return SSV_ABI_VERSION; }

int ssv_device_count(void)
{
	int n = 0;
	return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int ssv_sync(ssv_ctx *c)
{
	if (!c) return SSV_E_ARG;
	HIPCHECK(c, hipStreamSynchronize(c->st));
	return SSV_OK;
}

int ssv_host_alloc(size_t bytes, void **p)
{
	if (!p) return SSV_E_ARG;
	*p = nullptr;
	hipError_t e = pinned_new(p, bytes ? bytes : 1, hipHostMallocPortable);
	if (e != hipSuccess) { g_create_error = std::string("page-locked allocation: ") + hipGetErrorString(e); *p = nullptr; return SSV_E_NOMEM; }
	return SSV_OK;
}

int ssv_host_free(void *p)
{
	if (p && pinned_delete(p) != hipSuccess) return SSV_E_HIP;
	return SSV_OK;
}

int ssv_host_register(void *p, size_t bytes)
{
	if (!p || !bytes) return SSV_E_ARG;
	const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
	if (e != hipSuccess) { (void)hipGetLastError(); g_create_error = std::string("hipHostRegister: ") + hipGetErrorString(e); return SSV_E_HIP; }
	return SSV_OK;
}

int ssv_host_bind_near(void *p, size_t bytes, int device)
{
	bind_near(p, bytes, device);
	return SSV_OK;
}

int ssv_host_unregister(void *p)
{
	if (p && hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return SSV_E_HIP; }
	return SSV_OK;
}

int ssv_batch_prefetch(ssv_ctx *c, const ssv_batch_t *b)
{
	if (!c || !b) return SSV_E_ARG;
	CHECK(check_batch(c, b));
	if (b->mem != SSV_MEM_HOST) { c->err = "ssv_batch_prefetch takes host batches"; return SSV_E_ARG; }
	if (c->pf.size() >= 2) { c->err = "two prefetched batches are pending already"; return SSV_E_STATE; }
	HIPCHECK(c, hipSetDevice(c->device));
	const int set = (int)(c->pf_count & 1);
	// the set was last read by the kernels of the batch two announcements ago, all of them launched on st by now
	HIPCHECK(c, hipEventRecord(c->ev_st, c->st));
	HIPCHECK(c, hipStreamWaitEvent(c->st_h2d, c->ev_st, 0));
	CHECK(upload_host_batch(c, b, set, c->st_h2d));
	HIPCHECK(c, hipEventRecord(c->ss[set].ready, c->st_h2d));
	c->pf.push_back(ssv_ctx::Prefetched{*b, set});
	++c->pf_count;
	return SSV_OK;
}

int ssv_batch_prefetch_drop(ssv_ctx *c)
{
	if (!c) return SSV_E_ARG;
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->pf.empty()) HIPCHECK(c, hipStreamSynchronize(c->st_h2d)); // their host arrays are the caller's again when this returns
	c->pf.clear();
	return SSV_OK;
}

const char *ssv_last_error(const ssv_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }
void *ssv_stream(ssv_ctx *c) { return c ? (void *)c->st : nullptr; }

// test/debug helper: a device batch as a host batch (arrays owned by the context, valid until the next call)
int ssv_batch_to_host(ssv_ctx *c, const ssv_batch_t *dev, ssv_batch_t *host)
{
	if (!c || !dev || !host || dev->mem != SSV_MEM_DEVICE) return SSV_E_ARG;
	size_t off[COL_COUNT + 1]; off[0] = 0; // every column 64-byte aligned
	for (int k = 0; k < COL_COUNT; ++k) off[k + 1] = off[k] + ((col_bytes(*dev, k) + 63) & ~(size_t)63);
	CHECK(ensure_host(c, c->h_batch, off[COL_COUNT] + 64));
	uint8_t *base = P<uint8_t>(c->h_batch);
	for (int k = 0; k < COL_COUNT; ++k) {
		const void *src = col_get(*dev, k);
		if (src && col_bytes(*dev, k)) HIPCHECK(c, hipMemcpyAsync(base + off[k], src, col_bytes(*dev, k), hipMemcpyDeviceToHost, c->st));
	}
	HIPCHECK(c, hipStreamSynchronize(c->st));
	*host = *dev;
	host->mem = SSV_MEM_HOST;
	for (int k = 0; k < COL_COUNT; ++k) col_set(*host, k, kBatchCols[k].nullable && !col_get(*dev, k) ? nullptr : base + off[k]);
	host->rec = nullptr; // (the lines stay on the device: the host batch is the classic columns)
	return SSV_OK;
}

// ---- a batch kept: the decoded records of a file stay in HBM for the passes that follow ----
int ssv_batch_retain(ssv_ctx *c, const ssv_batch_t *b, ssv_batch_t *out)
{
	if (!c || !b || !out) return SSV_E_ARG;
	HIPCHECK(c, hipSetDevice(c->device));
	if ((b->mem & ~(int)SSV_MEM_PERSISTENT) != SSV_MEM_DEVICE) { c->err = "ssv_batch_retain takes device batches"; return SSV_E_ARG; } // (so no announced host batch is consumed below)
	DevBatch d;
	CHECK(stage_batch(c, b, d)); // (builds the record lines when the batch has none)
	const size_t n = (size_t)b->n;
	RetainedSlab R(n, (size_t)b->n_cigar_total, (size_t)b->seqqual_bytes);
	CHECK(R.copy_runs(c, b));
	static const bool timing = [] { const char *e = getenv("SSV_TIMING"); return e ? atoi(e) : 0; }() >= 2; // SSV_TIMING=2: per-chunk detail
	const auto t0 = std::chrono::steady_clock::now();
	CHECK(R.take(c));
	const auto t1 = std::chrono::steady_clock::now();
	const void *src[7] = {d.tid, d.pos, d.n_cigar, d.ends, d.rec, d.cigar, d.seqqual};
	const size_t bytes[7] = {n * 4, n * 4, n * 2, n, n * sizeof(ssv_record), R.cigar_total * 4, R.seq_bytes};
	if (!d.ends && n) { // no cigar_ends column: built from the lines, straight into the slab
		k_build_ends<<<grid_for(d.n, BLOCK), BLOCK, 0, c->st>>>(d, R.part<uint8_t>(3));
		HIPCHECK(c, hipGetLastError());
	}
	for (int k = 0; k < 7; ++k) if (src[k] && bytes[k]) HIPCHECK(c, hipMemcpyAsync(R.part<uint8_t>(k), src[k], bytes[k], hipMemcpyDeviceToDevice, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st)); // the source (the decoder's buffers) may be overwritten by the next decode
	if (timing) fprintf(stderr, "[timing] (retain: %lld records, %zu bytes: hipMalloc %.4f s, copies + wait %.4f s)\n", (long long)b->n, R.off[8], std::chrono::duration<double>(t1 - t0).count(),
	                    std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count());
	R.hand_out(out, b->max_ref_span);
	return SSV_OK;
}

int ssv_batch_release(ssv_ctx *c, ssv_batch_t *b)
{
	if (!c || !b) return SSV_E_ARG;
	if (b->mem != (SSV_MEM_DEVICE | SSV_MEM_PERSISTENT) || !b->tid) { c->err = "not a batch of ssv_batch_retain"; return SSV_E_ARG; }
	HIPCHECK(c, hipSetDevice(c->device));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	{ // the batch's arena (the slab starts with the tid column): given back to the device when its last batch goes, unless it is the newest one - that one starts over
		const uint8_t *at = reinterpret_cast<const uint8_t *>(b->tid);
		size_t k = 0;
		while (k < c->arenas.size() && !(at >= c->arenas[k].base && at < c->arenas[k].base + c->arenas[k].cap)) ++k;
		if (k == c->arenas.size()) { c->err = "not a batch of ssv_batch_retain (no arena holds it)"; return SSV_E_ARG; }
		// ... and the slab must be one that is live: a copy of a batch released before (or any pointer into an arena) would count the arena down a second
		// time and hand its memory back while other batches still live in it
		auto &slabs = c->arenas[k].slabs;
		const auto it = std::find(slabs.begin(), slabs.end(), (size_t)(at - c->arenas[k].base));
		if (it == slabs.end()) { c->err = "not a live batch of ssv_batch_retain (released before, or not the start of a batch)"; return SSV_E_ARG; }
		slabs.erase(it);
		for (size_t j = c->pairdup_live.size(); j-- > 0;) if (c->pairdup_live[j].slab == (const void *)at) c->pairdup_live.erase(c->pairdup_live.begin() + (long)j); // (its rows go with it)
		if (--c->arenas[k].live == 0) {
			if (k + 1 == c->arenas.size()) c->arenas[k].used = 0;
			else { c->spare_arenas.push_back({c->arenas[k].base, c->arenas[k].cap}); c->arenas.erase(c->arenas.begin() + (long)k); } // (kept for the next retain: ssv_ctx::spare_arenas)
		}
	}
	free(const_cast<ssv_tid_run *>(b->tid_runs));
	memset(b, 0, sizeof(*b));
	return SSV_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------------------------------------------------

int ssv_prof_enable(ssv_ctx *c, int on)
{
	if (!c) return SSV_E_ARG;
	prof_collect(c);
	c->prof_mode = on;
	return SSV_OK;
}

int ssv_prof_reset(ssv_ctx *c)
{
	if (!c) return SSV_E_ARG;
	prof_collect(c);
	for (int k = 0; k < P_COUNT; ++k) { c->prof_ms[k] = 0; c->prof_launches[k] = 0; c->prof_units[k] = 0; }
	return SSV_OK;
}

int ssv_prof_get(ssv_ctx *c, const char *name, double *total_ms, int64_t *launches, int64_t *units)
{
	if (!c || !name) return SSV_E_ARG;
	prof_collect(c);
	for (int k = 0; k < P_COUNT; ++k) {
		if (strcmp(name, kProfNames[k]) == 0) {
			if (total_ms) *total_ms = c->prof_ms[k];
			if (launches) *launches = c->prof_launches[k];
			if (units) *units = c->prof_units[k];
			return SSV_OK;
		}
	}
	return SSV_E_ARG;
}

const char *ssv_prof_names(void) { return kProfNameList; }

#include "bamdec_api.inc"
#include "realign_api.inc"
#include "readthrough_api.inc"
#include "samdec_api.inc"
#include "alnpack_api.inc"
#include "dup_api.inc"
#include "sort_api.inc"
#include "pairdup_api.inc"
#include "region_api.inc"
#include "group_api.inc"


// Streams are synchronised and every handle goes here, in this order; the buffers - members of the context and of the stages' states - go with `delete c`, behind
// the streams that may have used them.
void ssv_ctx_destroy(ssv_ctx *c)
{
	if (!c) return;
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->st);

	table_helper_stop(c); // (a rebuild still pending ends first: it reads the buffers that go below)
	for (auto &t : c->clip->tab) if (t.in_flight && t.via_link) { table_link_wait(c, t); t.in_flight = false; } // (a table still on its way out)
	bamdec_release_handles(c);
	samdec_release_handles(c);
	if (c->st_h2d) { (void)hipStreamSynchronize(c->st_h2d); (void)hipStreamDestroy(c->st_h2d); }
	for (auto &a : c->arenas) if (a.base) (void)hipFree(a.base);
	for (auto &a : c->spare_arenas) (void)hipFree(a.base);
	{ size_t cap = 0; if (uint8_t *b = arena_ahead_take(c, &cap)) (void)hipFree(b); }
	for (auto &S : c->ss) if (S.ready) (void)hipEventDestroy(S.ready);
	if (c->ev_st) (void)hipEventDestroy(c->ev_st);
	for (auto &t : c->clip->tab) {
		if (t.copied) (void)hipEventDestroy(t.copied);
		if (t.small_ev) (void)hipEventDestroy(t.small_ev);
		if (c->link.signal_destroy && t.copied_sig.handle) (void)c->link.signal_destroy(t.copied_sig);
		if (c->link.signal_destroy && t.big_sig.handle) (void)c->link.signal_destroy(t.big_sig);
		if (t.packed_ev) (void)hipEventDestroy(t.packed_ev);
	}
	if (c->st_copy) { (void)hipStreamSynchronize(c->st_copy); (void)hipStreamDestroy(c->st_copy); }
	if (c->ev_packed) (void)hipEventDestroy(c->ev_packed);
	for (ProfRec &r : c->prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
	for (hipEvent_t e : c->prof_pool) (void)hipEventDestroy(e);
	(void)hipStreamDestroy(c->st);
	delete c;
}

int ssv_ctx_create(int device, ssv_ctx **out)
{
	if (!out) return SSV_E_ARG;
	*out = nullptr;
	int ndev = 0;
	hipError_t e = hipGetDeviceCount(&ndev);
	if (e != hipSuccess || ndev <= 0) {
		g_create_error = std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") + "); libseeksv_hip has no CPU path";
		return SSV_E_NODEVICE;
	}
	if (device < 0 || device >= ndev) { g_create_error = "device ordinal out of range"; return SSV_E_ARG; }
	if ((e = hipSetDevice(device)) != hipSuccess) { g_create_error = hipGetErrorString(e); return SSV_E_NODEVICE; }
	ssv_ctx *c = new ssv_ctx();
	c->device = device;
	c->clip.reset(new ssv_clip_state()); c->isz.reset(new ssv_isize_state()); c->getsv.reset(new ssv_getsv_state());
	if ((e = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking)) != hipSuccess) { g_create_error = hipGetErrorString(e); delete c; return SSV_E_NODEVICE; }
	TableSet *tab = c->clip->tab;
	bool ok = true;
	for (hipStream_t *s : {&c->st_copy, &c->st_h2d}) ok = ok && hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess;
	for (hipEvent_t *ev : {&c->ev_st, &c->ss[0].ready, &c->ss[1].ready, &c->ev_packed, &tab[0].packed_ev, &tab[1].packed_ev, &tab[0].copied, &tab[1].copied, &tab[0].small_ev, &tab[1].small_ev})
		ok = ok && hipEventCreateWithFlags(ev, hipEventDisableTiming) == hipSuccess;
	if (!ok) { g_create_error = "cannot create the copy stream / events"; ssv_ctx_destroy(c); return SSV_E_NODEVICE; }
	link_init(c);
	if (c->link.ok) for (int k = 0; k < 2; ++k) if (c->link.signal_create(0, 0, nullptr, &tab[k].copied_sig) != HSA_STATUS_SUCCESS || c->link.signal_create(0, 0, nullptr, &tab[k].big_sig) != HSA_STATUS_SUCCESS) { c->link.ok = false; break; }
	*out = c;
	return SSV_OK;
}

} // extern "C"
