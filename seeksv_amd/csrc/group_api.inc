// group_api.inc - the one exchange step of a range-partitioned run (included by seeksv_hip.hip inside extern "C").
// Every rank (one context = one GPU = one host thread) ends the getsv passes with a vector of partial results - discordant counts per
// junction, depth sums per range, point depths - that must be added up over the ranks (SURVEY 8e).  The vectors are all-gathered with
// RCCL over xGMI (ncclAllGather: every GPU has a direct link to each peer; the payload is KBs to a few MB, i.e. latency bound) and summed
// locally.  librccl is loaded on first use (dlopen): a single-GPU run never touches it.  Ranks that share one GPU (a test hook: several
// ranks on one device cannot form an RCCL communicator) exchange through host memory instead.  SSV_GROUP_RCCL_ONE=1 makes a group of ONE
// rank an RCCL communicator too (ncclCommInitAll over one device): every line of the RCCL branch - dlopen, the communicator, the
// collective's kernel, the polled stream, the copy back, abort and destroy - then runs on a one-GPU box.
namespace {

typedef void *rcclComm_t;
struct RcclApi {
	void *lib = nullptr;
	int (*CommInitAll)(rcclComm_t *, int, const int *) = nullptr;
	int (*AllGather)(const void *, void *, size_t, int, rcclComm_t, hipStream_t) = nullptr;
	int (*CommDestroy)(rcclComm_t) = nullptr;
	int (*CommAbort)(rcclComm_t) = nullptr;
	const char *(*GetErrorString)(int) = nullptr;
	bool load(std::string &err)
	{
		if (lib) return true;
		for (const char *name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) { lib = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (lib) break; }
		if (!lib) { err = std::string("cannot load librccl.so: ") + dlerror(); return false; }
		CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(lib, "ncclCommInitAll"));
		AllGather = reinterpret_cast<decltype(AllGather)>(dlsym(lib, "ncclAllGather"));
		CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
		CommAbort = reinterpret_cast<decltype(CommAbort)>(dlsym(lib, "ncclCommAbort"));
		GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
		if (!CommInitAll || !AllGather || !CommDestroy) { err = "librccl.so lacks ncclCommInitAll / ncclAllGather / ncclCommDestroy"; return false; }
		return true;
	}
};
RcclApi g_rccl;
constexpr int RCCL_UINT8 = 1; // ncclUint8 (rccl.h: ncclInt8 = 0, ncclUint8 = 1)

} // namespace

struct ssv_group {
	int n = 0;
	std::vector<ssv_ctx *> ctx;
	bool is_rccl = false;         // false: host-memory exchange
	std::vector<rcclComm_t> comm; // sized once at creation, never resized; an entry is nulled (under mu) when the communicators are aborted
	// a reusable barrier on the group's mutex that also carries what the ranks have to agree on: did any of them fail, do they all bring the
	// same number of bytes
	std::mutex mu;
	std::condition_variable cv;
	std::vector<std::vector<uint8_t>> slot;
	int arrived = 0, generation = 0;
	bool any_failed = false, last_failed = false;
	size_t round_bytes = 0;
	bool round_has_bytes = false, size_mismatch = false, last_mismatch = false;
	bool aborted = false;
	int in_call = 0;       // ranks inside ncclAllGather right now (it only enqueues): an abort waits for them, so no handle is freed under a caller
	bool broken = false;   // a rank did not show up in time, or the communicators were aborted: every later call fails at once
	std::string err;
	std::vector<DBuf> d_send, d_recv;
	double timeout_s = 600;
	int fail_rank = -1, fail_stage = 0; // test hook SSV_GROUP_FAIL=<rank>:<stage> (1: before the exchange, 2: the collective itself, 3: the wait behind an issued collective)
};

int ssv_group_create(ssv_ctx **ctxs, int n, ssv_group **out)
{
	if (!ctxs || n < 1 || !out) return SSV_E_ARG;
	*out = nullptr;
	ssv_group *g = new ssv_group();
	g->n = n; g->ctx.assign(ctxs, ctxs + n); g->slot.resize((size_t)n); g->d_send.resize((size_t)n); g->d_recv.resize((size_t)n);
	if (const char *e = getenv("SSV_GROUP_TIMEOUT_S")) g->timeout_s = std::max(0.05, atof(e));
	if (const char *e = getenv("SSV_GROUP_FAIL")) { g->fail_rank = atoi(e); const char *q = strchr(e, ':'); g->fail_stage = q ? atoi(q + 1) : 1; }
	bool distinct = n > 1 || getenv("SSV_GROUP_RCCL_ONE");
	for (int a = 0; a < n; ++a) for (int b = a + 1; b < n; ++b) if (ctxs[a]->device == ctxs[b]->device) distinct = false;
	if (distinct) {
		if (!g_rccl.load(g->err)) { g_create_error = g->err; delete g; return SSV_E_NODEVICE; }
		std::vector<int> devs((size_t)n);
		for (int a = 0; a < n; ++a) devs[(size_t)a] = ctxs[a]->device;
		g->comm.assign((size_t)n, nullptr);
		const int rc = g_rccl.CommInitAll(g->comm.data(), n, devs.data());
		if (rc != 0) { g_create_error = std::string("ncclCommInitAll: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error"); delete g; return SSV_E_HIP; }
		g->is_rccl = true;
	}
	*out = g;
	return SSV_OK;
}

void ssv_group_destroy(ssv_group *g)
{
	if (!g) return;
	for (rcclComm_t c : g->comm) if (c) (void)g_rccl.CommDestroy(c);
	for (size_t k = 0; k < g->d_send.size(); ++k) {
		(void)hipSetDevice(g->ctx[k]->device); // (a rank's buffers go with its device current)
		g->d_send[k].reset(); g->d_recv[k].reset();
	}
	delete g;
}

int ssv_group_uses_rccl(const ssv_group *g) { return g && g->is_rccl ? 1 : 0; }

enum { AGREE_OK = 0, AGREE_FAILED = 1, AGREE_SIZES = 2, AGREE_TIMEOUT = 3 };

// All ranks meet here and leave with the SAME answer: AGREE_FAILED when any of them came with `failed` set, AGREE_SIZES when their byte
// counts differ (`bytes` is ignored with check_size false), AGREE_TIMEOUT when a rank did not arrive within the group's time limit (the
// group is broken from then on: the missing rank's thread is gone or stuck, nothing can be exchanged any more).
static int group_agree(ssv_group *g, bool failed, bool check_size = false, size_t bytes = 0)
{
	std::unique_lock<std::mutex> lk(g->mu);
	if (g->broken) return AGREE_TIMEOUT;
	if (failed) g->any_failed = true;
	if (check_size) {
		if (!g->round_has_bytes) { g->round_bytes = bytes; g->round_has_bytes = true; }
		else if (g->round_bytes != bytes) g->size_mismatch = true;
	}
	const int gen = g->generation;
	if (++g->arrived == g->n) {
		g->arrived = 0; g->last_failed = g->any_failed; g->last_mismatch = g->size_mismatch;
		g->any_failed = false; g->size_mismatch = false; g->round_has_bytes = false;
		++g->generation; g->cv.notify_all();
	} else if (!g->cv.wait_for(lk, std::chrono::duration<double>(g->timeout_s), [&] { return g->generation != gen || g->broken; }) || g->broken) {
		g->broken = true; g->cv.notify_all();
		return AGREE_TIMEOUT;
	}
	// (the answer of this round cannot be overwritten before every rank has read it: the next round completes only when all have arrived again)
	return g->last_failed ? AGREE_FAILED : g->last_mismatch ? AGREE_SIZES : AGREE_OK;
}

static int agree_error(ssv_group *g, ssv_ctx *c, int a, int own_rc)
{
	if (own_rc != SSV_OK) return own_rc; // (the rank's own text is in c->err)
	if (a == AGREE_FAILED) { c->err = "another rank failed before the exchange: nothing was gathered"; return SSV_E_STATE; }
	if (a == AGREE_SIZES) { c->err = "ranks contributed vectors of different sizes"; return SSV_E_ARG; }
	{ std::unique_lock<std::mutex> lk(g->mu); c->err = g->aborted ? "the group's communicators were aborted after a failed exchange: the group is unusable"
	                                                                : "a rank did not reach the exchange in time (SSV_GROUP_TIMEOUT_S): the group is unusable"; }
	return SSV_E_STATE;
}

// tear the communicators down so that ranks waiting inside the collective (or in the stream behind it) come back
static void group_abort(ssv_group *g)
{
	std::vector<rcclComm_t> victims;
	{
		std::unique_lock<std::mutex> lk(g->mu);
		g->broken = true; g->aborted = true;
		g->cv.wait_for(lk, std::chrono::seconds(5), [&] { return g->in_call == 0; }); // (ncclAllGather only enqueues; a call that does not come back is not waited for for ever)
		victims = g->comm;                          // the handles leave under the lock and their entries are nulled IN PLACE: the vector keeps its
		for (rcclComm_t &c : g->comm) c = nullptr;  // size, a rank that looks its communicator up meanwhile finds a null handle or `broken`, not freed memory
		g->cv.notify_all();
	}
	for (rcclComm_t c : victims) if (c) { if (g_rccl.CommAbort) (void)g_rccl.CommAbort(c); else (void)g_rccl.CommDestroy(c); }
}

// every rank calls this once per exchange, from its own thread.  Whatever goes wrong on ONE rank - a failed allocation or copy, a vector of
// another size, an error out of ncclAllGather, a thread that never arrives - every rank RETURNS, all with an error.
int ssv_group_allgather(ssv_group *g, int rank, const void *send, size_t bytes, void *recv)
{
	if (!g || rank < 0 || rank >= g->n || (bytes && (!send || !recv))) return SSV_E_ARG;
	ssv_ctx *c = g->ctx[(size_t)rank];
	const bool inject1 = g->fail_rank == rank && g->fail_stage == 1, inject2 = g->fail_rank == rank && g->fail_stage == 2, inject3 = g->fail_rank == rank && g->fail_stage == 3;
	if (g->is_rccl) {
		// Everything that can fail on one rank alone - device selection, buffers, the copy of its vector - happens BEFORE the collective, and the
		// ranks agree through the host that all of them got there with vectors of one size: a rank that returned early would leave the others
		// waiting in ncclAllGather (and in the stream synchronisation behind it) for ever.
		auto prepare = [&]() -> int {
			if (inject1) { c->err = "SSV_GROUP_FAIL: injected failure before the exchange"; return SSV_E_HIP; }
			HIPCHECK(c, hipSetDevice(c->device));
			CHECK(ensure(c, g->d_send[(size_t)rank], bytes + 16)); CHECK(ensure(c, g->d_recv[(size_t)rank], bytes * (size_t)g->n + 16));
			if (bytes) HIPCHECK(c, hipMemcpyAsync(g->d_send[(size_t)rank].p, send, bytes, hipMemcpyHostToDevice, c->st));
			HIPCHECK(c, hipStreamSynchronize(c->st));
			return SSV_OK;
		};
		const int prc = prepare();
		const int a = group_agree(g, prc != SSV_OK, true, bytes);
		if (a != AGREE_OK || prc != SSV_OK) return agree_error(g, c, a, prc);
		// The collective.  A rank whose ncclAllGather fails (or that waits longer than the group's limit for the stream behind it) aborts ALL
		// communicators of the group: the peers' kernels end, their waits below return, and the second agreement hands everybody the error.
		rcclComm_t mine = nullptr;
		{ std::unique_lock<std::mutex> lk(g->mu); if (!g->broken && !inject2) { mine = g->comm[(size_t)rank]; if (mine) ++g->in_call; } } // (a peer may abort the group at any time: the handle is read under the lock)
		int own = SSV_OK;
		const int rc = inject2 ? 1 : !mine ? 0 : g_rccl.AllGather(g->d_send[(size_t)rank].p, g->d_recv[(size_t)rank].p, bytes, RCCL_UINT8, mine, c->st);
		if (mine) { std::unique_lock<std::mutex> lk(g->mu); --g->in_call; g->cv.notify_all(); }
		if (!mine && !inject2) { c->err = "the exchange was aborted: another rank failed inside the collective"; own = SSV_E_STATE; }
		else if (inject3) { c->err = "SSV_GROUP_FAIL: injected failure behind an issued collective: communicators aborted"; own = SSV_E_STATE; group_abort(g); (void)hipStreamSynchronize(c->st); }
		else if (rc != 0) {
			c->err = std::string("ncclAllGather: ") + (inject2 ? "SSV_GROUP_FAIL: injected failure" : g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
			own = SSV_E_HIP;
			group_abort(g);
		} else {
			const auto t0 = std::chrono::steady_clock::now();
			for (;;) {
				const hipError_t q = hipStreamQuery(c->st);
				if (q == hipSuccess) break;
				if (q != hipErrorNotReady) { c->err = std::string("ncclAllGather (stream): ") + hipGetErrorString(q); own = SSV_E_HIP; group_abort(g); break; }
				bool broken; { std::unique_lock<std::mutex> lk(g->mu); broken = g->broken; }
				if (broken) { c->err = "the exchange was aborted: another rank failed inside the collective"; own = SSV_E_STATE; break; }
				if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > g->timeout_s) {
					c->err = "ncclAllGather did not finish in time (SSV_GROUP_TIMEOUT_S): communicators aborted"; own = SSV_E_STATE; group_abort(g); break;
				}
				std::this_thread::sleep_for(std::chrono::microseconds(20));
			}
		}
		if (own == SSV_OK && bytes) {
			hipError_t e = hipMemcpyAsync(recv, g->d_recv[(size_t)rank].p, bytes * (size_t)g->n, hipMemcpyDeviceToHost, c->st);
			if (e == hipSuccess) e = hipStreamSynchronize(c->st);
			if (e != hipSuccess) { c->err = std::string("copy of the gathered vectors: ") + hipGetErrorString(e); own = SSV_E_HIP; }
		}
		const int a2 = group_agree(g, own != SSV_OK);
		if (own != SSV_OK) return own;
		if (a2 == AGREE_FAILED) { c->err = "another rank failed inside the exchange"; return SSV_E_STATE; }
		if (a2 != AGREE_OK) return agree_error(g, c, a2, SSV_OK);
		return SSV_OK;
	}
	// ranks on one GPU: through host memory.  Phase one: every rank leaves its vector in its slot and the ranks
	// agree that all did, with one size; phase two: everybody has copied all slots (nobody overwrites a slot before everybody has read it).
	int prc = SSV_OK;
	if (inject1) { c->err = "SSV_GROUP_FAIL: injected failure before the exchange"; prc = SSV_E_HIP; }
	else {
		std::unique_lock<std::mutex> lk(g->mu);
		g->slot[(size_t)rank].assign((const uint8_t *)send, (const uint8_t *)send + bytes);
	}
	const int a = group_agree(g, prc != SSV_OK, true, bytes);
	if (a != AGREE_OK || prc != SSV_OK) return agree_error(g, c, a, prc);
	int own = SSV_OK;
	if (inject2) { c->err = "SSV_GROUP_FAIL: injected failure inside the exchange"; own = SSV_E_HIP; }
	else for (int r = 0; r < g->n && bytes; ++r) memcpy((uint8_t *)recv + (size_t)r * bytes, g->slot[(size_t)r].data(), bytes); // (slots are stable between the two barriers)
	const int a2 = group_agree(g, own != SSV_OK);
	if (own != SSV_OK) return own;
	if (a2 == AGREE_FAILED) { c->err = "another rank failed inside the exchange"; return SSV_E_STATE; }
	if (a2 != AGREE_OK) return agree_error(g, c, a2, SSV_OK);
	return SSV_OK;
}
