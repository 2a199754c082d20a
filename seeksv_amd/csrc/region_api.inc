// region_api.inc - C ABI of `run -L` / `run -X` (the records that stay resident restricted to a list of regions); included by seeksv_hip.hip, kernels in
// region_kernels.h.  Two entry points - ssv_region_retain for a decoder's batch, ssv_batch_select for a batch that is retained already - over one routine.

struct ssv_region_state {
	// the list (ssv_regions_set)
	bool set = false;
	int exclude = 0;
	int32_t n_targets = 0;
	int64_t n_regions = 0;
	DBuf off, s, t;
	// what the last call handed out in its info (host memory, the context's until the next call)
	std::vector<uint32_t> change_index;
	std::vector<int32_t> change_tid;
	// the calls' temporaries (grow-only while batches stream through; ssv_regions_clear gives them back)
	DBuf keep, at, idx, cig_n, seq_b, cig_at, seq_at, flag, mark, mark_at, tile_last, tile_prev, ch_index, ch_tid, raw_runs;
	HBuf h_changes, h_raw_runs;
	SmallWords small;
	void drop()
	{
		for (DBuf *x : {&keep, &at, &idx, &cig_n, &seq_b, &cig_at, &seq_at, &flag, &mark, &mark_at, &tile_last, &tile_prev, &ch_index, &ch_tid, &raw_runs}) x->reset();
	}
};

namespace {

enum RegionWord { RW_KEPT, RW_CIG, RW_CHANGES, RW_LAST_TID, RW_RAW_RUNS, RW_COUNT32 }; // u32 words of the small block; at byte 32 one u64: bytes of bases + qualities
constexpr size_t REGION_SMALL_BYTES = 64;
constexpr int REGION_SMALL_U64_AT = 4;
static_assert(RW_COUNT32 * 4 <= REGION_SMALL_U64_AT * 8, "the u32 words end where the u64 word begins");
constexpr uint32_t REGION_RAW_RUN_CAP = TidLists::RAW_RUN_CAP;

// is b a retained batch that is live: the start of a slab some arena counts (what ssv_batch_release asks before it gives one back)
bool retained_is_live(const ssv_ctx *c, const ssv_batch_t *b)
{
	if (b->mem != (SSV_MEM_DEVICE | SSV_MEM_PERSISTENT) || !b->tid || b->n < 0 || b->n >= (1ll << 31)) return false;
	if (b->n > 0 && (!b->pos || !b->n_cigar || !b->cigar_ends || !b->rec)) return false;
	const uint8_t *at = reinterpret_cast<const uint8_t *>(b->tid);
	for (const auto &a : c->arenas)
		if (at >= a.base && at < a.base + a.cap) return std::find(a.slabs.begin(), a.slabs.end(), (size_t)(at - a.base)) != a.slabs.end();
	return false;
}

// The contig changes among the records of a batch that are not UNMAP|MUNMAP (sort_kernels.h's kernels, as ssv_batch_sort runs them), into the state's lists;
// prev_tid: the contig of the last such record before the batch, and behind it on return.  Synchronises the stream.
int region_changes(ssv_ctx *c, ssv_region_state &S, const int32_t *tid, const ssv_record *rec, int64_t n, int32_t &prev_tid)
{
	S.change_index.clear(); S.change_tid.clear();
	if (n == 0) return SSV_OK;
	const int64_t n_tiles = (n + BLOCK - 1) / BLOCK;
	CHECK(ensure(c, S.flag, (size_t)n * 2 + 16)); CHECK(ensure(c, S.mark, (size_t)n * 4 + 16)); CHECK(ensure(c, S.mark_at, (size_t)n * 4 + 16));
	CHECK(ensure(c, S.tile_last, (size_t)n_tiles * 4 + 16)); CHECK(ensure(c, S.tile_prev, (size_t)n_tiles * 4 + 16));
	CHECK(ensure(c, c->scan_scratch, (size_t)scan_scratch_elems(n) * 4 + 64));
	uint32_t *w = P<uint32_t>(S.small.dev);
	k_sort_flags<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(rec, n, P<uint16_t>(S.flag));
	k_tid_tile_last<<<(unsigned)n_tiles, BLOCK, 0, c->st>>>(tid, P<uint16_t>(S.flag), n, P<int32_t>(S.tile_last));
	k_tid_tile_carry<<<1, WAVE, 0, c->st>>>(P<int32_t>(S.tile_last), n_tiles, prev_tid, P<int32_t>(S.tile_prev), reinterpret_cast<int32_t *>(w + RW_LAST_TID));
	k_sort_change_mark<<<(unsigned)n_tiles, BLOCK, 0, c->st>>>(tid, P<uint16_t>(S.flag), n, P<int32_t>(S.tile_prev), P<uint32_t>(S.mark));
	exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(S.mark), P<uint32_t>(S.mark_at), n, 0u, P<uint32_t>(c->scan_scratch), w + RW_CHANGES);
	HIPCHECK(c, hipGetLastError());
	CHECK(S.small.fetch(c));
	const uint32_t *hs = P<uint32_t>(S.small.host);
	const size_t m = hs[RW_CHANGES];
	prev_tid = (int32_t)hs[RW_LAST_TID];
	if (!m) return SSV_OK;
	CHECK(ensure(c, S.ch_index, m * 4 + 16)); CHECK(ensure(c, S.ch_tid, m * 4 + 16)); CHECK(ensure_host(c, S.h_changes, m * 8 + 16));
	k_sort_change_place<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(P<uint32_t>(S.mark), P<uint32_t>(S.mark_at), tid, n, P<uint32_t>(S.ch_index), P<int32_t>(S.ch_tid));
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipMemcpyAsync(S.h_changes.p, S.ch_index.p, m * 4, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipMemcpyAsync(P<uint8_t>(S.h_changes) + m * 4, S.ch_tid.p, m * 4, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const uint32_t *ix = P<uint32_t>(S.h_changes);
	const int32_t *tv = reinterpret_cast<const int32_t *>(ix + m);
	S.change_index.assign(ix, ix + m);
	S.change_tid.assign(tv, tv + m);
	return SSV_OK;
}

void region_info(const ssv_region_state &S, int64_t n_in, int64_t n_kept, int uncopied, int32_t last_tid, ssv_region_info *info)
{
	memset(info, 0, sizeof(*info));
	info->n_in = n_in; info->n_kept = n_kept; info->uncopied = uncopied; info->last_tid = last_tid;
	info->n_changes = (uint32_t)S.change_index.size(); info->change_index = S.change_index.data(); info->change_tid = S.change_tid.data();
}

// The one routine.  d: the input where it lies (lines and cigar_ends are there).  hand_back: when every record stays nothing is written and *uncopied is set -
// the caller hands its input out.  Otherwise *out is a new retained batch of the kept records.  The input is only read.
int region_run(ssv_ctx *c, const DevBatch &d, bool hand_back, int32_t last_tid, ssv_batch_t *out, ssv_region_info *info, bool *uncopied)
{
	ssv_region_state &S = *c->region;
	const int64_t n = d.n;
	*uncopied = false;
	CHECK(S.small.reserve(c, REGION_SMALL_BYTES));
	uint32_t *w = P<uint32_t>(S.small.dev);
	uint64_t *w64 = P<uint64_t>(S.small.dev) + REGION_SMALL_U64_AT;
	const uint32_t *hs = P<uint32_t>(S.small.host);
	const uint64_t *hs64 = P<uint64_t>(S.small.host) + REGION_SMALL_U64_AT;
	CHECK(S.small.clear(c));
	const RegionList L{P<uint32_t>(S.off), P<int32_t>(S.s), P<int32_t>(S.t), S.n_targets};

	// ---- which records stay, and where ----
	if (n) {
		ProfScope ps(c, P_REGION_SELECT, n);
		CHECK(ensure(c, S.keep, (size_t)n + 16)); CHECK(ensure(c, S.at, (size_t)n * 4 + 16));
		CHECK(ensure(c, c->scan_scratch, (size_t)scan_scratch_elems(n) * 4 + 64));
		k_region_keep<<<grid_for(n, BLOCK * REGION_TILES), BLOCK, 0, c->st>>>(d, L, S.exclude, P<uint8_t>(S.keep));
		exclusive_scan<uint8_t, uint32_t>(c->st, P<uint8_t>(S.keep), P<uint32_t>(S.at), n, 0u, P<uint32_t>(c->scan_scratch), w + RW_KEPT);
		HIPCHECK(c, hipGetLastError());
	}
	CHECK(S.small.fetch(c));
	const int64_t m = (int64_t)hs[RW_KEPT];
	int32_t prev_tid = last_tid;
	if (hand_back && m == n) { // every record stays: the input is the output
		{
			ProfScope ps(c, P_REGION_SELECT, n);
			CHECK(region_changes(c, S, d.tid, d.rec, n, prev_tid));
		}
		*uncopied = true;
		region_info(S, n, n, 1, prev_tid, info);
		return SSV_OK;
	}

	// ---- what the kept records take in the batch that stays ----
	size_t out_cig = 0, out_seq = 0;
	if (m) {
		ProfScope ps(c, P_REGION_SELECT, m);
		for (DBuf *x : {&S.idx, &S.cig_n, &S.seq_b, &S.cig_at}) CHECK(ensure(c, *x, (size_t)m * 4 + 16));
		CHECK(ensure(c, S.seq_at, (size_t)m * 8 + 16));
		CHECK(ensure(c, c->scan_scratch64, (size_t)scan_scratch_elems(m) * 8 + 64));
		k_region_place<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(d, P<uint8_t>(S.keep), P<uint32_t>(S.at), P<uint32_t>(S.idx), P<uint32_t>(S.cig_n), P<uint32_t>(S.seq_b));
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(S.cig_n), P<uint32_t>(S.cig_at), m, 0u, P<uint32_t>(c->scan_scratch), w + RW_CIG);
		exclusive_scan<uint32_t, uint64_t>(c->st, P<uint32_t>(S.seq_b), P<uint64_t>(S.seq_at), m, 0ull, P<uint64_t>(c->scan_scratch64), w64);
		HIPCHECK(c, hipGetLastError());
		CHECK(S.small.fetch(c));
		out_cig = (size_t)hs[RW_CIG]; out_seq = (size_t)hs64[0];
	}

	// ---- memory (the last point where the call can fail for lack of it), and the records into it ----
	RetainedSlab R((size_t)m, out_cig, out_seq);
	CHECK(R.take(c));
	const RetDst dst = R.dst();
	if (m) {
		ProfScope ps(c, P_REGION_GATHER, m);
		k_region_gather<<<grid_for(m * RET_SUB, BLOCK), BLOCK, 0, c->st>>>(d, P<uint32_t>(S.idx), m, P<uint32_t>(S.cig_at), P<uint64_t>(S.seq_at), P<uint32_t>(S.seq_b), dst);
		HIPCHECK(c, hipGetLastError());
	}
	// ---- the output's tid column as runs, under the decoders' cap, and its contig changes ----
	if (m) {
		ProfScope ps(c, P_REGION_SELECT, m);
		CHECK(ensure(c, S.raw_runs, (size_t)REGION_RAW_RUN_CAP * sizeof(TidRun))); CHECK(ensure_host(c, S.h_raw_runs, (size_t)REGION_RAW_RUN_CAP * sizeof(TidRun)));
		k_tid_raw_runs<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(dst.tid, m, P<TidRun>(S.raw_runs), REGION_RAW_RUN_CAP, w + RW_RAW_RUNS); // (its counter: zero since the clear above)
		HIPCHECK(c, hipGetLastError());
		HIPCHECK(c, hipMemcpyAsync(S.h_raw_runs.p, S.raw_runs.p, (size_t)REGION_RAW_RUN_CAP * sizeof(TidRun), hipMemcpyDeviceToHost, c->st));
	}
	{
		ProfScope ps(c, P_REGION_SELECT, m);
		CHECK(region_changes(c, S, dst.tid, dst.rec, m, prev_tid)); // (synchronises: the runs and their count are on the host, and the source may go)
	}
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const uint32_t nr = m ? hs[RW_RAW_RUNS] : 0u;
	if (nr >= 1 && nr <= REGION_RAW_RUN_CAP) {
		ssv_tid_run *runs = R.new_runs(c, nr);
		if (!runs) return SSV_E_NOMEM;
		const TidRun *r = P<TidRun>(S.h_raw_runs);
		for (uint32_t k = 0; k < nr; ++k) runs[k] = ssv_tid_run{(int64_t)r[k].index, r[k].tid, 0};
		std::sort(runs, runs + nr, [](const ssv_tid_run &a, const ssv_tid_run &b) { return a.first < b.first; });
	}
	R.hand_out(out, d.max_ref_span);
	region_info(S, n, m, 0, prev_tid, info);
	return SSV_OK;
}

} // namespace

int ssv_regions_set(ssv_ctx *c, const ssv_region *regions, int64_t n, int32_t n_targets, int exclude)
{
	if (!c) return SSV_E_ARG;
	if (n < 0 || n >= (1ll << 31) || (n > 0 && !regions) || n_targets < 0) { c->err = "ssv_regions_set: bad arguments"; return SSV_E_ARG; }
	for (int64_t k = 0; k < n; ++k) {
		const ssv_region &r = regions[k];
		if (r.tid < 0 || r.tid >= n_targets || r.s < 0 || r.s >= r.t) { c->err = "ssv_regions_set: a region outside the contigs, or with s < 0 or s >= t"; return SSV_E_ARG; }
		if (k > 0 && (regions[k - 1].tid > r.tid || (regions[k - 1].tid == r.tid && regions[k - 1].t >= r.s))) {
			c->err = "ssv_regions_set: the list is not normalised (sorted by contig and start, no two regions overlapping or abutting)"; return SSV_E_ARG;
		}
	}
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->region) c->region.reset(new ssv_region_state());
	ssv_region_state &S = *c->region;
	std::vector<uint32_t> off((size_t)n_targets + 1, 0u);
	std::vector<int32_t> st((size_t)n * 2 + 1, 0);
	for (int64_t k = 0; k < n; ++k) { ++off[(size_t)regions[k].tid + 1]; st[(size_t)k] = regions[k].s; st[(size_t)(n + k)] = regions[k].t; }
	for (int32_t t = 0; t < n_targets; ++t) off[(size_t)t + 1] += off[(size_t)t];
	HIPCHECK(c, hipStreamSynchronize(c->st)); // (a list still in use by kernels of the call before)
	S.set = false;
	CHECK(ensure(c, S.off, off.size() * 4 + 16)); CHECK(ensure(c, S.s, (size_t)n * 4 + 16)); CHECK(ensure(c, S.t, (size_t)n * 4 + 16));
	HIPCHECK(c, hipMemcpyAsync(S.off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->st));
	if (n) {
		HIPCHECK(c, hipMemcpyAsync(S.s.p, st.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->st));
		HIPCHECK(c, hipMemcpyAsync(S.t.p, st.data() + n, (size_t)n * 4, hipMemcpyHostToDevice, c->st));
	}
	HIPCHECK(c, hipStreamSynchronize(c->st)); // (the host vectors go)
	S.set = true; S.exclude = exclude ? 1 : 0; S.n_targets = n_targets; S.n_regions = n;
	return SSV_OK;
}

int ssv_regions_clear(ssv_ctx *c)
{
	if (!c) return SSV_E_ARG;
	if (!c->region) return SSV_OK;
	HIPCHECK(c, hipSetDevice(c->device));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	c->region.reset();
	return SSV_OK;
}

int ssv_region_lds_capacity(void) { return REGION_LDS_CAP; }

int ssv_region_retain(ssv_ctx *c, const ssv_batch_t *b, int32_t last_tid, ssv_batch_t *out, ssv_region_info *info)
{
	if (!c) return SSV_E_ARG;
	if (!b || !out || !info) { c->err = "ssv_region_retain: NULL argument"; return SSV_E_ARG; }
	if ((b->mem & ~(int)SSV_MEM_PERSISTENT) != SSV_MEM_DEVICE) { c->err = "ssv_region_retain takes device batches"; return SSV_E_ARG; } // (so no announced host batch is consumed below)
	if (!c->region || !c->region->set) { c->err = "ssv_region_retain: no list of regions is set (ssv_regions_set)"; return SSV_E_STATE; }
	HIPCHECK(c, hipSetDevice(c->device));
	DevBatch d;
	CHECK(stage_batch(c, b, d)); // (builds the record lines when the batch has none)
	CHECK(staged_ends(c, d));
	bool uncopied = false;
	CHECK(region_run(c, d, false, last_tid, out, info, &uncopied));
	prof_collect(c);
	return SSV_OK;
}

int ssv_batch_select(ssv_ctx *c, ssv_batch_t *in, int32_t last_tid, ssv_batch_t *out, ssv_region_info *info)
{
	if (!c) return SSV_E_ARG;
	if (!in || !out || !info) { c->err = "ssv_batch_select: NULL argument"; return SSV_E_ARG; }
	if (!retained_is_live(c, in)) { c->err = "ssv_batch_select takes a live batch of ssv_batch_retain, ssv_dup_retain, ssv_batch_sort or (marked) ssv_pairdup_retain"; return SSV_E_ARG; }
	if (pd_live(c, in)) { c->err = "ssv_batch_select: the batch carries rows of ssv_pairdup_retain that no ssv_pairdup_mark has used yet"; return SSV_E_ARG; }
	if (!c->region || !c->region->set) { c->err = "ssv_batch_select: no list of regions is set (ssv_regions_set)"; return SSV_E_STATE; }
	HIPCHECK(c, hipSetDevice(c->device));
	DevBatch d;
	CHECK(stage_batch(c, in, d));
	bool uncopied = false;
	ssv_batch_t made;
	CHECK(region_run(c, d, true, last_tid, &made, info, &uncopied));
	if (uncopied) made = *in; // the same device memory, its tid_runs with it
	else {
		ssv_batch_t gone = *in;
		const int rc = ssv_batch_release(c, &gone);
		if (rc != SSV_OK) { const std::string err = c->err; (void)ssv_batch_release(c, &made); c->err = err; return rc; } // (cannot happen to a batch that passed the check above)
	}
	memset(in, 0, sizeof(*in));
	*out = made;
	prof_collect(c);
	return SSV_OK;
}
