// sort_api.inc - C ABI of `run -u` (the retained batches of an original in any order, coordinate sorted in HBM); included by seeksv_hip.hip, kernels in sort_kernels.h

struct ssv_sort_state {
	// what the last ssv_batch_sort handed out (host memory, the context's until the next call)
	std::vector<ssv_batch_t> batches;
	std::vector<int64_t> change_first;
	std::vector<uint32_t> change_index;
	std::vector<int32_t> change_tid;
	// a call's temporaries (given back when it returns: the passes that follow get the memory)
	DBuf src, keys[2], vals[2], cig_n, seq_b, cig_at, seq_at, flag, mark, at, tile_last, tile_prev, ch_index, ch_tid, raw_runs;
	HBuf h_changes, h_raw_runs;
	SmallWords small;
	void drop()
	{
		for (DBuf *x : {&src, &keys[0], &keys[1], &vals[0], &vals[1], &cig_n, &seq_b, &cig_at, &seq_at, &flag, &mark, &at, &tile_last, &tile_prev, &ch_index, &ch_tid, &raw_runs}) x->reset();
	}
};

namespace {

constexpr size_t SORT_SMALL_BYTES = 256;
constexpr int SORT_SMALL_U64_AT = 8; // the u64 words of the small block start at byte 64: [0] operations, [1] bytes of bases + qualities of an output batch
enum { SW_CHANGES = ssv::SW_COUNT32 };
static_assert((SW_CHANGES + 1) * 4 <= SORT_SMALL_U64_AT * 8, "the u32 words end where the u64 words begin");
constexpr uint32_t SORT_RAW_RUN_CAP = TidLists::RAW_RUN_CAP;
constexpr int64_t SORT_DEFAULT_BATCH = (int64_t)16 << 20;

inline int bits_of(uint64_t x) { int b = 0; while (x) { ++b; x >>= 1; } return b; }

// The contig changes among the records of one batch that are not UNMAP|MUNMAP (tid: its hot column, rec: its lines), appended to the lists; prev_tid: the
// contig of the last such record before the batch, and behind it on return.
int sort_changes(ssv_ctx *c, ssv_sort_state &S, const int32_t *tid, const ssv_record *rec, int64_t n, int32_t &prev_tid)
{
	if (n == 0) return SSV_OK;
	const int64_t n_tiles = (n + BLOCK - 1) / BLOCK;
	CHECK(ensure(c, S.flag, (size_t)n * 2 + 16)); CHECK(ensure(c, S.mark, (size_t)n * 4 + 16)); CHECK(ensure(c, S.at, (size_t)n * 4 + 16));
	CHECK(ensure(c, S.tile_last, (size_t)n_tiles * 4 + 16)); CHECK(ensure(c, S.tile_prev, (size_t)n_tiles * 4 + 16));
	CHECK(ensure(c, c->scan_scratch, (size_t)scan_scratch_elems(n) * 4 + 64));
	uint32_t *w = P<uint32_t>(S.small.dev);
	k_sort_flags<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(rec, n, P<uint16_t>(S.flag));
	k_tid_tile_last<<<(unsigned)n_tiles, BLOCK, 0, c->st>>>(tid, P<uint16_t>(S.flag), n, P<int32_t>(S.tile_last));
	k_tid_tile_carry<<<1, WAVE, 0, c->st>>>(P<int32_t>(S.tile_last), n_tiles, prev_tid, P<int32_t>(S.tile_prev), reinterpret_cast<int32_t *>(w + SW_LAST_TID));
	k_sort_change_mark<<<(unsigned)n_tiles, BLOCK, 0, c->st>>>(tid, P<uint16_t>(S.flag), n, P<int32_t>(S.tile_prev), P<uint32_t>(S.mark));
	exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(S.mark), P<uint32_t>(S.at), n, 0u, P<uint32_t>(c->scan_scratch), w + SW_CHANGES);
	HIPCHECK(c, hipGetLastError());
	CHECK(S.small.fetch(c));
	const uint32_t *hs = P<uint32_t>(S.small.host);
	const size_t m = hs[SW_CHANGES];
	prev_tid = (int32_t)hs[SW_LAST_TID];
	if (!m) return SSV_OK;
	CHECK(ensure(c, S.ch_index, m * 4 + 16)); CHECK(ensure(c, S.ch_tid, m * 4 + 16)); CHECK(ensure_host(c, S.h_changes, m * 8 + 16));
	k_sort_change_place<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(P<uint32_t>(S.mark), P<uint32_t>(S.at), tid, n, P<uint32_t>(S.ch_index), P<int32_t>(S.ch_tid));
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipMemcpyAsync(S.h_changes.p, S.ch_index.p, m * 4, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipMemcpyAsync(P<uint8_t>(S.h_changes) + m * 4, S.ch_tid.p, m * 4, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const uint32_t *ix = P<uint32_t>(S.h_changes);
	const int32_t *tv = reinterpret_cast<const int32_t *>(ix + m);
	S.change_index.insert(S.change_index.end(), ix, ix + m);
	S.change_tid.insert(S.change_tid.end(), tv, tv + m);
	return SSV_OK;
}

void sort_result(ssv_sort_state &S, int64_t n_records, int already_sorted, ssv_sorted *out)
{
	memset(out, 0, sizeof(*out));
	out->n_records = n_records; out->n_batches = (int64_t)S.batches.size(); out->already_sorted = already_sorted;
	out->batches = S.batches.data(); out->change_first = S.change_first.data(); out->change_index = S.change_index.data(); out->change_tid = S.change_tid.data();
}

} // namespace

int ssv_batch_sort(ssv_ctx *c, ssv_batch_t *in, int64_t n_in, int32_t n_targets, int64_t max_out_records, ssv_sorted *out)
{
	if (!c) return SSV_E_ARG;
	if (!out || n_in < 0 || (n_in > 0 && !in) || n_targets < 0 || max_out_records < 0) { c->err = "ssv_batch_sort: bad arguments"; return SSV_E_ARG; }
	int64_t N = 0;
	int32_t span = 0;
	bool span_unknown = false;
	for (int64_t k = 0; k < n_in; ++k) {
		const ssv_batch_t &b = in[k];
		if (b.mem != (SSV_MEM_DEVICE | SSV_MEM_PERSISTENT) || b.n < 0 || b.n >= (1ll << 31) || !b.tid || (b.n > 0 && (!b.pos || !b.n_cigar || !b.cigar_ends || !b.rec))) {
			c->err = "ssv_batch_sort takes batches of ssv_batch_retain"; return SSV_E_ARG;
		}
		N += b.n;
		if (b.n > 0) { span = std::max(span, b.max_ref_span); span_unknown = span_unknown || b.max_ref_span <= 0; }
	}
	if (N >= (1ll << 32)) { c->err = "ssv_batch_sort: 2^32 records or more (the sort carries a record's index as 32 bits)"; return SSV_E_RANGE; }
	if (span_unknown) span = 0;
	if (max_out_records == 0) {
		const char *e = getenv("SSV_SORT_BATCH_RECORDS"); // (tests) small output batches
		max_out_records = e && atoll(e) > 0 ? atoll(e) : SORT_DEFAULT_BATCH;
	}
	max_out_records = std::min<int64_t>(max_out_records, (1ll << 31) - 1);
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->sort) c->sort.reset(new ssv_sort_state());
	ssv_sort_state &S = *c->sort;
	const bool in_is_ours = !S.batches.empty() && in == S.batches.data(); // (the outputs of the call before, sorted again)
	const std::vector<ssv_batch_t> inputs(in, in + n_in);
	struct Drop { ssv_sort_state &S; ~Drop() { S.drop(); } } drop{S};
	CHECK(S.small.reserve(c, SORT_SMALL_BYTES));
	uint32_t *w = P<uint32_t>(S.small.dev);
	uint64_t *w64 = P<uint64_t>(S.small.dev) + SORT_SMALL_U64_AT;
	const uint32_t *hs = P<uint32_t>(S.small.host);
	const uint64_t *hs64 = P<uint64_t>(S.small.host) + SORT_SMALL_U64_AT;

	// ---- the inputs as one sequence; is it in order already ----
	const int n_src = (int)std::max<int64_t>(1, n_in);
	std::vector<SortSrc> tab((size_t)n_src, SortSrc{});
	{
		int64_t at = 0;
		for (int64_t k = 0; k < n_in; ++k) {
			const ssv_batch_t &b = inputs[(size_t)k];
			tab[(size_t)k] = SortSrc{at, b.tid, b.pos, b.n_cigar, b.cigar_ends, b.rec, b.cigar, b.seqqual};
			at += b.n;
		}
	}
	CHECK(ensure(c, S.src, tab.size() * sizeof(SortSrc)));
	HIPCHECK(c, hipMemcpyAsync(S.src.p, tab.data(), tab.size() * sizeof(SortSrc), hipMemcpyHostToDevice, c->st));
	CHECK(S.small.clear(c));
	const SortSrc *src = P<SortSrc>(S.src);
	if (N) {
		ProfScope ps(c, P_SORT_KEYS, N);
		k_sort_check<<<grid_for(N, BLOCK), BLOCK, 0, c->st>>>(src, n_src, N, n_targets, w);
		HIPCHECK(c, hipGetLastError());
	}
	CHECK(S.small.fetch(c)); // (the table's host copy is read by now)
	if (hs[SW_BAD]) { c->err = "ssv_batch_sort: a record's contig id is not below n_targets"; return SSV_E_ARG; }
	const bool down = hs[SW_DOWN] != 0;
	const int p_bits = bits_of(hs[SW_MAXP]), t_bits = bits_of((uint64_t)n_targets);

	// From here on the lists of the call before are gone.  A failure below gives back what it made and leaves the inputs as they were.
	std::vector<ssv_batch_t> made;
	S.batches.clear(); S.change_first.assign(1, 0); S.change_index.clear(); S.change_tid.clear();
	auto fail = [&](int rc) {
		const std::string err = c->err;
		for (size_t k = made.size(); k-- > 0;) (void)ssv_batch_release(c, &made[k]);
		c->err = err;
		S.batches.clear(); S.change_first.clear(); S.change_index.clear(); S.change_tid.clear();
		return rc;
	};
	int32_t prev_tid = 0;

	if (!down) { // in order: the inputs are the outputs
		for (const ssv_batch_t &b : inputs) {
			ProfScope ps(c, P_SORT_KEYS, b.n);
			const int rc = sort_changes(c, S, b.tid, b.rec, b.n, prev_tid);
			if (rc != SSV_OK) return fail(rc);
			S.change_first.push_back((int64_t)S.change_index.size());
		}
		S.batches = inputs;
		if (!in_is_ours) for (int64_t k = 0; k < n_in; ++k) memset(&in[k], 0, sizeof(in[k])); // (one owner: the batches are the result's now)
		sort_result(S, N, 1, out);
		return SSV_OK;
	}

	auto body = [&]() -> int {
		// ---- keys of the bits that can differ, sorted ----
		const int64_t nt = rs_tiles(N);
		for (int k = 0; k < 2; ++k) { CHECK(ensure(c, S.keys[k], (size_t)N * 8 + 16)); CHECK(ensure(c, S.vals[k], (size_t)N * 4 + 16)); }
		CHECK(ensure(c, c->ghist, (size_t)256 * nt * 4)); CHECK(ensure(c, c->scan_scratch, (size_t)scan_scratch_elems(256 * nt) * 4 + 64));
		uint64_t *keys[2] = {P<uint64_t>(S.keys[0]), P<uint64_t>(S.keys[1])};
		uint32_t *vals[2] = {P<uint32_t>(S.vals[0]), P<uint32_t>(S.vals[1])};
		{
			ProfScope ps(c, P_SORT_KEYS, N);
			k_sort_keys<<<grid_for(N, BLOCK), BLOCK, 0, c->st>>>(src, n_src, N, n_targets, p_bits, keys[0], vals[0]);
			HIPCHECK(c, hipGetLastError());
		}
		int cur;
		{
			ProfScope ps(c, P_SORT_RADIX, N);
			cur = radix_sort_pairs(c->st, keys, vals, N, p_bits + t_bits, P<uint32_t>(c->ghist), P<uint32_t>(c->scan_scratch));
			HIPCHECK(c, hipGetLastError());
		}
		const uint32_t *perm = vals[cur];

		// ---- one output batch after the other ----
		for (int64_t first = 0; first < N;) {
			int64_t count = std::min(max_out_records, N - first);
			uint64_t out_cig = 0, out_seq = 0;
			for (;;) { // (a batch whose operations would not fit cigar_off's 32 bits is cut earlier: halved until they do - one record has at most 65535)
				ProfScope ps(c, P_SORT_GATHER, count);
				for (DBuf *x : {&S.cig_n, &S.seq_b}) CHECK(ensure(c, *x, (size_t)count * 4 + 16));
				for (DBuf *x : {&S.cig_at, &S.seq_at}) CHECK(ensure(c, *x, (size_t)count * 8 + 16));
				CHECK(ensure(c, c->scan_scratch64, (size_t)scan_scratch_elems(count) * 8 + 64));
				k_sort_sizes<<<grid_for(count, BLOCK), BLOCK, 0, c->st>>>(src, n_src, perm, first, count, P<uint32_t>(S.cig_n), P<uint32_t>(S.seq_b));
				exclusive_scan<uint32_t, uint64_t>(c->st, P<uint32_t>(S.cig_n), P<uint64_t>(S.cig_at), count, 0ull, P<uint64_t>(c->scan_scratch64), w64 + 0);
				exclusive_scan<uint32_t, uint64_t>(c->st, P<uint32_t>(S.seq_b), P<uint64_t>(S.seq_at), count, 0ull, P<uint64_t>(c->scan_scratch64), w64 + 1);
				HIPCHECK(c, hipGetLastError());
				CHECK(S.small.fetch(c));
				out_cig = hs64[0]; out_seq = hs64[1];
				if (out_cig < (1ull << 32) || count == 1) break;
				count = (count + 1) / 2;
			}
			RetainedSlab R((size_t)count, (size_t)out_cig, (size_t)out_seq);
			CHECK(R.take(c));
			const RetDst dst = R.dst();
			{
				ProfScope ps(c, P_SORT_GATHER, count);
				k_sort_gather<<<grid_for(count * SORT_SUB, BLOCK), BLOCK, 0, c->st>>>(src, n_src, perm, first, count, P<uint64_t>(S.cig_at), P<uint64_t>(S.seq_at), P<uint32_t>(S.seq_b), dst);
				HIPCHECK(c, hipGetLastError());
			}
			// the tid column as runs, under the decoders' cap
			CHECK(ensure(c, S.raw_runs, (size_t)SORT_RAW_RUN_CAP * sizeof(TidRun))); CHECK(ensure_host(c, S.h_raw_runs, (size_t)SORT_RAW_RUN_CAP * sizeof(TidRun)));
			HIPCHECK(c, hipMemsetAsync(w + SW_RAW_RUNS, 0, 4, c->st));
			{
				ProfScope ps(c, P_SORT_KEYS, count);
				k_tid_raw_runs<<<grid_for(count, BLOCK), BLOCK, 0, c->st>>>(dst.tid, count, P<TidRun>(S.raw_runs), SORT_RAW_RUN_CAP, w + SW_RAW_RUNS);
				HIPCHECK(c, hipGetLastError());
				HIPCHECK(c, hipMemcpyAsync(S.h_raw_runs.p, S.raw_runs.p, (size_t)SORT_RAW_RUN_CAP * sizeof(TidRun), hipMemcpyDeviceToHost, c->st));
				CHECK(sort_changes(c, S, dst.tid, dst.rec, count, prev_tid)); // (synchronises: the runs and their count are on the host)
			}
			const uint32_t nr = hs[SW_RAW_RUNS];
			if (nr >= 1 && nr <= SORT_RAW_RUN_CAP) {
				ssv_tid_run *runs = R.new_runs(c, nr);
				if (!runs) return SSV_E_NOMEM;
				const TidRun *r = P<TidRun>(S.h_raw_runs);
				for (uint32_t k = 0; k < nr; ++k) runs[k] = ssv_tid_run{(int64_t)r[k].index, r[k].tid, 0};
				std::sort(runs, runs + nr, [](const ssv_tid_run &a, const ssv_tid_run &b) { return a.first < b.first; });
			}
			ssv_batch_t b;
			R.hand_out(&b, span);
			made.push_back(b);
			S.change_first.push_back((int64_t)S.change_index.size());
			first += count;
		}
		return SSV_OK;
	};
	const int rc = body();
	if (rc != SSV_OK) return fail(rc);
	// the inputs go (a failure here leaves a batch that is nobody's: it cannot happen to batches that passed the checks above unless one was given twice)
	for (int64_t k = 0; k < n_in; ++k) {
		ssv_batch_t b = inputs[(size_t)k];
		CHECK(ssv_batch_release(c, &b));
		if (!in_is_ours) memset(&in[k], 0, sizeof(in[k]));
	}
	S.batches = made;
	sort_result(S, N, 0, out);
	prof_collect(c);
	return SSV_OK;
}
