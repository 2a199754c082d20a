// pairdup_api.inc - C ABI of `run -D` (duplicate read pairs by the unclipped 5' ends of both reads, in any record order); included by seeksv_hip.hip, kernels in
// pairdup_kernels.h.  Which retained batches carry rows is written down in ssv_ctx::pairdup_live (ssv_batch_release strikes a batch out there too).

struct ssv_pairdup_state {
	// ssv_pairdup_retain's temporaries
	DBuf hnames, hoff, cig_n, cig_at, seq_b, seq_at;
	SmallWords small;
	// ssv_pairdup_mark's
	DBuf src, part, at, keys[2], vals[2], first, pat, w1, w2, w3, g1, g2;
	// when the mark returns everything goes back, the retain calls' temporaries too (the mark ends the retention: the sort and the passes that follow get the memory)
	void drop() { for (DBuf *x : {&src, &part, &at, &keys[0], &keys[1], &vals[0], &vals[1], &first, &pat, &w1, &w2, &w3, &g1, &g2, &hnames, &hoff, &cig_n, &cig_at, &seq_b, &seq_at}) x->reset(); }
};

namespace {

enum PdWord { PW_BAD, PW_CIG, PW_SEQ, PW_PART, PW_PAIRS, PW_MARKED, PW_MANY, PW_COUNT }; // u64 words of the small block
constexpr size_t PD_SMALL_BYTES = 64;
static_assert(PW_COUNT * 8 <= PD_SMALL_BYTES, "the small block holds every word");

ssv_ctx::PairdupLive *pd_live(ssv_ctx *c, const ssv_batch_t *b)
{
	if (!b || b->mem != (SSV_MEM_DEVICE | SSV_MEM_PERSISTENT) || !b->tid) return nullptr;
	for (auto &e : c->pairdup_live) if (e.slab == (const void *)b->tid && e.n == b->n) return &e;
	return nullptr;
}

} // namespace

int ssv_pairdup_retain(ssv_ctx *c, const ssv_batch_t *b, const ssv_names_t *nm, ssv_batch_t *out)
{
	if (!c) return SSV_E_ARG;
	if (!b || !nm || !out) { c->err = "ssv_pairdup_retain: NULL argument"; return SSV_E_ARG; }
	if ((b->mem & ~(int)SSV_MEM_PERSISTENT) != SSV_MEM_DEVICE) { c->err = "ssv_pairdup_retain takes device batches"; return SSV_E_ARG; }
	CHECK(check_names(c, nm, b->n, "ssv_pairdup_retain"));
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->pairdup) c->pairdup.reset(new ssv_pairdup_state());
	ssv_pairdup_state &S = *c->pairdup;
	DevBatch d;
	CHECK(stage_batch(c, b, d));
	CHECK(staged_ends(c, d));
	DevNames names{nullptr, nullptr, 0};
	if (d.n) CHECK(stage_names(c, nm, d.n, S.hnames, S.hoff, names));
	const int64_t N = d.n;
	const uint64_t mask = env_low_bits_mask("SSV_DUP_DIGEST_BITS"); // (tests) so that names collide
	CHECK(S.small.reserve(c, PD_SMALL_BYTES));
	uint64_t *sm = P<uint64_t>(S.small.dev);
	const uint64_t *hs = P<uint64_t>(S.small.host);
	CHECK(S.small.clear(c));

	// ---- what every record takes in the batch that stays ----
	if (N) {
		ProfScope ps(c, P_PAIRDUP_ENDS, N);
		CHECK(ensure(c, S.cig_n, (size_t)N * 4 + 16)); CHECK(ensure(c, S.cig_at, (size_t)N * 4 + 16)); CHECK(ensure(c, S.seq_b, (size_t)N * 4 + 16)); CHECK(ensure(c, S.seq_at, (size_t)N * 8 + 16));
		CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(N + 1) * 4)); CHECK(ensure(c, c->scan_scratch64, scan_scratch_elems(N + 1) * 8));
		k_pd_sizes<<<grid_for(N, BLOCK), BLOCK, 0, c->st>>>(d, P<uint32_t>(S.cig_n), P<uint32_t>(S.seq_b));
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(S.cig_n), P<uint32_t>(S.cig_at), N, 0u, P<uint32_t>(c->scan_scratch), reinterpret_cast<uint32_t *>(sm + PW_CIG));
		exclusive_scan<uint32_t, uint64_t>(c->st, P<uint32_t>(S.seq_b), P<uint64_t>(S.seq_at), N, 0ull, P<uint64_t>(c->scan_scratch64), sm + PW_SEQ);
		HIPCHECK(c, hipGetLastError());
	}
	CHECK(S.small.fetch(c));
	const size_t out_cig = (size_t)hs[PW_CIG], out_seq = (size_t)hs[PW_SEQ];

	// ---- memory (the last point where the call can fail for lack of it): the seven parts of every retained batch, then the rows ----
	RetainedSlab R((size_t)N, out_cig, out_seq, (size_t)N * sizeof(PdRow) + 16);
	CHECK(R.copy_runs(c, b));
	CHECK(R.take(c));
	PdRow *rows = R.part<PdRow>(7);

	// ---- the rows, and the records into the slab ----
	if (N) {
		ProfScope ps(c, P_PAIRDUP_ENDS, N);
		k_pd_rows<<<grid_for(N * DUP_SUB, BLOCK), BLOCK, 0, c->st>>>(d, names, mask, rows, reinterpret_cast<uint32_t *>(sm + PW_BAD));
		DupView v;
		memset(&v, 0, sizeof(v));
		v.b = d; v.nb = names; v.n = N;
		const DupDst dst{R.dst(), nullptr, nullptr};
		k_dup_gather<<<grid_for(N * DUP_SUB, BLOCK), BLOCK, 0, c->st>>>(v, 0, N, nullptr, P<uint32_t>(S.cig_at), P<uint64_t>(S.seq_at), P<uint32_t>(S.seq_b), nullptr, nullptr, 1, dst);
		HIPCHECK(c, hipGetLastError());
	}
	CHECK(S.small.fetch(c)); // (the source - the decoder's buffers - may be overwritten by the next decode)
	if (hs[PW_BAD]) { c->err = "ssv_pairdup_retain: a record that takes part comes without its qualities (decode with keep_all_seq)"; return SSV_E_ARG; }
	for (size_t k = c->pairdup_live.size(); k-- > 0;) if (c->pairdup_live[k].slab == (const void *)R.slab) c->pairdup_live.erase(c->pairdup_live.begin() + (long)k);
	c->pairdup_live.push_back(ssv_ctx::PairdupLive{R.slab, N, rows});
	R.hand_out(out, b->max_ref_span);
	return SSV_OK;
}

int ssv_pairdup_rows(ssv_ctx *c, const ssv_batch_t *b, const void **dev_rows)
{
	if (!c) return SSV_E_ARG;
	const ssv_ctx::PairdupLive *e = dev_rows ? pd_live(c, b) : nullptr;
	if (!e) { c->err = "ssv_pairdup_rows: not a batch of ssv_pairdup_retain with live rows"; return SSV_E_ARG; }
	*dev_rows = e->rows;
	return SSV_OK;
}

// A hook of the tests, not part of the ABI (no declaration in seeksv_hip.h): the rows of a batch copied to host memory of the caller's, [n] rows of 24 bytes.
int ssv_pairdup_rows_to_host(ssv_ctx *c, const ssv_batch_t *b, void *rows);
int ssv_pairdup_rows_to_host(ssv_ctx *c, const ssv_batch_t *b, void *rows)
{
	const void *dev = nullptr;
	CHECK(ssv_pairdup_rows(c, b, &dev));
	HIPCHECK(c, hipSetDevice(c->device));
	if (b->n > 0) {
		if (!rows) { c->err = "ssv_pairdup_rows_to_host: no room"; return SSV_E_ARG; }
		HIPCHECK(c, hipMemcpyAsync(rows, dev, (size_t)b->n * sizeof(PdRow), hipMemcpyDeviceToHost, c->st));
	}
	HIPCHECK(c, hipStreamSynchronize(c->st));
	return SSV_OK;
}

int ssv_pairdup_mark(ssv_ctx *c, ssv_batch_t *batches, int64_t n_batches, ssv_pairdup_stats *stats)
{
	if (!c) return SSV_E_ARG;
	if (!stats || n_batches < 0 || (n_batches > 0 && !batches)) { c->err = "ssv_pairdup_mark: bad arguments"; return SSV_E_ARG; }
	int64_t N = 0;
	std::vector<PdSrc> tab((size_t)std::max<int64_t>(1, n_batches), PdSrc{0, nullptr, nullptr});
	for (int64_t k = 0; k < n_batches; ++k) {
		const ssv_ctx::PairdupLive *e = pd_live(c, &batches[k]);
		bool twice = false;
		for (int64_t j = 0; j < k && e; ++j) twice = twice || batches[j].tid == batches[k].tid;
		if (!e || twice || (batches[k].n > 0 && !batches[k].rec)) { c->err = "ssv_pairdup_mark takes batches of ssv_pairdup_retain, each once, that no call has marked yet"; return SSV_E_ARG; }
		tab[(size_t)k] = PdSrc{N, const_cast<ssv_record *>(batches[k].rec), static_cast<const PdRow *>(e->rows)};
		N += batches[k].n;
	}
	if (N >= (1ll << 32)) { c->err = "ssv_pairdup_mark: 2^32 records or more (a record's index is carried as 32 bits)"; return SSV_E_RANGE; }
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->pairdup) c->pairdup.reset(new ssv_pairdup_state());
	ssv_pairdup_state &S = *c->pairdup;
	struct Drop { ssv_pairdup_state &S; ~Drop() { S.drop(); } } drop{S};
	const int n_src = (int)tab.size();
	int bits;
	(void)env_low_bits_mask("SSV_DUP_DIGEST_BITS", &bits); // (the name sort looks at the bits that ssv_pairdup_retain kept)
	CHECK(S.small.reserve(c, PD_SMALL_BYTES));
	uint64_t *sm = P<uint64_t>(S.small.dev);
	const uint64_t *hs = P<uint64_t>(S.small.host);
	int64_t m = 0, n_pairs = 0, marked = 0, many = 0;

	if (N) {
		// ---- the rows that take part, with g, ordered by name hash ----
		CHECK(ensure(c, S.src, tab.size() * sizeof(PdSrc)));
		HIPCHECK(c, hipMemcpyAsync(S.src.p, tab.data(), tab.size() * sizeof(PdSrc), hipMemcpyHostToDevice, c->st));
		CHECK(S.small.clear(c));
		const PdSrc *src = P<PdSrc>(S.src);
		CHECK(ensure(c, S.part, (size_t)N * 4 + 16)); CHECK(ensure(c, S.at, (size_t)N * 4 + 16));
		CHECK(ensure(c, c->scan_scratch, (size_t)scan_scratch_elems(N + 1) * 4 + 64));
		{
			ProfScope ps(c, P_PAIRDUP_JOIN, N);
			k_pd_part<<<grid_for(N, BLOCK), BLOCK, 0, c->st>>>(src, n_src, N, P<uint32_t>(S.part));
			exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(S.part), P<uint32_t>(S.at), N, 0u, P<uint32_t>(c->scan_scratch), reinterpret_cast<uint32_t *>(sm + PW_PART));
			HIPCHECK(c, hipGetLastError());
		}
		CHECK(S.small.fetch(c)); // (the table's host copy is read by now)
		m = (int64_t)hs[PW_PART];
	}
	if (m) {
		const PdSrc *src = P<PdSrc>(S.src);
		const int64_t nt = rs_tiles(m);
		for (int k = 0; k < 2; ++k) { CHECK(ensure(c, S.keys[k], (size_t)m * 8 + 16)); CHECK(ensure(c, S.vals[k], (size_t)m * 4 + 16)); }
		CHECK(ensure(c, S.first, (size_t)m * 4 + 16)); CHECK(ensure(c, S.pat, (size_t)m * 4 + 16));
		CHECK(ensure(c, c->ghist, (size_t)256 * nt * 4)); CHECK(ensure(c, c->scan_scratch, (size_t)scan_scratch_elems(std::max<int64_t>(256 * nt, m + 1)) * 4 + 64));
		uint64_t *keys[2] = {P<uint64_t>(S.keys[0]), P<uint64_t>(S.keys[1])};
		uint32_t *vals[2] = {P<uint32_t>(S.vals[0]), P<uint32_t>(S.vals[1])};
		{
			ProfScope ps(c, P_PAIRDUP_JOIN, m);
			k_pd_compact<<<grid_for(N, BLOCK), BLOCK, 0, c->st>>>(src, n_src, N, P<uint32_t>(S.part), P<uint32_t>(S.at), keys[0], vals[0]);
			const int cur = radix_sort_pairs(c->st, keys, vals, m, bits, P<uint32_t>(c->ghist), P<uint32_t>(c->scan_scratch));
			k_pd_join<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(src, n_src, keys[cur], vals[cur], m, P<uint32_t>(S.first));
			exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(S.first), P<uint32_t>(S.pat), m, 0u, P<uint32_t>(c->scan_scratch), reinterpret_cast<uint32_t *>(sm + PW_PAIRS));
			HIPCHECK(c, hipGetLastError());
			CHECK(S.small.fetch(c));
			n_pairs = (int64_t)hs[PW_PAIRS];
			if (n_pairs) {
				// (the pairs' sorts use the name sort's buffers: the rows in name order move to the side that the first pair sort writes last)
				for (DBuf *x : {&S.w1, &S.w2, &S.w3}) CHECK(ensure(c, *x, (size_t)n_pairs * 8 + 16));
				for (DBuf *x : {&S.g1, &S.g2}) CHECK(ensure(c, *x, (size_t)n_pairs * 4 + 16));
				const int other = cur ^ 1;
				k_pd_pairs<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(src, n_src, vals[cur], P<uint32_t>(S.first), P<uint32_t>(S.pat), m, keys[other], vals[other], P<uint64_t>(S.w1), P<uint64_t>(S.w2),
				                                                     P<uint64_t>(S.w3), P<uint32_t>(S.g1), P<uint32_t>(S.g2));
				HIPCHECK(c, hipGetLastError());
				std::swap(keys[0], keys[other]); std::swap(vals[0], vals[other]); // keys[0] / vals[0]: the pairs with the first sort's word
			}
		}
		if (n_pairs) {
			// ---- by (score down, g up), then by the key from its least significant word: stable, so the first pair of every run of equal keys is its keeper ----
			ProfScope ps(c, P_PAIRDUP_MARK, n_pairs);
			int cur = 0;
			const uint64_t *words[3] = {P<uint64_t>(S.w3), P<uint64_t>(S.w2), P<uint64_t>(S.w1)};
			for (int pass = 0; pass < 4; ++pass) {
				uint64_t *k2[2] = {keys[cur], keys[cur ^ 1]};
				uint32_t *v2[2] = {vals[cur], vals[cur ^ 1]};
				if (pass > 0) k_pd_load_keys<<<grid_for(n_pairs, BLOCK), BLOCK, 0, c->st>>>(words[pass - 1], v2[0], n_pairs, k2[0]);
				cur ^= radix_sort_pairs(c->st, k2, v2, n_pairs, 64, P<uint32_t>(c->ghist), P<uint32_t>(c->scan_scratch));
			}
			// (from here on the call cannot fail for lack of memory: the flags are written by its last kernel)
			k_pd_pick<<<grid_for(n_pairs, BLOCK), BLOCK, 0, c->st>>>(src, n_src, vals[cur], n_pairs, P<uint64_t>(S.w1), P<uint64_t>(S.w2), P<uint64_t>(S.w3), P<uint32_t>(S.g1), P<uint32_t>(S.g2),
			                                                        reinterpret_cast<unsigned long long *>(sm + PW_MARKED));
			HIPCHECK(c, hipGetLastError());
			CHECK(S.small.fetch(c));
			marked = (int64_t)hs[PW_MARKED]; many = (int64_t)hs[PW_MANY];
		}
	}
	HIPCHECK(c, hipStreamSynchronize(c->st));
	// the rows are dead: the batches are ordinary retained batches from here on
	for (int64_t k = 0; k < n_batches; ++k)
		for (size_t j = c->pairdup_live.size(); j-- > 0;) if (c->pairdup_live[j].slab == (const void *)batches[k].tid) c->pairdup_live.erase(c->pairdup_live.begin() + (long)j);
	memset(stats, 0, sizeof(*stats));
	stats->records = N; stats->taking_part = m; stats->pairs = n_pairs; stats->unpaired = m - 2 * n_pairs; stats->groups_many = many; stats->pairs_marked = marked;
	prof_collect(c);
	return SSV_OK;
}
