// realign_api.inc - C ABI of the clipped-sequence re-aligner (included by seeksv_hip.hip; kernels in realign_kernels.h, realign_sorted_kernels.h, realign_gap_kernels.h, realign_alts_kernels.h, realign_split_kernels.h and realign_rows_kernels.h)

struct ssv_realign_state {
	DBuf ref, ctg, table, seqs, offs, hits, gaps, dropped;
	DBuf alts, alt_n, alt_off, alt_sums, alt_dense; // ssv_realign_query_alts: strided hits and counts, their scan, the dense list
	DBuf mates; // ssv_realign_query_split: one hit per query
	// ssv_realign_split_batch: qualities and names as uploaded, per read its records / operations / seqqual bytes and their scans, the batch handed out
	DBuf quals, names, name_off, row_n, op_n, sq_n, row_at, op_at, sq_at, rows_small, row_name, row_rec;
	DecodedColumns row_cols;
	DBuf skeys, svals, sdir; // the sorted index (ssv_realign_index_sorted); a context holds one kind of index at a time
	bool sorted = false;
	int32_t dir_bits = 0, max_occ = 0;
	const uint64_t *ref_p = nullptr; // device pointer used by the kernels (own copy or the caller's resident array)
	int64_t n_bases = 0;
	int32_t n_ctg = 0;
	uint64_t mask = 0;
	bool ready = false;
	// what the kernels know of the reference; table and mask are null and 0 while the sorted index stands
	RaIndex index() { return RaIndex{ref_p, n_bases, P<int64_t>(ctg), n_ctg, P<uint32_t>(table), mask}; }
};

// the reference and the contig offsets on the device (both kinds of index)
static int realign_reference(ssv_ctx *c, ssv_realign_state &R, const uint64_t *ref2bit, int32_t mem, int64_t n_bases, const int64_t *target_off, int32_t n_targets)
{
	const size_t words = (size_t)((n_bases + 31) / 32);
	if (mem == SSV_MEM_DEVICE) R.ref_p = ref2bit; // resident: used in place; the caller keeps one readable word of slack after it
	else {
		CHECK(ensure(c, R.ref, (words + 1) * 8));
		HIPCHECK(c, hipMemsetAsync((uint8_t *)R.ref.p + words * 8, 0, 8, c->st));
		HIPCHECK(c, hipMemcpyAsync(R.ref.p, ref2bit, words * 8, hipMemcpyHostToDevice, c->st));
		R.ref_p = P<uint64_t>(R.ref);
	}
	CHECK(ensure(c, R.ctg, (size_t)(n_targets + 1) * 8));
	HIPCHECK(c, hipMemcpyAsync(R.ctg.p, target_off, (size_t)(n_targets + 1) * 8, hipMemcpyHostToDevice, c->st));
	R.n_bases = n_bases; R.n_ctg = n_targets;
	return SSV_OK;
}

// What both index calls begin with: the arguments, the context's state, the other kind of index gone (a context holds one kind at a time; whichever
// buffers of the five are held are the other kind's), the reference on the device.  max_occ counts for the sorted index only.
static int realign_index_begin(ssv_ctx *c, bool sorted, const uint64_t *ref2bit, int32_t mem, int64_t n_bases, const int64_t *target_off, int32_t n_targets, int32_t max_occ = 1)
{
	if (!c || !ref2bit || !target_off || n_targets <= 0 || n_bases <= 0 || target_off[0] != 0 || target_off[n_targets] != n_bases) return SSV_E_ARG;
	if (sorted && (max_occ < 1 || max_occ > 65535)) { c->err = "max_occ outside 1..65535"; return SSV_E_ARG; }
	if (n_bases / RA_SAMPLE >= (int64_t)0xfffffffe) { c->err = "reference too long for the re-aligner's 32-bit slots"; return SSV_E_RANGE; }
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->ra) c->ra.reset(new ssv_realign_state());
	ssv_realign_state &R = *c->ra;
	R.ready = false;
	if (sorted ? R.table.p != nullptr : R.sorted) {
		HIPCHECK(c, hipStreamSynchronize(c->st));
		for (DBuf *b : {&R.table, &R.dropped, &R.skeys, &R.svals, &R.sdir}) HIPCHECK(c, b->release());
		R.mask = 0;
	}
	R.sorted = sorted;
	return realign_reference(c, R, ref2bit, mem, n_bases, target_off, n_targets);
}

int ssv_realign_index(ssv_ctx *c, const uint64_t *ref2bit, int32_t mem, int64_t n_bases, const int64_t *target_off, int32_t n_targets, int64_t *n_dropped)
{
	CHECK(realign_index_begin(c, false, ref2bit, mem, n_bases, target_off, n_targets));
	ssv_realign_state &R = *c->ra;
	const int64_t samples = (n_bases + RA_SAMPLE - 1) / RA_SAMPLE;
	uint64_t slots = 1024;
	while (slots < (uint64_t)samples * 2) slots <<= 1;
	CHECK(ensure(c, R.table, slots * 4));
	HIPCHECK(c, hipMemsetAsync(R.table.p, 0, slots * 4, c->st));
	CHECK(ensure(c, R.dropped, 8));
	HIPCHECK(c, hipMemsetAsync(R.dropped.p, 0, 8, c->st));
	R.mask = slots - 1;
	{
		ProfScope ps(c, P_REALIGN_INDEX, samples);
		k_ra_build<<<grid_for(samples, BLOCK), BLOCK, 0, c->st>>>(R.index(), reinterpret_cast<unsigned long long *>(R.dropped.p));
	}
	HIPCHECK(c, hipGetLastError());
	unsigned long long d = 0;
	HIPCHECK(c, hipMemcpyAsync(&d, R.dropped.p, 8, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	if (n_dropped) *n_dropped = (int64_t)d;
	R.ready = true;
	return SSV_OK;
}

// The sorted index: keys, six passes of the stable radix sort, the directory, the statistics (realign_sorted_kernels.h).  The sort's second pair of
// buffers, its histograms and the statistics' partial sums are freed when the index stands.
int ssv_realign_index_sorted(ssv_ctx *c, const uint64_t *ref2bit, int32_t mem, int64_t n_bases, const int64_t *target_off, int32_t n_targets, int32_t max_occ, ssv_realign_index_stats *stats)
{
	CHECK(realign_index_begin(c, true, ref2bit, mem, n_bases, target_off, n_targets, max_occ));
	ssv_realign_state &R = *c->ra;
	const int64_t samples = (n_bases + RA_SAMPLE - 1) / RA_SAMPLE;
	int bits = 0;
	while (bits < 30 && ((int64_t)2 << bits) <= samples) ++bits; // floor(log2(samples)), at most 30
	const int64_t nt = rs_tiles(samples), n_part = (samples + RAS_STATS_TILE - 1) / RAS_STATS_TILE;
	DBuf keys2, vals2, ghist, scratch, part;
	CHECK(ensure(c, R.skeys, (size_t)samples * 8)); CHECK(ensure(c, R.svals, (size_t)samples * 4)); CHECK(ensure(c, R.sdir, (((size_t)1 << bits) + 1) * 4));
	CHECK(ensure(c, keys2, (size_t)samples * 8)); CHECK(ensure(c, vals2, (size_t)samples * 4));
	CHECK(ensure(c, ghist, (size_t)256 * nt * 4)); CHECK(ensure(c, scratch, (size_t)scan_scratch_elems(256 * nt) * 4));
	CHECK(ensure(c, part, (size_t)(n_part + 1) * sizeof(RasStats)));
	uint64_t *keys[2] = {P<uint64_t>(R.skeys), P<uint64_t>(keys2)};
	uint32_t *vals[2] = {P<uint32_t>(R.svals), P<uint32_t>(vals2)};
	static_assert(((RAS_KEY_BITS + 7) / 8) % 2 == 0, "an even number of passes: the sorted pairs end in the buffers they started in");
	uint32_t n_indexed = 0;
	RasStats st;
	const uint32_t *dir_end = P<uint32_t>(R.sdir) + ((size_t)1 << bits); // = the number of indexed positions
	{
		ProfScope ps(c, P_REALIGN_INDEX, samples);
		k_ras_keys<<<grid_for(samples, BLOCK), BLOCK, 0, c->st>>>(R.index(), samples, keys[0], vals[0]);
		const int cur = radix_sort_pairs(c->st, keys, vals, samples, RAS_KEY_BITS, P<uint32_t>(ghist), P<uint32_t>(scratch));
		if (cur != 0) { c->err = "sorted index: the sort ended in its second buffer"; return SSV_E_STATE; }
		k_ras_dir<<<grid_for(((int64_t)1 << bits) + 1, BLOCK), BLOCK, 0, c->st>>>(keys[0], samples, bits, P<uint32_t>(R.sdir));
		k_ras_stats<<<(unsigned)n_part, BLOCK, 0, c->st>>>(keys[0], dir_end, (uint32_t)max_occ, P<RasStats>(part));
		k_ras_stats_sum<<<1, BLOCK, 0, c->st>>>(P<RasStats>(part), n_part, P<RasStats>(part) + n_part);
	}
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipMemcpyAsync(&n_indexed, dir_end, 4, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipMemcpyAsync(&st, P<RasStats>(part) + n_part, sizeof(st), hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	if (stats) { stats->n_indexed = (int64_t)n_indexed; stats->n_distinct = (int64_t)st.n_distinct; stats->occ_max = (int64_t)st.occ_max; stats->n_over_cap = (int64_t)st.n_over_cap; }
	R.dir_bits = bits; R.max_occ = max_occ;
	R.ready = true;
	return SSV_OK;
}

// One instantiation of the query kernel over the n sequences in R.seqs / R.offs -> R.hits: the arguments every one takes, inside the sorted index's
// and the alternates' (-> R.alts, max_alt per query, and R.alt_n) or the split reads' (-> R.mates) layers where the instantiation has them
extern "C++" template <bool SORTED, int FLOOR, bool ALTS, bool SPLIT = false> // (this file is included inside extern "C")
static void realign_launch_as(ssv_ctx *c, ssv_realign_state &R, int64_t n, int32_t max_alt)
{
	using Query = std::conditional_t<SORTED, RasQueryArgs, RaQueryArgs>;
	using Args = std::conditional_t<ALTS, RaAltArgs<Query>, std::conditional_t<SPLIT, RaSplitArgs<Query>, Query>>;
	Args a;
	static_cast<RaQueryArgs &>(a) = RaQueryArgs{R.index(), P<char>(R.seqs), P<uint64_t>(R.offs), n, P<RaHit>(R.hits)};
	if constexpr (SORTED) a.sx = RasIndex{P<uint64_t>(R.skeys), P<uint32_t>(R.svals), P<uint32_t>(R.sdir), R.dir_bits, R.max_occ};
	if constexpr (ALTS) { a.alts = P<RaHit>(R.alts); a.alt_n = P<int32_t>(R.alt_n); a.max_alt = max_alt; }
	if constexpr (SPLIT) a.mates = P<RaHit>(R.mates);
	k_ra_query_t<SORTED, Args, FLOOR, ALTS, SPLIT><<<grid_for(n, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(a);
}

// the query kernel of the index that stands - with the candidate floor at RA_K when `floor`, going on to the alternates when max_alt > 0 or to the mate
// pieces when `split` (at the default floor and without alternates only: the callers see to that)
static void realign_launch_query(ssv_ctx *c, ssv_realign_state &R, int64_t n, bool floor, int32_t max_alt = 0, bool split = false)
{
	static constexpr decltype(&realign_launch_as<false, RA_MIN_SCORE, false>) launch[2][2][3] = { // [sorted][floor][alts, 2 = split]: k_ra_query, k_ra_query_alts, k_ra_query_split, k_ra_query_floor, ... k_ras_query_floor_alts
		{{realign_launch_as<false, RA_MIN_SCORE, false>, realign_launch_as<false, RA_MIN_SCORE, true>, realign_launch_as<false, RA_MIN_SCORE, false, true>},
		 {realign_launch_as<false, RA_K, false>, realign_launch_as<false, RA_K, true>, nullptr}},
		{{realign_launch_as<true, RA_MIN_SCORE, false>, realign_launch_as<true, RA_MIN_SCORE, true>, realign_launch_as<true, RA_MIN_SCORE, false, true>},
		 {realign_launch_as<true, RA_K, false>, realign_launch_as<true, RA_K, true>, nullptr}}};
	ProfScope ps(c, P_REALIGN_QUERY, n);
	launch[R.sorted][floor][split ? 2 : max_alt > 0](c, R, n, max_alt);
}

// ssv_realign_query (gaps == nullptr), ssv_realign_query_gapped, - max_alt > 0 - ssv_realign_query_alts and - mates != nullptr, ungapped, no alternates -
// ssv_realign_query_split; `who` names the caller in the error text
static int realign_query(ssv_ctx *c, const char *seqs, const uint64_t *seq_off, int64_t n, ssv_realign_hit *hits, ssv_realign_gap *gaps, bool gapped, const char *who,
                         int32_t max_alt = 0, int64_t *alt_off = nullptr, ssv_realign_hit *alts = nullptr, ssv_realign_hit *mates = nullptr)
{
	if (mates && (gapped || max_alt > 0)) return SSV_E_ARG;
	if (!c || n < 0 || (n > 0 && (!seqs || !seq_off || !hits || (gapped && !gaps)))) return SSV_E_ARG;
	if (!c->ra || !c->ra->ready) { c->err = std::string(who) + " before ssv_realign_index"; return SSV_E_STATE; }
	if (n == 0) { if (alt_off) alt_off[0] = 0; return SSV_OK; }
	static_assert(sizeof(RaHit) == sizeof(ssv_realign_hit), "hit layout");
	static_assert(sizeof(RaGap) == sizeof(ssv_realign_gap), "gap layout");
	HIPCHECK(c, hipSetDevice(c->device));
	ssv_realign_state &R = *c->ra;
	const uint64_t bytes = seq_off[n];
	CHECK(ensure(c, R.seqs, bytes + 16)); CHECK(ensure(c, R.offs, (size_t)(n + 1) * 8)); CHECK(ensure(c, R.hits, (size_t)n * sizeof(RaHit)));
	if (gapped) CHECK(ensure(c, R.gaps, (size_t)n * sizeof(RaGap)));
	if (max_alt > 0) {
		CHECK(ensure(c, R.alts, (size_t)n * (size_t)max_alt * sizeof(RaHit))); CHECK(ensure(c, R.alt_n, (size_t)n * 4)); CHECK(ensure(c, R.alt_off, (size_t)(n + 1) * 8));
		CHECK(ensure(c, R.alt_sums, (size_t)scan_scratch_elems(n) * 8));
	}
	if (mates) CHECK(ensure(c, R.mates, (size_t)n * sizeof(RaHit)));
	HIPCHECK(c, hipMemcpyAsync(R.seqs.p, seqs, bytes, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemcpyAsync(R.offs.p, seq_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->st));
	realign_launch_query(c, R, n, gapped, max_alt, mates != nullptr);
	HIPCHECK(c, hipGetLastError());
	if (gapped) {
		RaGapArgs g;
		g.ref = R.ref_p; g.ctg_off = P<int64_t>(R.ctg); g.seqs = P<char>(R.seqs); g.seq_off = P<uint64_t>(R.offs); g.n = n; g.hits = P<RaHit>(R.hits); g.gaps = P<RaGap>(R.gaps);
		{
			ProfScope ps(c, P_REALIGN_GAP, n);
			k_ra_gap<<<grid_for(n, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(g);
		}
		HIPCHECK(c, hipGetLastError());
		HIPCHECK(c, hipMemcpyAsync(gaps, R.gaps.p, (size_t)n * sizeof(RaGap), hipMemcpyDeviceToHost, c->st));
	}
	if (max_alt > 0) { // counts -> offsets; the dense list's size is known on the host before it is gathered
		{
			ProfScope ps(c, P_REALIGN_ALTS, n);
			exclusive_scan<int32_t, int64_t>(c->st, P<int32_t>(R.alt_n), P<int64_t>(R.alt_off), n, (int64_t)0, P<int64_t>(R.alt_sums), P<int64_t>(R.alt_off) + n);
		}
		HIPCHECK(c, hipGetLastError());
		HIPCHECK(c, hipMemcpyAsync(alt_off, R.alt_off.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, c->st));
	}
	if (mates) HIPCHECK(c, hipMemcpyAsync(mates, R.mates.p, (size_t)n * sizeof(RaHit), hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipMemcpyAsync(hits, R.hits.p, (size_t)n * sizeof(RaHit), hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	if (max_alt > 0 && alt_off[n] > 0) {
		const int64_t total = alt_off[n];
		if (total > n * (int64_t)max_alt) { c->err = std::string(who) + ": more alternates than slots"; return SSV_E_STATE; }
		CHECK(ensure(c, R.alt_dense, (size_t)total * sizeof(RaHit)));
		{
			ProfScope ps(c, P_REALIGN_ALTS, total);
			k_ra_alt_compact<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(P<RaHit>(R.alts), P<int32_t>(R.alt_n), P<int64_t>(R.alt_off), n, max_alt, P<RaHit>(R.alt_dense));
		}
		HIPCHECK(c, hipGetLastError());
		HIPCHECK(c, hipMemcpyAsync(alts, R.alt_dense.p, (size_t)total * sizeof(RaHit), hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
	}
	return SSV_OK;
}

int ssv_realign_query(ssv_ctx *c, const char *seqs, const uint64_t *seq_off, int64_t n, ssv_realign_hit *hits)
{
	return realign_query(c, seqs, seq_off, n, hits, nullptr, false, "ssv_realign_query");
}

int ssv_realign_query_gapped(ssv_ctx *c, const char *seqs, const uint64_t *seq_off, int64_t n, ssv_realign_hit *hits, ssv_realign_gap *gaps)
{
	return realign_query(c, seqs, seq_off, n, hits, gaps, true, "ssv_realign_query_gapped");
}

int ssv_realign_query_alts(ssv_ctx *c, const char *seqs, const uint64_t *seq_off, int64_t n, int32_t max_alt, int32_t gapped, ssv_realign_hit *hits, ssv_realign_gap *gaps,
                           int64_t *alt_off, ssv_realign_hit *alts)
{
	if (max_alt < 1 || max_alt > RA_MAX_ALT || !alt_off || !alts || (gapped && !gaps)) return SSV_E_ARG;
	return realign_query(c, seqs, seq_off, n, hits, gapped ? gaps : nullptr, gapped != 0, "ssv_realign_query_alts", max_alt, alt_off, alts);
}

int ssv_realign_query_split(ssv_ctx *c, const char *seqs, const uint64_t *seq_off, int64_t n, ssv_realign_hit *hits, ssv_realign_hit *mates)
{
	if (!mates) return SSV_E_ARG;
	return realign_query(c, seqs, seq_off, n, hits, nullptr, false, "ssv_realign_query_split", 0, nullptr, nullptr, mates);
}

// The split query as it stands, then its reads, hits and mates as the records `seeksv realign -P` writes - built on the device, handed out as a device batch
// (realign_rows_kernels.h): sizes per read, three scans, one read-back of the totals, the rows.
int ssv_realign_split_batch(ssv_ctx *c, const char *seqs, const uint64_t *seq_off, int64_t n, const char *quals, const char *names, const uint64_t *name_off,
                            ssv_realign_hit *hits, ssv_realign_hit *mates, ssv_batch_t *out, ssv_names_t *out_names)
{
	if (!c) return SSV_E_ARG;
	if (!names || !name_off || !out || !out_names || !hits || !mates) { c->err = "ssv_realign_split_batch: names, name_off, hits, mates, out and out_names are required"; return SSV_E_ARG; }
	if (n > ((int64_t)1 << 30)) { c->err = "ssv_realign_split_batch: more than 2^30 reads in one call"; return SSV_E_ARG; }
	for (int64_t i = 0; i < n; ++i) { // (with its NUL a name is 2..255 bytes)
		const uint64_t a = name_off[i], b = name_off[i + 1];
		if (b < a + 2 || b - a > 255) { c->err = "ssv_realign_split_batch: read " + std::to_string(i) + ": a name is 1..254 bytes"; return SSV_E_ARG; }
	}
	CHECK(realign_query(c, seqs, seq_off, n, hits, nullptr, false, "ssv_realign_split_batch", 0, nullptr, nullptr, mates));
	memset(out, 0, sizeof(*out)); memset(out_names, 0, sizeof(*out_names));
	out->mem = SSV_MEM_DEVICE; out->max_ref_span = RA_MAX_Q;
	out_names->mem = SSV_MEM_DEVICE;
	if (n == 0) return SSV_OK;
	ssv_realign_state &R = *c->ra;
	hipStream_t st = c->st;
	const size_t N = (size_t)n;
	const uint64_t seq_bytes = seq_off[n], name_bytes = name_off[n];
	if (quals) { CHECK(ensure(c, R.quals, seq_bytes + 16)); HIPCHECK(c, hipMemcpyAsync(R.quals.p, quals, seq_bytes, hipMemcpyHostToDevice, st)); }
	CHECK(ensure(c, R.names, name_bytes + 16)); CHECK(ensure(c, R.name_off, (N + 1) * 8));
	HIPCHECK(c, hipMemcpyAsync(R.names.p, names, name_bytes, hipMemcpyHostToDevice, st));
	HIPCHECK(c, hipMemsetAsync(P<char>(R.names) + name_bytes, 0, 16, st));
	HIPCHECK(c, hipMemcpyAsync(R.name_off.p, name_off, (N + 1) * 8, hipMemcpyHostToDevice, st));
	for (DBuf *b : {&R.row_n, &R.op_n, &R.sq_n, &R.row_at, &R.op_at}) CHECK(ensure(c, *b, N * 4 + 16));
	CHECK(ensure(c, R.sq_at, N * 8 + 16)); CHECK(ensure(c, R.rows_small, 64));
	CHECK(ensure(c, c->scan_scratch, (size_t)scan_scratch_elems(n) * 8 + 64)); CHECK(ensure(c, c->scan_scratch64, (size_t)scan_scratch_elems(n) * 8 + 64));
	// R.rows_small: [0] records, [1] operations, [2..3] seqqual bytes u64
	uint32_t *sm = P<uint32_t>(R.rows_small);
	{
		ProfScope ps(c, P_REALIGN_ROWS, n);
		k_rr_sizes<<<grid_for(n, BLOCK), BLOCK, 0, st>>>(P<uint64_t>(R.offs), P<RaHit>(R.hits), P<RaHit>(R.mates), n, P<uint32_t>(R.row_n), P<uint32_t>(R.op_n), P<uint32_t>(R.sq_n));
		exclusive_scan<uint32_t, uint32_t>(st, P<uint32_t>(R.row_n), P<uint32_t>(R.row_at), n, 0u, P<uint32_t>(c->scan_scratch), sm);
		exclusive_scan<uint32_t, uint32_t>(st, P<uint32_t>(R.op_n), P<uint32_t>(R.op_at), n, 0u, P<uint32_t>(c->scan_scratch), sm + 1);
		exclusive_scan<uint32_t, uint64_t>(st, P<uint32_t>(R.sq_n), P<uint64_t>(R.sq_at), n, 0ull, P<uint64_t>(c->scan_scratch64), reinterpret_cast<uint64_t *>(sm + 2));
	}
	HIPCHECK(c, hipGetLastError());
	uint32_t tot[4];
	HIPCHECK(c, hipMemcpyAsync(tot, R.rows_small.p, 16, hipMemcpyDeviceToHost, st));
	HIPCHECK(c, hipStreamSynchronize(st));
	const size_t rows = tot[0], ops = tot[1];
	uint64_t sq_total;
	memcpy(&sq_total, tot + 2, 8);
	if (rows < N || rows > 2 * N || ops > 3 * rows) { c->err = "ssv_realign_split_batch: the sizes do not add up"; return SSV_E_STATE; }
	CHECK(R.row_cols.reserve(c, rows, 1.0)); CHECK(R.row_cols.reserve_variable(c, ops, (size_t)sq_total, 1.0)); // (64 bytes of slack behind seqqual: 8 must be readable)
	CHECK(ensure(c, R.row_rec, rows * sizeof(ssv_record) + 64)); CHECK(ensure(c, R.row_name, rows * 8 + 16));
	const RaRowsArgs a{P<char>(R.seqs), quals ? P<char>(R.quals) : nullptr, P<uint64_t>(R.offs), P<uint64_t>(R.name_off), P<RaHit>(R.hits), P<RaHit>(R.mates), n,
	                   P<uint32_t>(R.row_at), P<uint32_t>(R.op_at), P<uint64_t>(R.sq_at)};
	{
		ProfScope ps(c, P_REALIGN_ROWS, (int64_t)rows);
		k_rr_rows<<<grid_for(n, WAVES_PER_BLOCK), BLOCK, 0, st>>>(a, R.row_cols.view(), P<ssv_record>(R.row_rec), P<uint64_t>(R.row_name));
	}
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipStreamSynchronize(st));
	R.row_cols.fill(out, (int64_t)rows, (int64_t)ops, (int64_t)sq_total);
	out->rec = P<ssv_record>(R.row_rec);
	out_names->base = P<char>(R.names); out_names->off = P<uint64_t>(R.row_name); out_names->bytes = (int64_t)name_bytes;
	return SSV_OK;
}

int ssv_realign_free(ssv_ctx *c)
{
	if (!c) return SSV_E_ARG;
	HIPCHECK(c, hipSetDevice(c->device));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	c->ra.reset();
	return SSV_OK;
}
