// readthrough_api.inc - C ABI of `getsv -F` (FindJunction, process_bwasw.cpp:5-227), of `run -A` (the same session over the original's own split reads:
// ssv_rt_begin_original) and of `run -A -S` (that session with virtual candidates from SA tags: ssv_rt_begin_original_sa); included by seeksv_hip.hip, kernels
// in readthrough_kernels.h, splitread_kernels.h and splitread_sa_kernels.h

static_assert(sizeof(ssv::RtPairOut) == sizeof(ssv_rt_pair), "RtPairOut is the ABI line");

struct ssv_rt_state {
	enum { IDLE, SCANNING, FINISHED } phase = IDLE;
	int32_t min_mapq = 1, n_targets = 0;
	uint64_t hash_mask = ~0ull;
	int hash_bits = 64;
	bool original = false;                 // ssv_rt_begin_original: the split-read rule (splitread_kernels.h) in the place of FindJunction's selection and key
	bool stats_valid = false;              // a session of that mode has finished
	ssv_rt_original_counts stats{};
	DBuf ostats;                           // that mode's device counters (SR_N_*), zeroed at begin
	bool sa = false;                       // ssv_rt_begin_original_sa: sources also give virtual candidates from their SA tag (splitread_sa_kernels.h)
	bool sa_stats_valid = false;
	ssv_rt_original_sa_counts sa_stats{};
	int64_t n_virtual = 0;                 // virtual candidates among the n_cand of the store
	DBuf sa_counts;                        // SA_N_*, zeroed at begin
	DBuf ct_hash, ct_tid, ct_off, ct_names; // the contig table (SaContigs), built at begin
	uint64_t ct_mask = ~0ull;
	DBuf virt, ax_base, ax_off, ax_len;    // per batch: k_sa_parse's lines; a host descriptor's copy
	uint64_t rec_base = 0;                 // records scanned so far (file order)
	int64_t n_cand = 0;                    // candidates gathered so far
	uint64_t name_used = 0, seq_used = 0, cig_used = 0;
	DBuf rank, keep, at, cand, nbytes, sbytes, cops, small, hnames, hoff;
	DBuf cands, hash, names, seqs, cigs;   // the store: grows like the other arenas, contents kept
	DBuf keys[2], vals[2], held, partner, ev_flag, ev_at, ev_b, pairs, slices, cig_src, pseq, pcig, seq_out, cig_out;
	HBuf h_small, h_pairs, h_seqs, h_cigs;
};

// the mode's counters, and the contig table: the names hashed (SSV_SA_CONTIG_HASH_BITS cuts the hash for tests, as SSV_RT_HASH_BITS does the read names'),
// sorted by (hash, tid) on the host - once per session, a header's worth of names - and uploaded with the names' bytes
static int sa_begin(ssv_ctx *c, ssv_rt_state &R, int32_t nt, const char *const *target_names)
{
	CHECK(ensure(c, R.sa_counts, SA_N_STATS * 8));
	HIPCHECK(c, hipMemsetAsync(R.sa_counts.p, 0, SA_N_STATS * 8, c->st));
	R.ct_mask = env_low_bits_mask("SSV_SA_CONTIG_HASH_BITS");
	std::vector<uint64_t> off((size_t)nt + 1, 0);
	for (int32_t t = 0; t < nt; ++t) off[(size_t)t + 1] = off[(size_t)t] + strlen(target_names[t]);
	std::vector<uint8_t> blob((size_t)off[(size_t)nt] + 1);
	std::vector<std::pair<uint64_t, uint32_t>> keyed((size_t)nt);
	for (int32_t t = 0; t < nt; ++t) {
		const uint32_t len = (uint32_t)(off[(size_t)t + 1] - off[(size_t)t]);
		memcpy(blob.data() + off[(size_t)t], target_names[t], len);
		keyed[(size_t)t] = {sa_name_hash(blob.data() + off[(size_t)t], len) & R.ct_mask, (uint32_t)t};
	}
	std::sort(keyed.begin(), keyed.end());
	std::vector<uint64_t> hs((size_t)nt + 1);
	std::vector<uint32_t> ts((size_t)nt + 1);
	for (int32_t k = 0; k < nt; ++k) { hs[(size_t)k] = keyed[(size_t)k].first; ts[(size_t)k] = keyed[(size_t)k].second; }
	CHECK(ensure(c, R.ct_hash, hs.size() * 8)); CHECK(ensure(c, R.ct_tid, ts.size() * 4)); CHECK(ensure(c, R.ct_off, off.size() * 8)); CHECK(ensure(c, R.ct_names, blob.size()));
	HIPCHECK(c, hipMemcpyAsync(R.ct_hash.p, hs.data(), hs.size() * 8, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemcpyAsync(R.ct_tid.p, ts.data(), ts.size() * 4, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemcpyAsync(R.ct_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemcpyAsync(R.ct_names.p, blob.data(), blob.size(), hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st)); // (the vectors go)
	return SSV_OK;
}

static int rt_begin(ssv_ctx *c, const ssv_rt_params *p, bool original, bool sa = false, const char *const *target_names = nullptr)
{
	if (!c) return SSV_E_ARG;
	if (!p || p->n_targets < 0 || (p->n_targets > 0 && !p->name_rank)) { c->err = sa ? "ssv_rt_begin_original_sa: bad parameters" : original ? "ssv_rt_begin_original: bad parameters" : "ssv_rt_begin: bad parameters"; return SSV_E_ARG; }
	if (sa && p->n_targets > 0 && !target_names) { c->err = "ssv_rt_begin_original_sa: no contig names"; return SSV_E_ARG; }
	for (int32_t t = 0; sa && t < p->n_targets; ++t) if (!target_names[t]) { c->err = "ssv_rt_begin_original_sa: a contig without a name"; return SSV_E_ARG; }
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->rt) c->rt.reset(new ssv_rt_state());
	ssv_rt_state &R = *c->rt;
	R.phase = ssv_rt_state::IDLE;
	R.original = original; R.stats_valid = false;
	R.sa = sa; R.sa_stats_valid = false; R.n_virtual = 0;
	if (sa) CHECK(sa_begin(c, R, p->n_targets, target_names));
	if (original) {
		CHECK(ensure(c, R.ostats, SR_N_STATS * 8));
		HIPCHECK(c, hipMemsetAsync(R.ostats.p, 0, SR_N_STATS * 8, c->st));
	}
	R.min_mapq = p->min_mapq; R.n_targets = p->n_targets;
	// SSV_RT_HASH_BITS (tests): the name hash cut to its low bits, so that names collide and the exact path runs
	R.hash_mask = env_low_bits_mask("SSV_RT_HASH_BITS", &R.hash_bits);
	R.rec_base = 0; R.n_cand = 0; R.name_used = R.seq_used = R.cig_used = 0;
	CHECK(ensure(c, R.rank, (size_t)p->n_targets * 4 + 16));
	if (p->n_targets) HIPCHECK(c, hipMemcpyAsync(R.rank.p, p->name_rank, (size_t)p->n_targets * 4, hipMemcpyHostToDevice, c->st));
	CHECK(ensure(c, R.small, 256)); CHECK(ensure_host(c, R.h_small, 256));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	R.phase = ssv_rt_state::SCANNING;
	return SSV_OK;
}

int ssv_rt_begin(ssv_ctx *c, const ssv_rt_params *p) { return rt_begin(c, p, false); }
int ssv_rt_begin_original(ssv_ctx *c, const ssv_rt_params *p) { return rt_begin(c, p, true); }
int ssv_rt_begin_original_sa(ssv_ctx *c, const ssv_rt_params *p, const char *const *target_names) { return rt_begin(c, p, true, true, target_names); }

int ssv_rt_original_sa_stats(ssv_ctx *c, ssv_rt_original_sa_counts *out)
{
	if (!c) return SSV_E_ARG;
	if (!c->rt || !c->rt->sa_stats_valid || c->rt->phase != ssv_rt_state::FINISHED) { c->err = "ssv_rt_original_sa_stats without a finished ssv_rt_begin_original_sa session"; return SSV_E_STATE; }
	if (!out) { c->err = "ssv_rt_original_sa_stats: no result"; return SSV_E_ARG; }
	*out = c->rt->sa_stats;
	return SSV_OK;
}

int ssv_rt_original_stats(ssv_ctx *c, ssv_rt_original_counts *out)
{
	if (!c) return SSV_E_ARG;
	if (!c->rt || !c->rt->stats_valid || c->rt->phase != ssv_rt_state::FINISHED) { c->err = "ssv_rt_original_stats without a finished ssv_rt_begin_original session"; return SSV_E_STATE; }
	if (!out) { c->err = "ssv_rt_original_stats: no result"; return SSV_E_ARG; }
	*out = c->rt->stats;
	return SSV_OK;
}

// The gather of a batch's m candidates in a session of ssv_rt_begin_original_sa: k_sa_parse gives every candidate one slot of the store, or two when it is a
// source with a virtual candidate; sizes, offsets and copies are ssv_rt_scan's, by slot.
static int sa_scan_candidates(ssv_ctx *c, ssv_rt_state &R, const DevBatch &d, const DevNames &names, const ssv_aux_t *aux, int64_t m)
{
	DevAux ax{aux->base, aux->off, aux->len, aux->encoding == SSV_AUX_SAM ? SA_ENC_SAM : SA_ENC_BAM};
	if (aux->mem == SSV_MEM_HOST) {
		CHECK(ensure(c, R.ax_base, (size_t)aux->bytes + 16)); CHECK(ensure(c, R.ax_off, (size_t)d.n * 8 + 16)); CHECK(ensure(c, R.ax_len, (size_t)d.n * 4 + 16));
		if (aux->bytes) HIPCHECK(c, hipMemcpyAsync(R.ax_base.p, aux->base, (size_t)aux->bytes, hipMemcpyHostToDevice, c->st));
		HIPCHECK(c, hipMemcpyAsync(R.ax_off.p, aux->off, (size_t)d.n * 8, hipMemcpyHostToDevice, c->st));
		HIPCHECK(c, hipMemcpyAsync(R.ax_len.p, aux->len, (size_t)d.n * 4, hipMemcpyHostToDevice, c->st));
		ax.base = P<uint8_t>(R.ax_base); ax.off = P<uint64_t>(R.ax_off); ax.len = P<uint32_t>(R.ax_len);
	}
	const SaContigs T{P<uint64_t>(R.ct_hash), P<uint32_t>(R.ct_tid), P<uint64_t>(R.ct_off), P<uint8_t>(R.ct_names), (int64_t)R.n_targets, R.ct_mask};
	uint32_t *sm = P<uint32_t>(R.small);
	uint32_t *slots = P<uint32_t>(R.keep), *slot_at = P<uint32_t>(R.at); // (select's two columns are free behind the compaction; m <= n)
	CHECK(ensure(c, R.virt, (size_t)m * sizeof(SaVirt) + 64));
	k_sa_parse<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(d, ax, T, P<uint32_t>(R.cand), m, R.min_mapq, P<SaVirt>(R.virt), slots, P<unsigned long long>(R.sa_counts));
	HIPCHECK(c, hipGetLastError());
	exclusive_scan<uint32_t, uint32_t>(c->st, slots, slot_at, m, 0u, P<uint32_t>(c->scan_scratch), sm + 4);
	HIPCHECK(c, hipMemcpyAsync(P<uint32_t>(R.h_small) + 4, sm + 4, 4, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const int64_t m2 = P<uint32_t>(R.h_small)[4];
	if (R.n_cand + m2 >= (int64_t)0xffffffffll) { c->err = "more than 2^32 read-through candidates"; return SSV_E_RANGE; }
	const size_t M1 = (size_t)m2 + 1;
	CHECK(ensure(c, R.nbytes, M1 * 8)); CHECK(ensure(c, R.sbytes, M1 * 8)); CHECK(ensure(c, R.cops, M1 * 8));
	CHECK(ensure(c, c->scan_scratch64, scan_scratch_elems(m2) * 8));
	CHECK(ensure(c, R.hash, (size_t)(R.n_cand + m2) * 8 + 16, true, (size_t)R.n_cand * 8));
	CHECK(ensure(c, R.cands, (size_t)(R.n_cand + m2) * sizeof(RtCand) + 64, true, (size_t)R.n_cand * sizeof(RtCand)));
	k_sa_measure<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(d, names, P<uint32_t>(R.cand), m, slot_at, slots, P<SaVirt>(R.virt), R.hash_mask, P<uint64_t>(R.nbytes), P<uint64_t>(R.sbytes),
	                                                      P<uint64_t>(R.cops), P<uint64_t>(R.hash) + R.n_cand);
	HIPCHECK(c, hipGetLastError());
	exclusive_scan<uint64_t, uint64_t>(c->st, P<uint64_t>(R.nbytes), P<uint64_t>(R.nbytes), m2, (uint64_t)R.name_used, P<uint64_t>(c->scan_scratch64), P<uint64_t>(R.nbytes) + m2);
	exclusive_scan<uint64_t, uint64_t>(c->st, P<uint64_t>(R.sbytes), P<uint64_t>(R.sbytes), m2, (uint64_t)R.seq_used, P<uint64_t>(c->scan_scratch64), P<uint64_t>(R.sbytes) + m2);
	exclusive_scan<uint64_t, uint64_t>(c->st, P<uint64_t>(R.cops), P<uint64_t>(R.cops), m2, (uint64_t)R.cig_used, P<uint64_t>(c->scan_scratch64), P<uint64_t>(R.cops) + m2);
	HIPCHECK(c, hipMemcpyAsync(P<uint64_t>(R.h_small) + 4, P<uint64_t>(R.nbytes) + m2, 8, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipMemcpyAsync(P<uint64_t>(R.h_small) + 5, P<uint64_t>(R.sbytes) + m2, 8, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipMemcpyAsync(P<uint64_t>(R.h_small) + 6, P<uint64_t>(R.cops) + m2, 8, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const uint64_t name_end = P<uint64_t>(R.h_small)[4], seq_end = P<uint64_t>(R.h_small)[5], cig_end = P<uint64_t>(R.h_small)[6];
	CHECK(ensure(c, R.names, name_end + 16, true, R.name_used));
	CHECK(ensure(c, R.seqs, seq_end + 16, true, R.seq_used));
	CHECK(ensure(c, R.cigs, cig_end * 4 + 16, true, R.cig_used * 4));
	k_sa_gather<<<grid_for(m, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(d, names, P<uint32_t>(R.cand), m, slot_at, slots, P<SaVirt>(R.virt), R.rec_base, (uint64_t)R.n_cand, P<uint64_t>(R.nbytes),
	                                                               P<uint64_t>(R.sbytes), P<uint64_t>(R.cops), P<RtCand>(R.cands) + R.n_cand, P<char>(R.names), P<uint8_t>(R.seqs),
	                                                               P<uint32_t>(R.cigs), P<unsigned long long>(R.ostats));
	HIPCHECK(c, hipGetLastError());
	R.n_cand += m2; R.n_virtual += m2 - m; R.name_used = name_end; R.seq_used = seq_end; R.cig_used = cig_end;
	return SSV_OK;
}

static int rt_scan(ssv_ctx *c, const ssv_batch_t *b, const ssv_names_t *nm, const ssv_aux_t *aux);

int ssv_rt_scan(ssv_ctx *c, const ssv_batch_t *b, const ssv_names_t *nm)
{
	if (c && c->rt && c->rt->phase == ssv_rt_state::SCANNING && c->rt->sa) { c->err = "ssv_rt_scan: a session of ssv_rt_begin_original_sa takes its batches through ssv_rt_scan_aux"; return SSV_E_STATE; }
	return rt_scan(c, b, nm, nullptr);
}

// a descriptor belongs to the batch when it describes as many records; a host descriptor's spans must lie inside its bytes
static int check_aux(ssv_ctx *c, const ssv_aux_t *aux, int64_t n)
{
	const char *bad = nullptr;
	if (!aux) bad = "no descriptor of the optional fields";
	else if (aux->n != n) bad = "the descriptor does not belong to the batch (another number of records)";
	else if (aux->mem != SSV_MEM_HOST && aux->mem != SSV_MEM_DEVICE) bad = "bad aux.mem";
	else if (aux->encoding != SSV_AUX_BAM && aux->encoding != SSV_AUX_SAM) bad = "bad aux.encoding";
	else if (n > 0 && (!aux->off || !aux->len || (!aux->base && (aux->mem == SSV_MEM_DEVICE || aux->bytes > 0)))) bad = "a batch with records needs base, off and len";
	else if (aux->mem == SSV_MEM_HOST && aux->bytes < 0) bad = "aux.bytes below 0";
	else if (aux->mem == SSV_MEM_HOST)
		for (int64_t i = 0; i < n && !bad; ++i) if (aux->off[i] > (uint64_t)aux->bytes || aux->len[i] > (uint64_t)aux->bytes - aux->off[i]) bad = "a record's optional fields lie outside aux.bytes";
	if (!bad) return SSV_OK;
	c->err = std::string("ssv_rt_scan_aux: ") + bad;
	return SSV_E_ARG;
}

int ssv_rt_scan_aux(ssv_ctx *c, const ssv_batch_t *b, const ssv_names_t *nm, const ssv_aux_t *aux)
{
	if (!c) return SSV_E_ARG;
	if (!c->rt || c->rt->phase != ssv_rt_state::SCANNING || !c->rt->sa) { c->err = "ssv_rt_scan_aux outside a session of ssv_rt_begin_original_sa"; return SSV_E_STATE; }
	if (!b || !nm) { c->err = "ssv_rt_scan_aux: no batch or no names"; return SSV_E_ARG; }
	CHECK(check_aux(c, aux, b->n));
	return rt_scan(c, b, nm, aux);
}

static int rt_scan(ssv_ctx *c, const ssv_batch_t *b, const ssv_names_t *nm, const ssv_aux_t *aux)
{
	if (!c) return SSV_E_ARG;
	if (!c->rt || c->rt->phase != ssv_rt_state::SCANNING) { c->err = "ssv_rt_scan before ssv_rt_begin"; return SSV_E_STATE; }
	if (!b || !nm) { c->err = "ssv_rt_scan: no batch or no names"; return SSV_E_ARG; }
	CHECK(check_names(c, nm, b->n, "ssv_rt_scan"));
	ssv_rt_state &R = *c->rt;
	HIPCHECK(c, hipSetDevice(c->device));
	DevBatch d;
	CHECK(stage_batch(c, b, d));
	const int64_t n = d.n;
	if (n == 0) return SSV_OK;
	ProfScope ps(c, R.sa ? P_SPLITREAD_SA_SCAN : R.original ? P_SPLITREAD_SCAN : P_RT_SCAN, n);
	CHECK(staged_ends(c, d));
	DevNames names;
	CHECK(stage_names(c, nm, n, R.hnames, R.hoff, names));
	// ---- select: the ends column (and behind a passing pair the flag / mapq of the line) -> ordered compaction ----
	CHECK(ensure(c, R.keep, (size_t)n * 4 + 16)); CHECK(ensure(c, R.at, (size_t)n * 4 + 16)); CHECK(ensure(c, R.cand, (size_t)n * 4 + 16));
	CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(n) * 4)); CHECK(ensure(c, c->scan_scratch64, scan_scratch_elems(n) * 8));
	uint32_t *sm = P<uint32_t>(R.small);
	HIPCHECK(c, hipMemsetAsync(R.small.p, 0, 256, c->st));
	if (R.original) k_sr_select<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(d, R.min_mapq, R.n_targets, P<uint32_t>(R.keep));
	else k_rt_select<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(d, R.min_mapq, R.n_targets, P<uint32_t>(R.keep));
	exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(R.keep), P<uint32_t>(R.at), n, 0u, P<uint32_t>(c->scan_scratch), sm);
	k_rt_place<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(P<uint32_t>(R.keep), P<uint32_t>(R.at), n, P<uint32_t>(R.cand));
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipMemcpyAsync(R.h_small.p, R.small.p, 16, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const int64_t m = P<uint32_t>(R.h_small)[0];
	if (m > 0 && R.sa) { CHECK(sa_scan_candidates(c, R, d, names, aux, m)); }
	else if (m > 0) {
		if (R.n_cand + m >= (int64_t)0xffffffffll) { c->err = "more than 2^32 read-through candidates"; return SSV_E_RANGE; }
		// ---- gather: sizes -> offsets in the store (carried over the batches) -> copies ----
		const size_t M1 = (size_t)m + 1;
		CHECK(ensure(c, R.nbytes, M1 * 8)); CHECK(ensure(c, R.sbytes, M1 * 8)); CHECK(ensure(c, R.cops, M1 * 8));
		CHECK(ensure(c, R.hash, (size_t)(R.n_cand + m) * 8 + 16, true, (size_t)R.n_cand * 8));
		CHECK(ensure(c, R.cands, (size_t)(R.n_cand + m) * sizeof(RtCand) + 64, true, (size_t)R.n_cand * sizeof(RtCand)));
		if (R.original) k_sr_measure<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(d, names, P<uint32_t>(R.cand), m, R.hash_mask, P<uint64_t>(R.nbytes), P<uint64_t>(R.sbytes), P<uint64_t>(R.cops),
		                                                                      P<uint64_t>(R.hash) + R.n_cand); // (a record without its bases does not carry the read: sm[8] stays 0)
		else k_rt_measure<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(d, names, P<uint32_t>(R.cand), m, R.hash_mask, P<uint64_t>(R.nbytes), P<uint64_t>(R.sbytes), P<uint64_t>(R.cops),
		                                                           P<uint64_t>(R.hash) + R.n_cand, sm + 8);
		HIPCHECK(c, hipGetLastError());
		exclusive_scan<uint64_t, uint64_t>(c->st, P<uint64_t>(R.nbytes), P<uint64_t>(R.nbytes), m, (uint64_t)R.name_used, P<uint64_t>(c->scan_scratch64), P<uint64_t>(R.nbytes) + m);
		exclusive_scan<uint64_t, uint64_t>(c->st, P<uint64_t>(R.sbytes), P<uint64_t>(R.sbytes), m, (uint64_t)R.seq_used, P<uint64_t>(c->scan_scratch64), P<uint64_t>(R.sbytes) + m);
		exclusive_scan<uint64_t, uint64_t>(c->st, P<uint64_t>(R.cops), P<uint64_t>(R.cops), m, (uint64_t)R.cig_used, P<uint64_t>(c->scan_scratch64), P<uint64_t>(R.cops) + m);
		HIPCHECK(c, hipMemcpyAsync(P<uint64_t>(R.h_small) + 4, P<uint64_t>(R.nbytes) + m, 8, hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipMemcpyAsync(P<uint64_t>(R.h_small) + 5, P<uint64_t>(R.sbytes) + m, 8, hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipMemcpyAsync(P<uint64_t>(R.h_small) + 6, P<uint64_t>(R.cops) + m, 8, hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipMemcpyAsync(P<uint32_t>(R.h_small) + 16, sm + 8, 4, hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
		if (P<uint32_t>(R.h_small)[16]) { c->err = "ssv_rt_scan: a kept record comes without its bases (read the file with keep_all_seq)"; return SSV_E_ARG; }
		const uint64_t name_end = P<uint64_t>(R.h_small)[4], seq_end = P<uint64_t>(R.h_small)[5], cig_end = P<uint64_t>(R.h_small)[6];
		CHECK(ensure(c, R.names, name_end + 16, true, R.name_used));
		CHECK(ensure(c, R.seqs, seq_end + 16, true, R.seq_used));
		CHECK(ensure(c, R.cigs, cig_end * 4 + 16, true, R.cig_used * 4));
		if (R.original) k_sr_gather<<<grid_for(m, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(d, names, P<uint32_t>(R.cand), m, R.rec_base, P<uint64_t>(R.nbytes), P<uint64_t>(R.sbytes), P<uint64_t>(R.cops),
		                                                                               P<RtCand>(R.cands) + R.n_cand, P<char>(R.names), P<uint8_t>(R.seqs), P<uint32_t>(R.cigs),
		                                                                               P<unsigned long long>(R.ostats));
		else k_rt_gather<<<grid_for(m, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(d, names, P<uint32_t>(R.cand), m, R.rec_base, P<uint64_t>(R.nbytes), P<uint64_t>(R.sbytes), P<uint64_t>(R.cops),
		                                                                    P<RtCand>(R.cands) + R.n_cand, P<char>(R.names), P<uint8_t>(R.seqs), P<uint32_t>(R.cigs));
		HIPCHECK(c, hipGetLastError());
		R.n_cand += m; R.name_used = name_end; R.seq_used = seq_end; R.cig_used = cig_end;
	}
	R.rec_base += (uint64_t)n;
	HIPCHECK(c, hipStreamSynchronize(c->st)); // the caller may reuse the batch (and its names) once this returns
	return SSV_OK;
}

// The candidate store and the finish temporaries hold every kept record's line, name, bases and CIGAR (GBs for a large -F file): handed back once the
// results are in host memory - the passes that follow on the same context (insert sizes, discordant pairs, depth) get that memory.
static void rt_release_store(ssv_ctx *c)
{
	ssv_rt_state &R = *c->rt;
	(void)hipStreamSynchronize(c->st);
	for (DBuf *b : {&R.keep, &R.at, &R.cand, &R.nbytes, &R.sbytes, &R.cops, &R.hnames, &R.hoff, &R.cands, &R.hash, &R.names, &R.seqs, &R.cigs,
	                &R.keys[0], &R.keys[1], &R.vals[0], &R.vals[1], &R.held, &R.partner, &R.ev_flag, &R.ev_at, &R.ev_b, &R.pairs, &R.slices, &R.cig_src, &R.pseq, &R.pcig,
	                &R.seq_out, &R.cig_out, &R.virt, &R.ax_base, &R.ax_off, &R.ax_len}) b->reset();
	R.n_cand = 0; R.n_virtual = 0; R.name_used = R.seq_used = R.cig_used = 0;
}

static int rt_finish(ssv_ctx *c, ssv_rt_result *out);

int ssv_rt_finish(ssv_ctx *c, ssv_rt_result *out)
{
	int rc = rt_finish(c, out);
	if (c && c->rt && c->rt->phase == ssv_rt_state::FINISHED) {
		ssv_rt_state &R = *c->rt;
		if (R.original && rc == SSV_OK) { // the session's counts (ssv_rt_original_stats)
			unsigned long long h[SR_N_STATS];
			if (hipMemcpyAsync(h, R.ostats.p, sizeof(h), hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) { c->err = "ssv_rt_finish: the counts did not come back"; rc = SSV_E_HIP; }
			else {
				if (R.sa) {
					unsigned long long g[SA_N_STATS];
					if (hipMemcpyAsync(g, R.sa_counts.p, sizeof(g), hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) { c->err = "ssv_rt_finish: the counts did not come back"; rc = SSV_E_HIP; }
					R.sa_stats.sa_tags = (int64_t)g[SA_N_TAGS]; R.sa_stats.sa_multi = (int64_t)g[SA_N_MULTI]; R.sa_stats.sa_refused = (int64_t)g[SA_N_REFUSED];
					R.sa_stats.virtuals = (int64_t)g[SA_N_VIRTUALS]; R.sa_stats.sa_redundant = (int64_t)g[SA_N_REDUNDANT]; R.sa_stats.pairs_from_sa = (int64_t)g[SA_N_PAIRS];
					R.sa_stats.sa_dropped_length = (int64_t)g[SA_N_LENGTH];
					R.sa_stats_valid = rc == SSV_OK;
				}
				R.stats.candidates = out->n_candidates; R.stats.hard_clipped = (int64_t)h[SR_N_HARD]; R.stats.pairs = out->n_pairs; R.stats.pairs_borrowed = (int64_t)h[SR_N_BORROWED];
				R.stats.dropped_no_carrier = (int64_t)h[SR_N_NO_CARRIER]; R.stats.dropped_length = (int64_t)h[SR_N_LENGTH];
				R.stats.store_bytes = (int64_t)(R.n_cand * (int64_t)(sizeof(RtCand) + 8) + (int64_t)R.name_used + (int64_t)R.seq_used + (int64_t)R.cig_used * 4);
				R.stats_valid = true;
			}
		}
		rt_release_store(c);
	}
	return rc;
}

static int rt_finish(ssv_ctx *c, ssv_rt_result *out)
{
	if (!c) return SSV_E_ARG;
	if (!c->rt || c->rt->phase != ssv_rt_state::SCANNING) { c->err = "ssv_rt_finish before ssv_rt_begin"; return SSV_E_STATE; }
	if (!out) { c->err = "ssv_rt_finish: no result"; return SSV_E_ARG; }
	ssv_rt_state &R = *c->rt;
	HIPCHECK(c, hipSetDevice(c->device));
	memset(out, 0, sizeof(*out));
	const int64_t n = R.n_cand;
	out->n_candidates = n - R.n_virtual; // (kept records: a virtual candidate is none)
	R.phase = ssv_rt_state::FINISHED;
	if (n == 0) return SSV_OK;
	ProfScope ps(c, R.sa ? P_SPLITREAD_SA_FINISH : R.original ? P_SPLITREAD_FINISH : P_RT_FINISH, n);
	// ---- pair: stable sort of (hash, candidate) - candidates are in file order - then one lane per run of equal hashes ----
	const size_t N = (size_t)n;
	CHECK(ensure(c, R.keys[0], N * 8 + 16)); CHECK(ensure(c, R.keys[1], N * 8 + 16)); CHECK(ensure(c, R.vals[0], N * 4 + 16)); CHECK(ensure(c, R.vals[1], N * 4 + 16));
	const int64_t nt = rs_tiles(n);
	CHECK(ensure(c, c->ghist, (size_t)256 * nt * 4)); CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(256 * nt) * 4));
	HIPCHECK(c, hipMemcpyAsync(R.keys[0].p, R.hash.p, N * 8, hipMemcpyDeviceToDevice, c->st));
	k_iota<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(P<uint32_t>(R.vals[0]), n);
	uint64_t *kp[2] = {P<uint64_t>(R.keys[0]), P<uint64_t>(R.keys[1])};
	uint32_t *vp[2] = {P<uint32_t>(R.vals[0]), P<uint32_t>(R.vals[1])};
	const int cur = radix_sort_pairs(c->st, kp, vp, n, (R.hash_bits + 7) / 8 * 8, P<uint32_t>(c->ghist), P<uint32_t>(c->scan_scratch));
	CHECK(ensure(c, R.held, N * 4 + 16)); CHECK(ensure(c, R.partner, N * 4 + 16));
	HIPCHECK(c, hipMemsetAsync(R.partner.p, 0xff, N * 4, c->st));
	if (R.sa) k_sa_pair<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(kp[cur], vp[cur], n, P<RtCand>(R.cands), P<char>(R.names), P<int32_t>(R.held), P<int32_t>(R.partner), P<unsigned long long>(R.ostats),
	                                                          P<unsigned long long>(R.sa_counts));
	else if (R.original) k_sr_pair<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(kp[cur], vp[cur], n, P<RtCand>(R.cands), P<char>(R.names), P<int32_t>(R.held), P<int32_t>(R.partner), P<unsigned long long>(R.ostats));
	else k_rt_pair<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(kp[cur], vp[cur], n, P<RtCand>(R.cands), P<char>(R.names), P<int32_t>(R.held), P<int32_t>(R.partner));
	HIPCHECK(c, hipGetLastError());
	// ---- pair events in the order of their completing record ----
	CHECK(ensure(c, R.ev_flag, N * 4 + 16)); CHECK(ensure(c, R.ev_at, N * 4 + 16)); CHECK(ensure(c, R.ev_b, N * 4 + 16));
	CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(n) * 4)); CHECK(ensure(c, c->scan_scratch64, scan_scratch_elems(n) * 8));
	uint32_t *sm = P<uint32_t>(R.small);
	HIPCHECK(c, hipMemsetAsync(R.small.p, 0, 256, c->st));
	k_rt_flag_pairs<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(P<int32_t>(R.partner), n, P<uint32_t>(R.ev_flag));
	exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(R.ev_flag), P<uint32_t>(R.ev_at), n, 0u, P<uint32_t>(c->scan_scratch), sm);
	k_rt_place<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(P<uint32_t>(R.ev_flag), P<uint32_t>(R.ev_at), n, P<uint32_t>(R.ev_b));
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipMemcpyAsync(R.h_small.p, R.small.p, 16, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const int64_t m = P<uint32_t>(R.h_small)[0];
	out->n_pairs = m;
	if (m == 0) return SSV_OK;
	// ---- per event: key, microhomology, seqs as slices; then the seqs in ASCII and the CIGAR sources ----
	const size_t M = (size_t)m, M1 = M + 1;
	CHECK(ensure(c, R.pairs, M * sizeof(RtPairOut) + 64)); CHECK(ensure(c, R.slices, M * 2 * sizeof(RtSlice) + 64)); CHECK(ensure(c, R.cig_src, M * 8 + 16));
	CHECK(ensure(c, R.pseq, M1 * 8)); CHECK(ensure(c, R.pcig, M1 * 8));
	k_rt_keys<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(P<uint32_t>(R.ev_b), P<int32_t>(R.partner), m, P<RtCand>(R.cands), P<int32_t>(R.rank), P<RtPairOut>(R.pairs),
	                                                   P<RtSlice>(R.slices), P<uint32_t>(R.cig_src), P<uint64_t>(R.pseq), P<uint64_t>(R.pcig));
	if (R.original) k_sr_borrow<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(P<uint32_t>(R.ev_b), P<int32_t>(R.partner), m, P<RtCand>(R.cands), P<RtSlice>(R.slices), P<unsigned long long>(R.ostats));
	HIPCHECK(c, hipGetLastError());
	exclusive_scan<uint64_t, uint64_t>(c->st, P<uint64_t>(R.pseq), P<uint64_t>(R.pseq), m, 0ull, P<uint64_t>(c->scan_scratch64), P<uint64_t>(R.pseq) + m);
	exclusive_scan<uint64_t, uint64_t>(c->st, P<uint64_t>(R.pcig), P<uint64_t>(R.pcig), m, 0ull, P<uint64_t>(c->scan_scratch64), P<uint64_t>(R.pcig) + m);
	HIPCHECK(c, hipMemcpyAsync(P<uint64_t>(R.h_small) + 4, P<uint64_t>(R.pseq) + m, 8, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipMemcpyAsync(P<uint64_t>(R.h_small) + 5, P<uint64_t>(R.pcig) + m, 8, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const uint64_t seq_total = P<uint64_t>(R.h_small)[4], cig_total = P<uint64_t>(R.h_small)[5];
	CHECK(ensure(c, R.seq_out, seq_total + 16)); CHECK(ensure(c, R.cig_out, cig_total * 4 + 16));
	k_rt_emit<<<grid_for(m, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(m, P<RtCand>(R.cands), P<uint8_t>(R.seqs), P<uint32_t>(R.cigs), P<RtSlice>(R.slices), P<uint32_t>(R.cig_src),
	                                                             P<uint64_t>(R.pseq), P<uint64_t>(R.pcig), P<RtPairOut>(R.pairs), P<char>(R.seq_out), P<uint32_t>(R.cig_out));
	HIPCHECK(c, hipGetLastError());
	CHECK(ensure_host(c, R.h_pairs, M * sizeof(RtPairOut) + 64)); CHECK(ensure_host(c, R.h_seqs, seq_total + 16)); CHECK(ensure_host(c, R.h_cigs, cig_total * 4 + 16));
	HIPCHECK(c, hipMemcpyAsync(R.h_pairs.p, R.pairs.p, M * sizeof(RtPairOut), hipMemcpyDeviceToHost, c->st));
	if (seq_total) HIPCHECK(c, hipMemcpyAsync(R.h_seqs.p, R.seq_out.p, seq_total, hipMemcpyDeviceToHost, c->st));
	if (cig_total) HIPCHECK(c, hipMemcpyAsync(R.h_cigs.p, R.cig_out.p, cig_total * 4, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	prof_collect(c);
	out->pairs = P<ssv_rt_pair>(R.h_pairs); out->seqs = P<char>(R.h_seqs); out->cigars = P<uint32_t>(R.h_cigs);
	return SSV_OK;
}
