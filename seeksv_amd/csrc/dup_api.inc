// dup_api.inc - C ABI of `run -M` (duplicate read pairs marked while the sample is retained); included by seeksv_hip.hip, kernels in dup_kernels.h

struct ssv_dup_state {
	enum { IDLE, ACTIVE, ENDED } phase = IDLE;
	uint64_t mask = ~0ull;           // SSV_DUP_DIGEST_BITS
	uint64_t emitted = 0;            // records handed out so far: record i of a call's view is record emitted + i of the file
	int64_t entries = 0;             // digests in the set
	ssv_dup_stats st{};
	DBuf set_keys, set_when;         // the digest set: slots + 1 words each (dup_kernels.h DupSet)
	uint64_t slots = 0;
	// the run held back, in two sets of buffers in turn (a call reads one and writes the other)
	struct Hold {
		DBuf tid, pos, ncig, ends, rec, cigar, seq, names, noff;
		int64_t n = 0, cig = 0;
		uint64_t seq_bytes = 0, name_bytes = 0;
		int32_t span = 0;              // max_ref_span of the batches its records came from (0: unknown)
	} hold[2];
	int cur = 0;
	// a call's temporaries
	DBuf sel, at, cand, wave_break, rs, rat, rfirst, keys, rstart, isdup, keeper, fresh, mark, cig_n, cig_at, seq_b, seq_at, name_b, name_at, wave_cnt, wave_part, tmp, hnames, hoff;
	SmallWords small;
};

namespace {

enum DupWord { DW_M, DW_CUT, DW_UNSORTED, DW_BAD, DW_OUT_CIG, DW_OUT_SEQ, DW_HOLD_CIG, DW_HOLD_SEQ, DW_HOLD_NAMES, DW_PART, DW_RUNS, DW_DUPS, DW_GROUPS, DW_FRESH, DW_TAILS, DW_COUNT };
constexpr size_t DUP_SMALL_BYTES = 256;
static_assert(DW_COUNT * 8 <= DUP_SMALL_BYTES, "the small block holds every word");

DupSet dup_set_view(ssv_dup_state &D)
{
	int lg = 0;
	while ((1ull << lg) < D.slots) ++lg;
	return DupSet{P<uint64_t>(D.set_keys), P<uint64_t>(D.set_when), D.slots - 1, 64 - lg};
}

int dup_set_clear(ssv_ctx *c, DBuf &keys, DBuf &when, uint64_t slots)
{
	CHECK(ensure(c, keys, (slots + 1) * 8)); CHECK(ensure(c, when, (slots + 1) * 8));
	HIPCHECK(c, hipMemsetAsync(keys.p, 0, (slots + 1) * 8, c->st));
	HIPCHECK(c, hipMemsetAsync(when.p, 0xff, (slots + 1) * 8, c->st));
	return SSV_OK;
}

// room for `need` digests at half full at the most: doubled, the entries put in again
int dup_set_grow(ssv_ctx *c, ssv_dup_state &D, int64_t need)
{
	uint64_t slots = D.slots;
	while (slots < 2 * (uint64_t)need) slots *= 2;
	if (slots == D.slots) return SSV_OK;
	DBuf keys, when;
	CHECK(dup_set_clear(c, keys, when, slots));
	const DupSet from = dup_set_view(D);
	std::swap(D.set_keys, keys); std::swap(D.set_when, when);
	const uint64_t old = D.slots;
	D.slots = slots;
	k_dup_rehash<<<grid_for((int64_t)old + 1, BLOCK), BLOCK, 0, c->st>>>(from, dup_set_view(D));
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipStreamSynchronize(c->st)); // (the old arrays go with `keys` and `when`)
	return SSV_OK;
}

} // namespace

int ssv_dup_begin(ssv_ctx *c)
{
	if (!c) return SSV_E_ARG;
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->dup) c->dup.reset(new ssv_dup_state());
	ssv_dup_state &D = *c->dup;
	D.phase = ssv_dup_state::IDLE;
	D.mask = env_low_bits_mask("SSV_DUP_DIGEST_BITS"); // (tests) so that digests collide
	const char *e = getenv("SSV_DUP_SET_SLOTS"); // (tests) a small start, so that the set grows
	uint64_t slots = 16;
	const uint64_t want = e ? (uint64_t)std::max<long long>(16, atoll(e)) : (uint64_t)1 << 16;
	while (slots < want) slots *= 2;
	CHECK(dup_set_clear(c, D.set_keys, D.set_when, slots));
	D.slots = slots;
	D.emitted = 0; D.entries = 0; D.st = ssv_dup_stats{};
	for (auto &h : D.hold) { h.n = 0; h.cig = 0; h.seq_bytes = 0; h.name_bytes = 0; h.span = 0; }
	CHECK(D.small.reserve(c, DUP_SMALL_BYTES));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	D.phase = ssv_dup_state::ACTIVE;
	return SSV_OK;
}

int ssv_dup_retain(ssv_ctx *c, const ssv_batch_t *b, const ssv_names_t *nm, int last, ssv_batch_t *out, int64_t *carried)
{
	if (!c) return SSV_E_ARG;
	if (!c->dup || c->dup->phase != ssv_dup_state::ACTIVE) { c->err = "ssv_dup_retain before ssv_dup_begin, or after the last batch"; return SSV_E_STATE; }
	if (!b || !nm || !out || !carried) { c->err = "ssv_dup_retain: NULL argument"; return SSV_E_ARG; }
	if ((b->mem & ~(int)SSV_MEM_PERSISTENT) != SSV_MEM_DEVICE) { c->err = "ssv_dup_retain takes device batches"; return SSV_E_ARG; }
	CHECK(check_names(c, nm, b->n, "ssv_dup_retain"));
	ssv_dup_state &D = *c->dup;
	HIPCHECK(c, hipSetDevice(c->device));
	DevBatch d;
	CHECK(stage_batch(c, b, d));
	CHECK(staged_ends(c, d));
	DevNames names{nullptr, nullptr, 0};
	if (d.n) CHECK(stage_names(c, nm, d.n, D.hnames, D.hoff, names));
	ssv_dup_state::Hold &H = D.hold[D.cur], &H2 = D.hold[D.cur ^ 1];
	DupView v;
	v.a = DevBatch{H.n, P<int32_t>(H.tid), P<int32_t>(H.pos), P<uint16_t>(H.ncig), P<uint8_t>(H.ends), P<ssv_record>(H.rec), P<uint32_t>(H.cigar), P<uint8_t>(H.seq), H.span};
	v.b = d; v.na = DevNames{P<char>(H.names), P<uint64_t>(H.noff), 0}; v.nb = names;
	const int64_t N = v.n = H.n + d.n;
	if (N >= (1ll << 31)) { c->err = "ssv_dup_retain: the hold-back and the batch together exceed 2^31 records"; return SSV_E_RANGE; }
	const size_t n4 = (size_t)N * 4 + 16;
	const int64_t nw = (int64_t)grid_for(N, BLOCK) * WAVES_PER_BLOCK;
	uint64_t *sm = P<uint64_t>(D.small.dev);
	const uint64_t *hs = P<uint64_t>(D.small.host);
	auto w32 = [&](int k) { return reinterpret_cast<uint32_t *>(sm + k); };
	CHECK(D.small.clear(c));
	CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(N + 1) * 4)); CHECK(ensure(c, c->scan_scratch64, scan_scratch_elems(N + 1) * 8));
	uint32_t *sc32 = P<uint32_t>(c->scan_scratch);
	uint64_t *sc64 = P<uint64_t>(c->scan_scratch64);

	// ---- select: records with a neighbour at their position, the start of the trailing run, the order of the input ----
	if (N) {
		ProfScope ps(c, P_DUP_SELECT, N);
		CHECK(ensure(c, D.sel, n4)); CHECK(ensure(c, D.at, n4)); CHECK(ensure(c, D.cand, n4)); CHECK(ensure(c, D.wave_break, (size_t)nw * 4));
		k_dup_select<<<grid_for(N, BLOCK), BLOCK, 0, c->st>>>(v, P<uint32_t>(D.sel), P<int32_t>(D.wave_break), w32(DW_UNSORTED));
		k_dup_cut<<<1, WAVE, 0, c->st>>>(v, P<int32_t>(D.wave_break), nw, w32(DW_CUT));
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(D.sel), P<uint32_t>(D.at), N, 0u, sc32, w32(DW_M));
		k_rt_place<<<grid_for(N, BLOCK), BLOCK, 0, c->st>>>(P<uint32_t>(D.sel), P<uint32_t>(D.at), N, P<uint32_t>(D.cand));
		HIPCHECK(c, hipGetLastError());
	}
	CHECK(D.small.fetch(c));
	if (hs[DW_UNSORTED]) { c->err = "ssv_dup_retain: the records are not coordinate sorted"; return SSV_E_ARG; }
	const int64_t m = (int64_t)hs[DW_M], cut = last ? N : (int64_t)hs[DW_CUT], n_hold = N - cut;

	// ---- what every record takes where it goes (and: does every record that takes part come with its qualities); the runs of the selected records ----
	if (N) {
		ProfScope ps(c, P_DUP_RETAIN, N);
		for (DBuf *x : {&D.cig_n, &D.cig_at, &D.seq_b, &D.name_b}) CHECK(ensure(c, *x, n4));
		CHECK(ensure(c, D.seq_at, (size_t)N * 8 + 16)); CHECK(ensure(c, D.name_at, (size_t)N * 8 + 16));
		CHECK(ensure(c, D.wave_part, (size_t)nw * 4)); CHECK(ensure(c, D.wave_cnt, (size_t)nw * 4)); CHECK(ensure(c, D.tmp, std::max(n4, (size_t)nw * 4)));
		k_dup_sizes<<<grid_for(N, BLOCK), BLOCK, 0, c->st>>>(v, cut, P<uint32_t>(D.cig_n), P<uint32_t>(D.seq_b), P<uint32_t>(D.name_b), P<uint32_t>(D.wave_part), w32(DW_BAD));
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(D.cig_n), P<uint32_t>(D.cig_at), cut, 0u, sc32, w32(DW_OUT_CIG));
		exclusive_scan<uint32_t, uint64_t>(c->st, P<uint32_t>(D.seq_b), P<uint64_t>(D.seq_at), cut, 0ull, sc64, sm + DW_OUT_SEQ);
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(D.cig_n) + cut, P<uint32_t>(D.cig_at) + cut, n_hold, 0u, sc32, w32(DW_HOLD_CIG));
		exclusive_scan<uint32_t, uint64_t>(c->st, P<uint32_t>(D.seq_b) + cut, P<uint64_t>(D.seq_at) + cut, n_hold, 0ull, sc64, sm + DW_HOLD_SEQ);
		exclusive_scan<uint32_t, uint64_t>(c->st, P<uint32_t>(D.name_b) + cut, P<uint64_t>(D.name_at) + cut, n_hold, 0ull, sc64, sm + DW_HOLD_NAMES);
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(D.wave_part), P<uint32_t>(D.tmp), nw, 0u, sc32, w32(DW_PART));
		HIPCHECK(c, hipGetLastError());
	}
	if (m) {
		ProfScope ps(c, P_DUP_MARK, m);
		const size_t m4 = (size_t)m * 4 + 16;
		for (DBuf *x : {&D.rs, &D.rat, &D.rfirst, &D.rstart, &D.isdup, &D.keeper, &D.fresh}) CHECK(ensure(c, *x, m4));
		CHECK(ensure(c, D.keys, (size_t)m * sizeof(DupKey) + 16));
		k_dup_run_starts<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(v, P<uint32_t>(D.cand), m, P<uint32_t>(D.rs));
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(D.rs), P<uint32_t>(D.rat), m, 0u, sc32, w32(DW_RUNS));
		k_rt_place<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(P<uint32_t>(D.rs), P<uint32_t>(D.rat), m, P<uint32_t>(D.rfirst));
		HIPCHECK(c, hipGetLastError());
	}
	CHECK(D.small.fetch(c));
	if (hs[DW_BAD]) { c->err = "ssv_dup_retain: a record that takes part comes without its qualities (decode with keep_all_seq)"; return SSV_E_ARG; }
	const int64_t n_runs = (int64_t)hs[DW_RUNS], out_cig = (int64_t)hs[DW_OUT_CIG], hold_cig = (int64_t)hs[DW_HOLD_CIG], part = (int64_t)hs[DW_PART];
	const uint64_t out_seq = hs[DW_OUT_SEQ], hold_seq = hs[DW_HOLD_SEQ], hold_names = hs[DW_HOLD_NAMES];

	// ---- groups: the heads that are not their group's keeper ----
	if (N) { CHECK(ensure(c, D.mark, (size_t)N + 16)); HIPCHECK(c, hipMemsetAsync(D.mark.p, 0, (size_t)N, c->st)); }
	int64_t n_dup = 0, n_groups = 0;
	if (m) {
		ProfScope ps(c, P_DUP_MARK, m);
		HIPCHECK(c, hipMemsetAsync(D.isdup.p, 0, (size_t)m * 4, c->st)); HIPCHECK(c, hipMemsetAsync(D.keeper.p, 0, (size_t)m * 4, c->st));
		k_dup_keys<<<grid_for(m * DUP_SUB, BLOCK), BLOCK, 0, c->st>>>(v, P<uint32_t>(D.cand), m, cut, D.mask, P<DupKey>(D.keys));
		k_dup_groups<<<grid_for(n_runs, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(P<DupKey>(D.keys), P<uint32_t>(D.cand), P<uint32_t>(D.rfirst), n_runs, m, cut, P<uint32_t>(D.rstart),
		                                                                      P<uint32_t>(D.isdup), P<uint32_t>(D.keeper), P<uint8_t>(D.mark));
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(D.isdup), P<uint32_t>(D.tmp), m, 0u, sc32, w32(DW_DUPS));
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(D.keeper), P<uint32_t>(D.tmp), m, 0u, sc32, w32(DW_GROUPS));
		HIPCHECK(c, hipGetLastError());
		CHECK(D.small.fetch(c));
		n_dup = (int64_t)hs[DW_DUPS]; n_groups = (int64_t)hs[DW_GROUPS];
	}

	// ---- memory: the set, the batch that stays, the next hold-back (the last point where the call can fail and leave everything as it was) ----
	if (n_dup) CHECK(dup_set_grow(c, D, D.entries + n_dup));
	CHECK(ensure(c, H2.tid, (size_t)n_hold * 4 + 16)); CHECK(ensure(c, H2.pos, (size_t)n_hold * 4 + 16)); CHECK(ensure(c, H2.ncig, (size_t)n_hold * 2 + 16)); CHECK(ensure(c, H2.ends, (size_t)n_hold + 16));
	CHECK(ensure(c, H2.rec, (size_t)n_hold * sizeof(ssv_record) + 64)); CHECK(ensure(c, H2.cigar, (size_t)hold_cig * 4 + 64)); CHECK(ensure(c, H2.seq, (size_t)hold_seq + 64));
	CHECK(ensure(c, H2.names, (size_t)hold_names + 16)); CHECK(ensure(c, H2.noff, (size_t)n_hold * 8 + 16));
	RetainedSlab R((size_t)cut, (size_t)out_cig, (size_t)out_seq);
	CHECK(R.take(c));

	// ---- the marked heads' digests into the set; then every settled tail asks it ----
	int64_t n_tail_waves = 0;
	if (n_dup) {
		ProfScope ps(c, P_DUP_MARK, n_dup);
		k_dup_insert<<<grid_for(m, BLOCK), BLOCK, 0, c->st>>>(dup_set_view(D), P<DupKey>(D.keys), P<uint32_t>(D.isdup), P<uint32_t>(D.rstart), m, D.emitted, P<uint32_t>(D.fresh));
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(D.fresh), P<uint32_t>(D.tmp), m, 0u, sc32, w32(DW_FRESH));
		HIPCHECK(c, hipGetLastError());
	}
	if (D.entries + n_dup > 0 && cut > 0) { // (an empty set marks no tail: a stream without duplicates never reads a tail's line or name)
		ProfScope ps(c, P_DUP_MARK, cut);
		n_tail_waves = (int64_t)grid_for(cut, BLOCK) * WAVES_PER_BLOCK;
		k_dup_tails<<<grid_for(cut, BLOCK), BLOCK, 0, c->st>>>(v, cut, dup_set_view(D), D.mask, D.emitted, P<uint32_t>(D.sel), P<uint32_t>(D.at), P<uint32_t>(D.rstart), P<uint8_t>(D.mark),
		                                                       P<uint32_t>(D.wave_cnt));
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(D.wave_cnt), P<uint32_t>(D.tmp), n_tail_waves, 0u, sc32, w32(DW_TAILS));
		HIPCHECK(c, hipGetLastError());
	}

	// ---- gather: the settled records into the slab, the trailing run into the other hold-back ----
	{
		ProfScope ps(c, P_DUP_RETAIN, N);
		if (cut) {
			const DupDst dst{R.dst(), nullptr, nullptr};
			k_dup_gather<<<grid_for(cut * DUP_SUB, BLOCK), BLOCK, 0, c->st>>>(v, 0, cut, P<uint8_t>(D.mark), P<uint32_t>(D.cig_at), P<uint64_t>(D.seq_at), P<uint32_t>(D.seq_b), nullptr, nullptr, 1, dst);
		}
		if (n_hold) {
			const DupDst dst{{P<int32_t>(H2.tid), P<int32_t>(H2.pos), P<uint16_t>(H2.ncig), P<uint8_t>(H2.ends), P<ssv_record>(H2.rec), P<uint32_t>(H2.cigar), P<uint8_t>(H2.seq)}, P<char>(H2.names),
			                 P<uint64_t>(H2.noff)};
			k_dup_gather<<<grid_for(n_hold * DUP_SUB, BLOCK), BLOCK, 0, c->st>>>(v, cut, n_hold, nullptr, P<uint32_t>(D.cig_at), P<uint64_t>(D.seq_at), P<uint32_t>(D.seq_b), P<uint64_t>(D.name_at),
			                                                                    P<uint32_t>(D.name_b), 0, dst);
		}
		HIPCHECK(c, hipGetLastError());
	}
	CHECK(D.small.fetch(c)); // (the source - the decoder's buffers - may be overwritten by the next decode)
	const int32_t span = (H.n && d.n) ? ((H.span && d.max_ref_span) ? std::max(H.span, d.max_ref_span) : 0) : (H.n ? H.span : d.max_ref_span);
	H2.n = n_hold; H2.cig = hold_cig; H2.seq_bytes = hold_seq; H2.name_bytes = hold_names; H2.span = n_hold ? span : 0;
	*carried = cut ? H.n : 0;
	H.n = 0;
	D.cur ^= 1;
	D.emitted += (uint64_t)cut;
	D.entries += n_dup ? (int64_t)hs[DW_FRESH] : 0;
	D.st.records += cut; D.st.taking_part += part; D.st.groups += n_groups; D.st.heads_marked += n_dup; D.st.tails_marked += n_tail_waves ? (int64_t)hs[DW_TAILS] : 0;
	D.st.set_entries = D.entries; D.st.held_max = std::max(D.st.held_max, n_hold);
	if (last) D.phase = ssv_dup_state::ENDED;
	R.hand_out(out, span);
	return SSV_OK;
}

int ssv_dup_finish(ssv_ctx *c, ssv_dup_stats *out)
{
	if (!c) return SSV_E_ARG;
	if (!c->dup || c->dup->phase == ssv_dup_state::IDLE) { c->err = "ssv_dup_finish before ssv_dup_begin"; return SSV_E_STATE; }
	if (!out) { c->err = "ssv_dup_finish: no result"; return SSV_E_ARG; }
	ssv_dup_state &D = *c->dup;
	HIPCHECK(c, hipSetDevice(c->device));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	*out = D.st;
	D.phase = ssv_dup_state::IDLE;
	for (auto &h : D.hold) { h.n = 0; for (DBuf *x : {&h.tid, &h.pos, &h.ncig, &h.ends, &h.rec, &h.cigar, &h.seq, &h.names, &h.noff}) x->reset(); }
	for (DBuf *x : {&D.set_keys, &D.set_when, &D.sel, &D.at, &D.cand, &D.wave_break, &D.rs, &D.rat, &D.rfirst, &D.keys, &D.rstart, &D.isdup, &D.keeper, &D.fresh, &D.mark, &D.cig_n, &D.cig_at, &D.seq_b,
	                &D.seq_at, &D.name_b, &D.name_at, &D.wave_cnt, &D.wave_part, &D.tmp, &D.hnames, &D.hoff}) x->reset(); // (the passes that follow get the memory)
	D.slots = 0;
	prof_collect(c);
	return SSV_OK;
}

// A hook of the tests, not part of the ABI (no declaration in seeksv_hip.h): the record lines of a device batch - a retained one too, whose flags live nowhere
// else - copied to host memory of the caller's, [n] lines.
int ssv_batch_lines_to_host(ssv_ctx *c, const ssv_batch_t *b, ssv_record *lines);
int ssv_batch_lines_to_host(ssv_ctx *c, const ssv_batch_t *b, ssv_record *lines)
{
	if (!c) return SSV_E_ARG;
	if (!b || (b->mem & ~(int)SSV_MEM_PERSISTENT) != SSV_MEM_DEVICE || (b->n > 0 && (!b->rec || !lines))) { c->err = "ssv_batch_lines_to_host: a device batch with record lines"; return SSV_E_ARG; }
	HIPCHECK(c, hipSetDevice(c->device));
	if (b->n > 0) HIPCHECK(c, hipMemcpyAsync(lines, b->rec, (size_t)b->n * sizeof(ssv_record), hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	return SSV_OK;
}
