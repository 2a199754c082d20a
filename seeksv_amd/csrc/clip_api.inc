// clip_api.inc - C ABI of getclip: the clip scan, the clustering of its events and the cluster table (included by seeksv_hip.hip;
// kernels in clip_kernels.h, table3_kernels.h, tile_sort.h, radix_sort.h; the host rebuild of the table's wire rows in table_wire.h)

// the dense cluster table: device columns + pinned host copy, double buffered so that the PCIe copy of one table can overlap
// with whatever the caller runs next (ssv_clip_cluster_async / ssv_clip_table_wait)
// plain host memory that only grows (the columns the helper thread rebuilds: nothing copies into them by address)
struct PlainBuf {
	void *p = nullptr; size_t cap = 0;
	PlainBuf() = default;
	PlainBuf(const PlainBuf &) = delete;
	PlainBuf &operator=(const PlainBuf &) = delete;
	~PlainBuf() { free(p); }
	bool ensure(size_t bytes)
	{
		if (bytes <= cap) return true;
		const size_t ncap = std::max(bytes, cap + cap / 2);
		free(p); p = malloc(ncap); cap = p ? ncap : 0;
		return p != nullptr;
	}
};

// the context's helper thread: one table set after the other, in the order ssv_clip_cluster_async queued them
struct TableHelper {
	std::thread th;
	std::mutex mu;
	std::condition_variable cv_go, cv_done;
	std::deque<int> jobs;
	bool quit = false;
};

struct TableSet {
	DBuf o_tid, o_pos, o_side, o_support, o_ll, o_lr, o_qmiss, o_ncig, o_stroff, o_cigoff, o_str, o_cig;
	HBuf h_tid, h_pos, h_side, h_support, h_ll, h_lr, h_qmiss, h_stroff, h_cigoff, h_ncig, h_str, h_cig;
	// format 3 (compact): pos, flags (in o_qmiss / h_qmiss), str, cig as above, plus
	DBuf o_len, o_sup, o_nc, o_runs, o_exc;
	HBuf h_len, h_sup, h_nc, h_runs, h_exc;
	int format = 0, base_bits = 4, len_bytes = 4, support_bytes = 4, ncig_bytes = 4;
	int64_t n_runs = 0, n_exc = 0;
	uint64_t str_bytes = 0, cig_ops = 0;
	int64_t support_sum = 0;
	// the columns ssv_clip_table_expand rebuilds on the host
	std::vector<int32_t> x_tid, x_support, x_ll, x_lr, x_ncig;
	std::vector<uint8_t> x_side, x_qmiss;
	std::vector<uint64_t> x_stroff, x_cigoff;
	bool expanded = false, ordered = false;
	hipEvent_t copied = nullptr;
	hsa_signal_t copied_sig{};                      // ... or, when the copy went to a named SDMA engine (LinkCopy), its HSA signal: zero when every piece has landed
	bool via_link = false;
	hsa_signal_t big_sig{}; size_t big_bytes = 0;     // the largest piece (the string block) on a signal of its own: it is the one that is timed
	hipEvent_t packed_ev = nullptr;                 // the set's pack kernels are done (its copy waits for it): one event per set - a copy that is
	                                                // still queued behind the table before must not see the next pass's record of a shared event
	bool in_flight = false;
	// format 3, the narrow wire form (table_wire.h; wire == 1): rows and position escapes cross instead of pos / len / support / ncig, and the CIGAR stream holds the kind-0
	// clusters' operations only; the helper thread rebuilds the handed-out columns into r_* while the strings are still crossing.  v_*: what is handed out, either way
	int wire = 0;
	DBuf o_row, o_pesc;
	HBuf h_row, h_pesc;
	int64_t pesc_tiles = 0, pesc_extra = 0, n_pesc = 0;
	uint64_t wire_ops = 0;                          // operations in the CIGAR stream that crossed (cig_ops: those of the handed-out c_cigar)
	uint64_t wire_piece[7] = {0};                   // bytes that crossed: rows (or the wide columns), flags, CIGAR stream, runs, base exceptions, position escapes, strings
	PlainBuf r_pos, r_len, r_sup, r_nc, r_cig;
	const void *v_pos = nullptr, *v_len = nullptr, *v_sup = nullptr, *v_nc = nullptr, *v_cig = nullptr;
	hipEvent_t small_ev = nullptr;                  // the small pieces have landed (the hipMemcpyAsync path; the link path has copied_sig)
	bool job_pending = false;                       // the helper thread still works on this set (guarded by TableHelper::mu)
	int job_rc = 0, job_expand_nt = -1;             // its result; >= 0: it also builds the expanded columns, on that many threads (0: as many as the machine has)
	std::string job_err;
	int64_t n_clusters = 0, n_events = 0;
	int packed = 0, qual_bits = 8, qual_group = 1, qual_radix = 0, cig_bytes = 4; // qual_group > 1 (format 3): qual_bits per group of that many qualities, radix = the alphabet's size
	uint8_t qual_alphabet[64] = {0};
};

struct ssv_clip_state {
	bool active = false;
	ssv_clip_params p{};
	DBuf d_last_tid, cand, cand_cnt, cand_off, kv_stage;
	DBuf ev, ev_meta, ev_idx, key_l, val_l, key_r[2], val_r[2];  // the pass's event lines (slots, with holes), per event in BAM order (l_qseq, n_cigar) and slot, and the sort keys / slots of the two sides
	int64_t ev_slots = 0;                                        // slots handed out so far
	int64_t ev_cap = 0, n_events = 0, n_l = 0, n_r = 0, n_long = 0;
	DBuf g_seq_bytes, g_cig_ops, g_seq_off, g_cig_off; // the copying path (batches without SSV_MEM_PERSISTENT)
	Arena blob;
	uint64_t sum_ncig = 0;
	int max_lq = 0, max_ncig = 0;
	// clustering temporaries / outputs
	DBuf keys2[2], vals2[2], evs, cum_l, cum_r, c_support, c_ll, c_lr, c_cig_ev, c_qmiss, c_mflag, c_mslot, c_mlist, c_bflag, c_boff, c_blist, c_dlist, bins4_tab, c_strings, slot_cnt, slot_bytes, tile_sums;
	DBuf o_slowlist, o_desc;
	TableSet tab[2];
	HostPool pool;             // ssv_clip_table_expand's threads, and the helper's rebuild
	std::mutex pool_mu;        // ... one user at a time: the caller's own expand may meet the helper at work on the other table set
	TableHelper helper;
	int expand_nt = -1;        // >= 0: a caller has expanded a table of this context with that n_threads - later tables get their expanded columns from the helper
	int tab_cur = 0;           // set of the most recent ssv_clip_cluster[_async]
	int table_mode = 0;        // ssv_clip_table_format: 0 ASCII, 3 compact
	DBuf qual_lut, qual_seen, pair_lut; HBuf h_qual_lut, h_pair_lut;
};

static void table_link_wait(ssv_ctx *c, TableSet &T)
{
	link_wait(c, T.copied_sig);
	link_wait(c, T.big_sig);
	if (T.big_bytes) { link_timed(c, T.big_sig, T.big_bytes, true); T.big_bytes = 0; }
}

static int ensure_events(ssv_ctx *c, int64_t need)
{
	ssv_clip_state &C = *c->clip;
	if (need <= C.ev_cap) return SSV_OK;
	int64_t ncap = std::max<int64_t>(need, C.ev_cap + C.ev_cap / 2);
	ncap = std::max<int64_t>(ncap, 1 << 16);
	CHECK(ensure(c, C.ev_meta, (size_t)ncap * 8, true, (size_t)C.n_events * 8));
	CHECK(ensure(c, C.ev_idx, (size_t)ncap * 4, true, (size_t)C.n_events * 4));
	CHECK(ensure(c, C.key_l, (size_t)ncap * 8, true, (size_t)C.n_l * 8));
	CHECK(ensure(c, C.val_l, (size_t)ncap * 4, true, (size_t)C.n_l * 4));
	CHECK(ensure(c, C.key_r[0], (size_t)ncap * 8, true, (size_t)C.n_r * 8));
	CHECK(ensure(c, C.val_r[0], (size_t)ncap * 4, true, (size_t)C.n_r * 4));
	C.ev_cap = ncap;
	return SSV_OK;
}

int ssv_clip_begin(ssv_ctx *c, const ssv_clip_params *p)
{
	if (!c || !p) return SSV_E_ARG;
	ssv_clip_state &C = *c->clip;
	// (the announced batches stay announced: a pass may end and the next begin in the middle of a stream of batches - and of a batch,
	// ssv_clip_scan_range; a caller that abandons a stream says so with ssv_batch_prefetch_drop)
	HIPCHECK(c, hipSetDevice(c->device));
	C.p = *p;
	C.active = true;
	C.n_events = 0; C.n_l = 0; C.n_r = 0; C.n_long = 0; C.sum_ncig = 0; C.max_lq = 0; C.max_ncig = 0; C.ev_slots = 0;
	C.blob.cur = 0; C.blob.used = 0;
	CHECK(ensure(c, C.d_last_tid, 16));
	CHECK(ensure(c, c->counters, sizeof(ClipCounters)));
	CHECK(ensure_host(c, c->h_counters, sizeof(ClipCounters)));
	HIPCHECK(c, hipMemsetAsync(C.d_last_tid.p, 0, 16, c->st));
	int *h_lt = P<int>(c->h_counters);
	*h_lt = p->initial_last_tid; // 0 in the reference, clip_reads.h:407
	HIPCHECK(c, hipMemcpyAsync(C.d_last_tid.p, h_lt, 4, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	return SSV_OK;
}

int ssv_clip_scan(ssv_ctx *c, const ssv_batch_t *b) { return b ? ssv_clip_scan_range(c, b, 0, b->n) : SSV_E_ARG; }

int ssv_clip_scan_range(ssv_ctx *c, const ssv_batch_t *b, int64_t rec_begin, int64_t rec_end)
{
	if (!c || !b) return SSV_E_ARG;
	ssv_clip_state &C = *c->clip;
	if (!C.active) { c->err = "ssv_clip_scan before ssv_clip_begin"; return SSV_E_STATE; }
	if (rec_begin < 0 || rec_begin > rec_end || rec_end > b->n) { c->err = "ssv_clip_scan_range: bad record range"; return SSV_E_ARG; }
	HIPCHECK(c, hipSetDevice(c->device));
	if (b->n == 0) return SSV_OK;
	DevBatch d;
	CHECK(stage_batch(c, b, d, rec_end < b->n));
	if (!d.cigar) { c->err = "batch without cigar"; return SSV_E_ARG; }
	d.n = rec_end; // what lies behind the range is not looked at (nor does it move the contig-switch state)
	if (rec_end == 0) return SSV_OK;
	CHECK(staged_ends(c, d)); // (the batcher did not fill the cigar_ends column: built from the lines)
	const bool persistent = b->mem == (SSV_MEM_DEVICE | SSV_MEM_PERSISTENT);
	const int64_t ntiles = (d.n + CC_TILE - 1) / CC_TILE;
	const unsigned grid = scan_blocks(ntiles, "SSV_CLIP_SCAN_BLOCKS", 256 * 6);
	CHECK(ensure(c, c->tile_cnt, ntiles * 4));
	CHECK(ensure(c, c->tile_off, ntiles * 4));
	CHECK(ensure(c, c->tile_base, ntiles * 4));
	CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(std::max<int64_t>(ntiles, 1)) * 4));
	if (c->stage_cap == 0) c->stage_cap = std::max<int64_t>(1 << 16, d.n / 8);
	ClipCounters *hc = P<ClipCounters>(c->h_counters);
	ClipCounters *dc = P<ClipCounters>(c->counters);
	for (int attempt = 0;; ++attempt) {
		const int64_t block_cap = (c->stage_cap + grid - 1) / grid;
		CHECK(ensure(c, c->stage, (size_t)block_cap * grid * 4));
		HIPCHECK(c, hipMemsetAsync(c->counters.p, 0, sizeof(ClipCounters), c->st));
		ClipScanArgs a;
		a.ends = d.ends; a.n = d.n;
		a.tile_cnt = P<uint32_t>(c->tile_cnt); a.tile_off = P<uint32_t>(c->tile_off); a.stage = P<uint32_t>(c->stage); a.block_cap = block_cap;
		a.overflow = &dc->overflow; a.ntiles = ntiles;
		{
			ProfScope ps(c, P_CLIP_SCAN, d.n);
			k_clip_scan_ends<<<grid, BLOCK, 0, c->st>>>(a);
		}
		HIPCHECK(c, hipGetLastError());
		// order across tiles: exclusive scan of the tile counts; its total is the number of candidates
		exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(c->tile_cnt), P<uint32_t>(c->tile_base), ntiles, 0u, P<uint32_t>(c->scan_scratch), reinterpret_cast<uint32_t *>(&dc->n_cand));
		HIPCHECK(c, hipMemcpyAsync(hc, c->counters.p, sizeof(ClipCounters), hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
		if (!hc->overflow) break;
		if (attempt > 4) { c->err = "clip staging overflow"; return SSV_E_HIP; }
		c->stage_cap = std::max<int64_t>(c->stage_cap * 4, (int64_t)(uint32_t)hc->n_cand * 4); // a workgroup's private region was too small
	}
	const int64_t ncand = (int64_t)(uint32_t)hc->n_cand;
	if (ncand > 0) {
		int64_t nb = 0, slot_base = 0;
		(void)slot_base;
		{
			ProfScope ps(c, P_CLIP_PLACE, ncand);
			const int64_t nwave = (ncand + 15) / 16; // k_clip_filter: four lanes per candidate, 16 candidates per wavefront
			CHECK(ensure(c, C.cand, ncand * 4)); CHECK(ensure(c, C.cand_cnt, ncand + 64)); CHECK(ensure(c, C.cand_off, nwave * 8));
			const int64_t nslot = 2 * (((ncand + 63) / 64) * 64); // two per candidate, whole workgroups (64 candidates each)
			if (C.ev_slots + nslot >= (1ll << 32) - 1) { c->err = "more than 2^32 event slots in one pass (the sorted permutation is 32 bits wide)"; return SSV_E_RANGE; }
			CHECK(ensure(c, C.ev, (size_t)(C.ev_slots + nslot) * sizeof(ClipEvent), true, (size_t)C.ev_slots * sizeof(ClipEvent)));
			CHECK(ensure(c, C.kv_stage, (size_t)nslot * 16));
			CHECK(ensure(c, c->scan_scratch64, scan_scratch_elems(nwave) * 8));
			CHECK(ensure_events(c, C.n_events + 2 * ncand));
			k_cand_place<<<grid_for(ntiles, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(P<uint32_t>(c->stage), P<uint32_t>(c->tile_cnt), P<uint32_t>(c->tile_off), P<uint32_t>(c->tile_base), ntiles,
			                                                                    P<uint32_t>(C.cand));
			ClipFilterArgs f;
			f.b = d; f.min_mapq = C.p.min_mapq; f.save_low_quality = C.p.save_low_quality; f.last_tid_in = P<int>(C.d_last_tid);
			f.use_ownership = C.p.use_ownership; f.rec_begin = rec_begin;
			f.own_lo = ((long long)C.p.own_lo_tid << 32) | (long long)(uint32_t)C.p.own_lo_pos;
			f.own_hi = ((long long)C.p.own_hi_tid << 32) | (long long)(uint32_t)C.p.own_hi_pos;
			k_clip_filter<<<grid_for(ncand, BLOCK / 4), BLOCK, 0, c->st>>>(f, P<uint32_t>(C.cand), ncand, P<ClipEvent>(C.ev) + C.ev_slots, P<uint4>(C.kv_stage), P<uint8_t>(C.cand_cnt), P<uint64_t>(C.cand_off));
			exclusive_scan<uint64_t, uint64_t>(c->st, P<uint64_t>(C.cand_off), P<uint64_t>(C.cand_off), nwave, 0ull, P<uint64_t>(c->scan_scratch64), reinterpret_cast<uint64_t *>(&dc->n_new));
			EventLists L;
			L.key_l = P<uint64_t>(C.key_l); L.val_l = P<uint32_t>(C.val_l); L.key_r = P<uint64_t>(C.key_r[0]); L.val_r = P<uint32_t>(C.val_r[0]);
			L.meta = P<uint2>(C.ev_meta); L.idx = P<uint32_t>(C.ev_idx);
			k_clip_place<<<grid_for(ncand, BLOCK), BLOCK, 0, c->st>>>(P<uint4>(C.kv_stage), P<uint8_t>(C.cand_cnt), P<uint64_t>(C.cand_off), ncand, L, C.n_events, C.n_l, C.n_r, C.ev_slots);
			k_event_max<<<512, BLOCK, 0, c->st>>>(P<uint2>(C.ev_meta), C.n_events, dc);
			HIPCHECK(c, hipGetLastError());
			HIPCHECK(c, hipMemcpyAsync(hc, c->counters.p, sizeof(ClipCounters), hipMemcpyDeviceToHost, c->st));
			HIPCHECK(c, hipStreamSynchronize(c->st));
			nb = (int64_t)(uint32_t)hc->n_new;
			slot_base = C.ev_slots;
			C.ev_slots += nslot;
		}
		if (nb > 0 && !persistent) {
			// the batch's buffers may be recycled after this call: the bytes its events point at move into context memory
			ProfScope ps(c, P_CLIP_GATHER, nb);
			CHECK(ensure(c, C.g_seq_bytes, nb * 4)); CHECK(ensure(c, C.g_cig_ops, nb * 4)); CHECK(ensure(c, C.g_seq_off, nb * 8)); CHECK(ensure(c, C.g_cig_off, nb * 8));
			CHECK(ensure(c, c->scan_scratch64, scan_scratch_elems(nb) * 8));
			k_gather_sizes<<<grid_for(nb, BLOCK), BLOCK, 0, c->st>>>(P<uint2>(C.ev_meta), C.n_events, nb, P<uint32_t>(C.g_seq_bytes), P<uint32_t>(C.g_cig_ops));
			exclusive_scan<uint32_t, uint64_t>(c->st, P<uint32_t>(C.g_seq_bytes), P<uint64_t>(C.g_seq_off), nb, 0ull, P<uint64_t>(c->scan_scratch64), reinterpret_cast<uint64_t *>(&dc->seq_total));
			exclusive_scan<uint32_t, uint64_t>(c->st, P<uint32_t>(C.g_cig_ops), P<uint64_t>(C.g_cig_off), nb, 0ull, P<uint64_t>(c->scan_scratch64), reinterpret_cast<uint64_t *>(&dc->cig_total));
			HIPCHECK(c, hipMemcpyAsync(hc, c->counters.p, sizeof(ClipCounters), hipMemcpyDeviceToHost, c->st));
			HIPCHECK(c, hipStreamSynchronize(c->st));
			void *seq_dst = nullptr, *cig_dst = nullptr;
			CHECK(arena_alloc(c, C.blob, (size_t)hc->seq_total + 16, &seq_dst));
			CHECK(arena_alloc(c, C.blob, (size_t)hc->cig_total * 4 + 16, &cig_dst));
			k_clip_gather<<<grid_for(nb, GROUPS_PER_BLOCK), BLOCK, 0, c->st>>>(P<ClipEvent>(C.ev), P<uint32_t>(C.ev_idx), C.n_events, nb, P<uint64_t>(C.g_seq_off), P<uint64_t>(C.g_cig_off),
			                                                                          reinterpret_cast<uint8_t *>(seq_dst), reinterpret_cast<uint32_t *>(cig_dst));
			HIPCHECK(c, hipGetLastError());
		}
		if (nb > 0) {
			const int64_t nbr = (int64_t)(hc->n_new >> 32);
			C.n_events += nb; C.n_r += nbr; C.n_l += nb - nbr; C.n_long += (int64_t)hc->n_long;
			C.max_lq = std::max(C.max_lq, hc->max_lq);
			C.max_ncig = std::max(C.max_ncig, hc->max_ncig);
			C.sum_ncig += hc->sum_ncig;
		}
	}
	k_last_tid<<<1, BLOCK, 0, c->st>>>(d, P<int>(C.d_last_tid));
	HIPCHECK(c, hipGetLastError());
	return SSV_OK;
}

int ssv_clip_event_count(ssv_ctx *c, int64_t *n)
{
	if (!c || !n) return SSV_E_ARG;
	ssv_clip_state &C = *c->clip;
	HIPCHECK(c, hipStreamSynchronize(c->st));
	*n = C.n_events;
	return SSV_OK;
}

// entries of the list of bases outside A/C/G/T that a compact table may carry before it falls back to 4-bit bases
static int64_t exc_cap_of(int64_t E)
{
	const char *e = getenv("SSV_EXC_CAP"); // (tests: a tiny list)
	return e ? (int64_t)atoll(e) : std::min<int64_t>(E / 2 + 65536, 0xffffffffll);
}

// the narrow wire form's position escapes: one place per tile of 256 slots, and a list for the others (runs' first clusters, gaps of 65535 bases or more) - a table
// with more of those than this crosses with the wide columns
static int64_t pesc_cap_of(int64_t E) { return E / 8 + 65536; }
static size_t pesc_bytes_of(int64_t E) { return ((size_t)grid_for(E, BLOCK) + (size_t)pesc_cap_of(E)) * 8 + 16; }

// ---- ssv_clip_cluster_async: the events of the pass -> a cluster table on its way to the host, in six phases ----

// 1. the table set's format fields for a pass of E events
static void table_begin(const ssv_clip_state &C, TableSet &T, int64_t E)
{
	const bool fmt3 = C.table_mode == 3;
	T.n_events = E; T.n_clusters = 0;
	T.packed = C.table_mode ? 1 : 0; T.qual_bits = 8; T.qual_group = 1; T.qual_radix = 0; memset(T.qual_alphabet, 0, sizeof(T.qual_alphabet));
	T.format = C.table_mode; T.base_bits = fmt3 ? 2 : 4; T.n_runs = 0; T.n_exc = 0; T.expanded = false; T.ordered = false;
	T.cig_bytes = fmt3 ? 2 : 4; T.len_bytes = fmt3 && C.max_lq < 65536 ? 2 : 4; T.support_bytes = fmt3 ? 2 : 4; T.ncig_bytes = fmt3 ? (C.max_ncig < 256 ? 1 : 2) : 4;
	if (fmt3 && getenv("SSV_TABLE_WIDE_COLUMNS")) { T.len_bytes = 4; T.support_bytes = 4; T.ncig_bytes = 2; } // (tests: the widths that only reads > 64 kb, > 65535-read clusters, > 255-operation CIGARs ask for)
	// what crosses: the narrow rows (table_wire.h) unless the pass asks for the columns themselves - SSV_TABLE_WIRE=wide, the wide columns above, the split scans
	// (SSV_PACK_COLS=split), reads so long that a row would hardly hold their lengths - or cluster_pack meets a value a row cannot hold
	static const bool split_cols = [] { const char *e = getenv("SSV_PACK_COLS"); return e && !strcmp(e, "split"); }();
	const char *we = getenv("SSV_TABLE_WIRE");
	T.wire = fmt3 && !split_cols && !getenv("SSV_TABLE_WIDE_COLUMNS") && !(we && !strcmp(we, "wide")) && C.max_lq <= (int)WIRE_LEN_MAX * 2 ? 1 : 0;
	T.wire_ops = 0; T.pesc_tiles = 0; T.pesc_extra = 0; T.n_pesc = 0; memset(T.wire_piece, 0, sizeof(T.wire_piece));
	T.v_pos = T.v_len = T.v_sup = T.v_nc = T.v_cig = nullptr;
	T.job_rc = 0; T.job_err.clear(); T.job_expand_nt = -1;
}

// 2. bin the events by (contig, side, position), BAM order inside a bin.  A coordinate-sorted BAM emits its '5' events in key order
//    already (key = start + 1): that is checked, not assumed; only the '3' events (key = start + reference span) need the sort, and
//    the two sorted lists interleave per contig.  Unsorted input takes the full sort.  *cur: which keys2[] holds the sorted keys
static int cluster_sort(ssv_ctx *c, bool fmt3, int *cur)
{
	ssv_clip_state &C = *c->clip;
	const int64_t E = C.n_events, EL = C.n_l, ER = C.n_r;
	ClipCounters *hc = P<ClipCounters>(c->h_counters);
	ClipCounters *dc = P<ClipCounters>(c->counters);
	const ClipEvent *ev = P<ClipEvent>(C.ev);
	ProfScope ps(c, P_SORT, E);
	HIPCHECK(c, hipMemsetAsync(c->counters.p, 0, sizeof(ClipCounters), c->st));
	if (EL > 1) k_check_sorted<<<grid_for(EL, BLOCK), BLOCK, 0, c->st>>>(P<uint64_t>(C.key_l), EL, &dc->l_unsorted);
	if (EL > 0) k_key_max<<<(unsigned)std::min<int64_t>(512, grid_for(EL, BLOCK)), BLOCK, 0, c->st>>>(P<uint64_t>(C.key_l), EL, &dc->max_key);
	if (ER > 0) k_key_max<<<(unsigned)std::min<int64_t>(512, grid_for(ER, BLOCK)), BLOCK, 0, c->st>>>(P<uint64_t>(C.key_r[0]), ER, &dc->max_key);
	// the '3' list is sorted up to small displacements: one windowed rank pass, checked (tile_sort.h); where the check fails (r_unsorted) the radix sort below takes over - the attempt is always made, there is no switch for it
	if (ER > 0) { CHECK(ensure(c, C.key_r[1], ER * 8)); CHECK(ensure(c, C.val_r[1], ER * 4)); }
	if (ER > 0) HIPCHECK(c, sort_nearly_sorted(c->st, P<uint64_t>(C.key_r[0]), P<uint32_t>(C.val_r[0]), P<uint64_t>(C.key_r[1]), P<uint32_t>(C.val_r[1]), ER, &dc->r_unsorted));
	if (fmt3) {
		// first guess of the table's quality alphabet: the qualities of the first events
		uint32_t *h_seen = reinterpret_cast<uint32_t *>(P<uint8_t>(c->h_totals) + 64);
		HIPCHECK(c, hipMemsetAsync(C.qual_seen.p, 0, 32, c->st));
		const int64_t ns = std::min<int64_t>(E, 4096); // (a value missed here is caught while packing, at the price of packing twice)
		k_qual_sample<<<grid_for(ns, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(ev, P<uint32_t>(C.ev_idx), ns, P<uint32_t>(C.qual_seen));
		HIPCHECK(c, hipMemcpyAsync(h_seen, C.qual_seen.p, 32, hipMemcpyDeviceToHost, c->st));
	}
	HIPCHECK(c, hipMemcpyAsync(hc, c->counters.p, sizeof(ClipCounters), hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const uint64_t max_key = hc->max_key;
	int key_bits = 1;
	while (key_bits < 64 && (max_key >> key_bits)) ++key_bits;
	CHECK(ensure(c, C.keys2[0], E * 8)); CHECK(ensure(c, C.evs, (size_t)E * sizeof(ClipEvent)));
	if (!hc->l_unsorted) {
		int rcur = ER > 0 && !hc->r_unsorted ? 1 : 0;
		if (ER > 0 && rcur == 0) {
			const int64_t nt = rs_tiles(ER);
			CHECK(ensure(c, c->ghist, 256 * nt * 4));
			CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(256 * nt) * 4));
			uint64_t *keys[2] = {P<uint64_t>(C.key_r[0]), P<uint64_t>(C.key_r[1])};
			uint32_t *vals[2] = {P<uint32_t>(C.val_r[0]), P<uint32_t>(C.val_r[1])};
			rcur = radix_sort_pairs(c->st, keys, vals, ER, key_bits, P<uint32_t>(c->ghist), P<uint32_t>(c->scan_scratch));
		}
		const int64_t Tn = (int64_t)(max_key >> 33) + 1;
		CHECK(ensure(c, C.cum_l, (size_t)(Tn + 2) * 4)); CHECK(ensure(c, C.cum_r, (size_t)(Tn + 2) * 4));
		k_side_bounds<<<grid_for(Tn + 1, BLOCK), BLOCK, 0, c->st>>>(P<uint64_t>(C.key_l), EL, P<uint64_t>(C.key_r[rcur]), ER, Tn, P<uint32_t>(C.cum_l), P<uint32_t>(C.cum_r));
		k_merge_sides<<<grid_for(E, BLOCK / 4), BLOCK, 0, c->st>>>(P<uint64_t>(C.key_l), P<uint32_t>(C.val_l), EL, P<uint64_t>(C.key_r[rcur]), P<uint32_t>(C.val_r[rcur]), ER,
		                                                       P<uint32_t>(C.cum_l), P<uint32_t>(C.cum_r), ev, P<uint64_t>(C.keys2[0]), P<ClipEvent>(C.evs));
		*cur = 0;
	} else {
		CHECK(ensure(c, C.keys2[1], E * 8)); CHECK(ensure(c, C.vals2[0], E * 4)); CHECK(ensure(c, C.vals2[1], E * 4));
		const int64_t nt = rs_tiles(E);
		CHECK(ensure(c, c->ghist, 256 * nt * 4));
		CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(256 * nt) * 4));
		k_concat_sides<<<grid_for(E, BLOCK), BLOCK, 0, c->st>>>(P<uint64_t>(C.key_l), P<uint32_t>(C.val_l), EL, P<uint64_t>(C.key_r[0]), P<uint32_t>(C.val_r[0]), ER,
		                                                        P<uint64_t>(C.keys2[0]), P<uint32_t>(C.vals2[0]));
		uint64_t *keys[2] = {P<uint64_t>(C.keys2[0]), P<uint64_t>(C.keys2[1])};
		uint32_t *vals[2] = {P<uint32_t>(C.vals2[0]), P<uint32_t>(C.vals2[1])};
		*cur = radix_sort_pairs(c->st, keys, vals, E, key_bits, P<uint32_t>(c->ghist), P<uint32_t>(c->scan_scratch));
		k_gather_lines<<<grid_for(E, BLOCK / 4), BLOCK, 0, c->st>>>(vals[*cur], E, ev, P<ClipEvent>(C.evs));
	}
	HIPCHECK(c, hipGetLastError());
	return SSV_OK;
}

// 3. greedy consensus clustering, one wavefront per multi-event bin: fills `ca` (ca.M: the events in multi-event bins)
static int cluster_bins(ssv_ctx *c, int cur, ClusterArgs &ca)
{
	ssv_clip_state &C = *c->clip;
	const int64_t E = C.n_events;
	ca.skey = P<uint64_t>(C.keys2[cur]); ca.E = E; ca.ev = P<ClipEvent>(C.evs);
	ca.match_rate = C.p.match_rate;
	ca.SL = ca.SR = (std::max(1, C.max_lq) + 3) & ~3; // |seq_left|, |seq_right| <= l_qseq, also after consensus growth; a multiple of four: k_cluster_bins4 moves dwords
	const size_t stride = 2 * ((size_t)ca.SL + (size_t)ca.SR);
	ProfScope ps(c, P_CLUSTER_BINS, E);
	CHECK(ensure(c, C.c_support, E * 4)); CHECK(ensure(c, C.c_ll, E * 4)); CHECK(ensure(c, C.c_lr, E * 4)); CHECK(ensure(c, C.c_cig_ev, E * 4));
	CHECK(ensure(c, C.c_qmiss, E)); CHECK(ensure(c, C.c_mflag, E * 4)); CHECK(ensure(c, C.c_mslot, E * 4));
	CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(E) * 4));
	ca.support = P<int32_t>(C.c_support); ca.c_ll = P<int32_t>(C.c_ll); ca.c_lr = P<int32_t>(C.c_lr); ca.c_cig_ev = P<uint32_t>(C.c_cig_ev);
	ca.c_qmiss = P<uint8_t>(C.c_qmiss); ca.mflag = P<uint32_t>(C.c_mflag); ca.mslot = P<uint32_t>(C.c_mslot);
	k_bin_mark<<<grid_for(E, BLOCK), BLOCK, 0, c->st>>>(ca.skey, E, P<uint32_t>(C.c_mflag), ca.support);
	exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(C.c_mflag), P<uint32_t>(C.c_mslot), E, 0u, P<uint32_t>(c->scan_scratch), P<uint32_t>(c->totals));
	HIPCHECK(c, hipMemcpyAsync(c->h_totals.p, c->totals.p, 4, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const int64_t M = *P<uint32_t>(c->h_totals); // events in multi-event bins: only they need consensus storage
	CHECK(ensure(c, C.c_strings, (size_t)std::max<int64_t>(M, 1) * stride));
	ca.strings = P<uint8_t>(C.c_strings);
	ca.M = M; ca.mlist = nullptr; ca.blist = nullptr; ca.n_bins = nullptr; ca.dlist = nullptr; ca.tab4 = nullptr; ca.deep_cap = 0;
	if (M > 0) {
		// one wavefront per slot of a multi-event bin (3 % of the slots; the waves that do not sit on a bin start leave at once)
		CHECK(ensure(c, C.c_mlist, M * 4));
		ca.mlist = P<uint32_t>(C.c_mlist);
		k_multi_list<<<grid_for(E, BLOCK), BLOCK, 0, c->st>>>(ca.mflag, ca.mslot, E, P<uint32_t>(C.c_mlist));
		// the bins' first slots, densely: every wavefront of the clustering kernel then has a bin (a bin has at least two slots)
		// (two counters in one 64-bit scan: the bins, and the deep ones among them - totals[1] = bins | deep bins << 32)
		ca.deep_cap = M / B4_DEEP + 1;
		CHECK(ensure(c, C.c_bflag, M * 8)); CHECK(ensure(c, C.c_boff, M * 8)); CHECK(ensure(c, C.c_blist, (M / 2 + 1) * 4)); CHECK(ensure(c, C.c_dlist, (size_t)ca.deep_cap * 4));
		CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(M) * 8));
		k_bin_start_flags<<<grid_for(M, BLOCK), BLOCK, 0, c->st>>>(ca.skey, E, ca.mlist, M, P<uint64_t>(C.c_bflag));
		exclusive_scan<uint64_t, uint64_t>(c->st, P<uint64_t>(C.c_bflag), P<uint64_t>(C.c_boff), M, 0ull, P<uint64_t>(c->scan_scratch), P<uint64_t>(c->totals) + 1);
		k_bin_start_list<<<grid_for(M, BLOCK), BLOCK, 0, c->st>>>(ca.mlist, P<uint64_t>(C.c_bflag), P<uint64_t>(C.c_boff), M, P<uint32_t>(C.c_blist), P<uint32_t>(C.c_dlist));
		ca.blist = P<uint32_t>(C.c_blist); ca.dlist = P<uint32_t>(C.c_dlist); ca.n_bins = P<uint32_t>(c->totals) + 2;
		// reads of up to 256 bases: four positions per lane, a wavefront = a workgroup, deep bins first; longer ones: a base per lane
		if (C.max_lq <= B4_CAP) {
			CHECK(ensure(c, C.bins4_tab, B4_TAB * 2));
			ca.tab4 = P<uint16_t>(C.bins4_tab);
			k_bins4_tables<<<1, BLOCK, 0, c->st>>>(ca.match_rate, P<uint16_t>(C.bins4_tab));
			k_cluster_bins4<<<(unsigned)(ca.deep_cap + M / 2 + 1), WAVE, 0, c->st>>>(ca);
		} else k_cluster_bins<<<grid_for(M / 2 + 1, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(ca);
	}
	HIPCHECK(c, hipGetLastError());
	return SSV_OK;
}

// the quality values seen (a bit per phred value) -> T.qual_bits / qual_group / qual_radix / qual_alphabet and the phred -> index table `lut` (0xff: not in the alphabet)
static void set_alphabet(TableSet &T, bool fmt3, const uint32_t seen[8], uint8_t *lut)
{
	memset(lut, 0xff, 256); memset(T.qual_alphabet, 0, sizeof(T.qual_alphabet));
	int n_vals = 0;
	for (int v = 0; v < 256; ++v) if ((seen[v >> 5] >> (v & 31)) & 1u) ++n_vals;
	T.qual_group = 1; T.qual_radix = n_vals;
	const char *ge = getenv("SSV_QUAL_GROUPS");
	const bool groups = !ge || atoi(ge) != 0;
	if (n_vals > 45 || (n_vals > 16 && !(fmt3 && groups))) { T.qual_bits = 8; return; } // (bytes: no index table)
	T.qual_bits = n_vals <= 2 ? 1 : n_vals <= 4 ? 2 : n_vals <= 8 ? 3 : 4;
	// format 3: alphabets whose size is far from a power of two go in groups - five values: three qualities as one number below 5^3 in 7 bits (2.33
	// bits a quality instead of 3), nine to eleven values: two in 7 bits (3.5 instead of 4); table3_kernels.h.  SSV_QUAL_GROUPS=0: one quality, one field.
	if (fmt3 && groups && n_vals == 5) { T.qual_bits = 7; T.qual_group = 3; }
	if (fmt3 && groups && n_vals >= 9 && n_vals <= 11) { T.qual_bits = 7; T.qual_group = 2; }
	// 17 to 45 values (a HiSeq-style 40-value alphabet): two to a group of 11 bits (45 x 45 = 2025 <= 2048) - 5.5 bits a quality instead of a byte
	if (fmt3 && groups && n_vals >= 17 && n_vals <= 45) { T.qual_bits = 11; T.qual_group = 2; }
	int k = 0;
	for (int v = 0; v < 256; ++v) if ((seen[v >> 5] >> (v & 31)) & 1u) { T.qual_alphabet[k] = (uint8_t)(v + 33); lut[v] = (uint8_t)k; ++k; } // increasing order; the table shows characters (phred + 33)
}

// three qualities to a group: ONE look-up per group (qual_dword3h) - the alphabet's R^3 triples of phred bytes hashed into 4096 slots by a multiplier under which
// no two of them meet (a few tries: 125 keys, 4096 slots); an entry = triple << 8 | the group's number, an empty slot matches no triple.  Returns the multiplier (0: none found)
static uint32_t build_triple_lut(const TableSet &T, uint32_t *tl)
{
	const int R = T.qual_radix;
	for (uint32_t m = 0x9e3779u; m < 0x9e3779u + 4096u * 2u; m += 2u) {
		for (int i = 0; i < (1 << TRI_BITS); ++i) tl[i] = 0xffffffffu;
		bool ok = true;
		for (int i2 = 0; i2 < R && ok; ++i2)
			for (int i1 = 0; i1 < R && ok; ++i1)
				for (int i0 = 0; i0 < R && ok; ++i0) {
					const uint32_t tri = (uint32_t)(T.qual_alphabet[i0] - 33) | ((uint32_t)(T.qual_alphabet[i1] - 33) << 8) | ((uint32_t)(T.qual_alphabet[i2] - 33) << 16);
					const uint32_t slot = (uint32_t)((uint64_t)tri * (m & 0xffffffu)) >> (32 - TRI_BITS); // (v_mul_u32_u24: the low 32 bits of the 24 x 24 bit product)
					if (tl[slot] != 0xffffffffu) ok = false;
					else tl[slot] = (tri << 8) | (uint32_t)(i0 + R * i1 + R * R * i2);
				}
		if (ok && (m & 0xffffffu)) return m & 0xffffffu;
	}
	return 0;
}

// two qualities (below phred 64) per look-up: 4096 entries over the index table `lut`, 0x8000 = a value outside the alphabet
static void build_pair_lut(const TableSet &T, const uint8_t *lut, uint16_t *pl)
{
	for (int q1 = 0; q1 < 64; ++q1)
		for (int q0 = 0; q0 < 64; ++q0) {
			const bool out = lut[q0] == 0xff || lut[q1] == 0xff;
			if (T.qual_group == 2) pl[q0 | (q1 << 6)] = out ? (uint16_t)0x8000 : (uint16_t)(lut[q0] + T.qual_radix * lut[q1]); // qual_dword3g: a pair IS a group
			else if (T.qual_group > 1) pl[q0 | (q1 << 6)] = out ? (uint16_t)0x8000 : (uint16_t)(lut[q0] | (lut[q1] << 4) | ((lut[q0] + T.qual_radix * lut[q1]) << 8));
			else pl[q0 | (q1 << 6)] = out ? (uint16_t)0x8000 : (uint16_t)(lut[q0] | (lut[q1] << T.qual_bits));
		}
}

// format 3's string kernels for the table's shape (quality width / grouping, base width, alphabet tracking, with or without the LDS stage)
static void pack3_launch(ssv_ctx *c, const TableSet &T, const PackArgs &pa, const Pack3Args &p3, PackDesc *dsc, const unsigned int *nc_dev, uint8_t *os, bool direct, bool track)
{
	ssv_clip_state &C = *c->clip;
	const int64_t E = pa.c.E, M = pa.c.M;
	// one group of lanes per cluster (the grid is an upper bound, the kernel reads the cluster count itself), then the base-by-base path
	const dim3 g(grid_for(E, GROUPS_PER_BLOCK));
	const dim3 gs3(grid_for(std::max<int64_t>(M + C.n_long, 1), BLOCK)); // k_pack3_slow: an item per lane (a wavefront then works off the ones with a cluster)
	const unsigned p3_blocks = 256u * 40u; // persistent (80 registers: six workgroups per CU resident); 2560 / 5120 / 10240 / 20480 workgroups measured in round 4: 1.20 / 1.18 / 1.14 / 1.16 ms for the group
	const dim3 gd((unsigned)std::max<int64_t>(1, std::min<int64_t>(p3_blocks, (E + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK)));
	// lanes per cluster of the direct kernel: as many as the longest read's base / quality stream has dwords, rounded up to the next whole share of a wavefront
	// (150 bases, grouped qualities: 11 -> 12 lanes, five clusters a wavefront); streams of more than 32 dwords take 16 lanes and several rounds
	int lpc = 16;
	{
		const int n_fast = std::max(1, std::min(C.max_lq, PACK_MAX_LQ));
		const int nd = std::max((n_fast * T.base_bits + 31) / 32, (int)((qual_stream_bits((uint64_t)n_fast, (uint64_t)T.qual_bits, (uint64_t)T.qual_group) + 31) / 32));
		if (nd <= 32) lpc = WAVE / (WAVE / nd);
	}
#define SSV_P3D(W_, B_, K_) k_pack3_direct<W_, B_, K_><<<gd, BLOCK, 0, c->st>>>(pa, p3, dsc, nc_dev, os, P<uint16_t>(C.pair_lut), lpc)
#define SSV_P3B(W_, B_, T_) do { if (direct) SSV_P3D(W_, B_, 1); else k_pack3_stream<W_, B_, T_><<<g, BLOCK, 0, c->st>>>(pa, p3, dsc, nc_dev, os); \
		k_pack3_slow<W_, B_, T_><<<gs3, BLOCK, 0, c->st>>>(pa, p3, os); } while (0)
	// grouped qualities: the direct kernel knows the two shapes, the staged and the bytewise kernels take the shape at run time (W = 0)
#define SSV_P3G(B_, T_) do { if (direct) { if (pa.qual_group == 3) SSV_P3D(7, B_, 3); else if (pa.qual_bits == 11) SSV_P3D(11, B_, 2); else SSV_P3D(7, B_, 2); } \
		else k_pack3_stream<0, B_, T_><<<g, BLOCK, 0, c->st>>>(pa, p3, dsc, nc_dev, os); \
		k_pack3_slow<0, B_, T_><<<gs3, BLOCK, 0, c->st>>>(pa, p3, os); } while (0)
#define SSV_P3GT(T_) do { if (T.base_bits == 2) SSV_P3G(2, T_); else SSV_P3G(4, T_); } while (0)
#define SSV_P3T(W_, T_) do { if (T.base_bits == 2) SSV_P3B(W_, 2, T_); else SSV_P3B(W_, 4, T_); } while (0)
#define SSV_P3(W_) do { if (track) SSV_P3T(W_, true); else SSV_P3T(W_, false); } while (0)
	if (pa.qual_group > 1) { if (track) SSV_P3GT(true); else SSV_P3GT(false); }
	else if (pa.qual_bits == 8) SSV_P3T(8, false); else if (pa.qual_bits == 4) SSV_P3(4); else if (pa.qual_bits == 3) SSV_P3(3); else if (pa.qual_bits == 2) SSV_P3(2); else SSV_P3(1);
#undef SSV_P3
#undef SSV_P3T
#undef SSV_P3B
#undef SSV_P3D
#undef SSV_P3G
#undef SSV_P3GT
}

// 4. the dense table, cut straight out of the reads' bytes.  Nothing here needs a size on the host before the kernels have run:
//    the buffers are sized by upper bounds (E clusters, E x the largest block, the events' CIGAR operations), the kernels read the
//    cluster count from device memory, and the one synchronisation comes after the pack kernels.  Packs again with wider columns or another
//    quality alphabet when the table asks for it; leaves T.n_clusters / str_bytes / cig_ops / n_runs / n_exc
static int cluster_pack(ssv_ctx *c, TableSet &T, const ClusterArgs &ca)
{
	ssv_clip_state &C = *c->clip;
	const int64_t E = ca.E;
	const bool fmt3 = T.format == 3;
	ProfScope ps(c, P_CLUSTER_PACK, E);
	uint32_t *h_seen = reinterpret_cast<uint32_t *>(P<uint8_t>(c->h_totals) + 64);
	uint8_t *lut = P<uint8_t>(C.h_qual_lut);
	uint32_t guess[8] = {0};
	if (fmt3) { memcpy(guess, h_seen, 32); set_alphabet(T, fmt3, guess, lut); }
	CHECK(ensure(c, C.slot_cnt, E * 8)); CHECK(ensure(c, C.slot_bytes, E * 8));
	CHECK(ensure(c, c->scan_scratch64, scan_scratch_elems(E) * 8));
	for (DBuf *b : {&T.o_tid, &T.o_pos, &T.o_support, &T.o_ll, &T.o_lr, &T.o_ncig, &C.o_slowlist}) CHECK(ensure(c, *b, E * 4 + 16));
	CHECK(ensure(c, T.o_side, E + 16)); CHECK(ensure(c, T.o_qmiss, E + 16));
	for (DBuf *b : {&T.o_stroff, &T.o_cigoff}) CHECK(ensure(c, *b, E * 8 + 16));
	CHECK(ensure(c, C.o_desc, (size_t)E * sizeof(PackDesc) + 64));
	CHECK(ensure(c, T.o_cig, (size_t)C.sum_ncig * 4 + 16));
	const int64_t exc_cap = exc_cap_of(E);
	if (fmt3) {
		CHECK(ensure(c, T.o_len, (size_t)E * 8 + 16)); CHECK(ensure(c, T.o_sup, (size_t)E * 4 + 16)); CHECK(ensure(c, T.o_nc, (size_t)E * 2 + 16));
		CHECK(ensure(c, T.o_runs, (size_t)E * sizeof(TableRun) + 16)); CHECK(ensure(c, T.o_exc, (size_t)exc_cap * 8 + 16));
		if (T.wire) { CHECK(ensure(c, T.o_row, (size_t)E * sizeof(WireRow) + 16)); CHECK(ensure(c, T.o_pesc, pesc_bytes_of(E))); }
	}
	// [0] clusters | CIGAR operations << 32, [1] string bytes, [2] slow-list length, [3] "a quality outside the alphabet" flag,
	// format 3: [4] runs | base exceptions << 32, [5] "a support count too wide" | "too many base exceptions" << 32
	uint64_t *tot = P<uint64_t>(c->totals);
	const uint64_t *h_tot = P<uint64_t>(c->h_totals);
	bool track = false;
	for (int attempt = 0;; ++attempt) {
		const size_t str_cap = (size_t)E * (size_t)(fmt3 ? table3_block_bytes((uint64_t)ca.SL + (uint64_t)ca.SR, T.base_bits, T.qual_bits, T.qual_group)
		                                             : table_block_bytes((uint64_t)ca.SL, (uint64_t)ca.SR, T.packed, (uint64_t)T.qual_bits));
		CHECK(ensure(c, T.o_str, str_cap + 16));
		PackArgs pa;
		pa.c = ca; pa.slot_cnt = P<uint64_t>(C.slot_cnt); pa.slot_bytes = P<uint64_t>(C.slot_bytes);
		pa.tid = P<int32_t>(T.o_tid); pa.pos = P<int32_t>(T.o_pos); pa.side = P<uint8_t>(T.o_side); pa.support = P<int32_t>(T.o_support); pa.ll = P<int32_t>(T.o_ll);
		pa.lr = P<int32_t>(T.o_lr); pa.qmiss = P<uint8_t>(T.o_qmiss); pa.ncig = P<int32_t>(T.o_ncig); pa.str_off = P<uint64_t>(T.o_stroff); pa.cig_off = P<uint64_t>(T.o_cigoff);
		pa.packed = T.packed; pa.qual_bits = T.qual_bits; pa.qual_group = T.qual_group; pa.qual_radix = T.qual_radix;
		pa.qual_fill = T.qual_bits != 8 && T.qual_alphabet[0] ? (uint32_t)(T.qual_alphabet[0] - 33) * 0x01010101u : 0u; pa.qlut = P<uint8_t>(C.qual_lut); pa.qual_seen = P<uint32_t>(C.qual_seen);
		pa.lut_miss = reinterpret_cast<int *>(tot + 3);
		pa.slow_list = P<uint32_t>(C.o_slowlist); pa.slow_count = reinterpret_cast<unsigned int *>(tot + 2);
		pa.format3 = fmt3 ? 1 : 0; pa.base_bits = T.base_bits;
		Pack3Args p3{};
		if (fmt3) {
			p3.pos = P<int32_t>(T.o_pos); p3.len = T.o_len.p; p3.support = T.o_sup.p; p3.ncig = T.o_nc.p; p3.flags = P<uint8_t>(T.o_qmiss);
			p3.len_bytes = T.len_bytes; p3.support_bytes = T.support_bytes; p3.ncig_bytes = T.ncig_bytes; p3.base_bits = T.base_bits;
			p3.runs = P<TableRun>(T.o_runs); p3.run_count = reinterpret_cast<unsigned int *>(tot + 4);
			p3.exc = P<uint64_t>(T.o_exc); p3.exc_count = reinterpret_cast<unsigned int *>(tot + 4) + 1; p3.exc_cap = (uint32_t)exc_cap;
			p3.support_miss = reinterpret_cast<int *>(tot + 5); p3.exc_miss = reinterpret_cast<int *>(tot + 5) + 1;
			p3.cig_bytes = T.cig_bytes; p3.cig_miss = reinterpret_cast<int *>(tot + 6);
			// [6] high half: "a value no narrow row holds", [7] the operations of all clusters | position escapes outside the tiles' places << 32
			p3.wire = T.wire; p3.row = P<WireRow>(T.o_row); p3.pos_esc = P<uint64_t>(T.o_pesc); p3.pos_esc_cap = (uint32_t)pesc_cap_of(E);
			p3.wire_miss = reinterpret_cast<int *>(tot + 6) + 1; p3.ops_total = reinterpret_cast<uint32_t *>(tot + 7); p3.pos_esc_count = reinterpret_cast<unsigned int *>(tot + 7) + 1;
		}
		HIPCHECK(c, hipMemsetAsync(tot, 0, 64, c->st));
		if (track) HIPCHECK(c, hipMemsetAsync(C.qual_seen.p, 0, 32, c->st));
		if (T.packed && T.qual_bits != 8) HIPCHECK(c, hipMemcpyAsync(C.qual_lut.p, C.h_qual_lut.p, 256, hipMemcpyHostToDevice, c->st));
		// format 3, the kernel without the LDS stage: two qualities per table look-up - for alphabets below phred 64 (every sequencer's)
		bool direct = fmt3 && !track;
		if (direct && T.qual_bits != 8) {
			for (int v = 64; v < 256; ++v) if (lut[v] != 0xff) direct = false;
			pa.tri_mul = 0;
			if (direct && T.qual_group == 3) {
				pa.tri_mul = build_triple_lut(T, P<uint32_t>(C.h_pair_lut));
				if (pa.tri_mul) HIPCHECK(c, hipMemcpyAsync(C.pair_lut.p, C.h_pair_lut.p, 16384, hipMemcpyHostToDevice, c->st));
				else direct = false; // (never seen; the staged kernel takes the shape at run time)
			} else if (direct) {
				build_pair_lut(T, lut, P<uint16_t>(C.h_pair_lut));
				HIPCHECK(c, hipMemcpyAsync(C.pair_lut.p, C.h_pair_lut.p, 8192, hipMemcpyHostToDevice, c->st));
			}
		}
		uint8_t *os = P<uint8_t>(T.o_str);
		PackDesc *dsc = P<PackDesc>(C.o_desc);
		// format 3: the scans behind the rows' columns over tiles of 256 slots (k_cluster_tile_sums, k_cluster_cols3_tiles); SSV_PACK_COLS=split: two words per slot,
		// two device-wide scans, then the columns, as before round 6
		static const bool split_cols = [] { const char *e = getenv("SSV_PACK_COLS"); return e && !strcmp(e, "split"); }();
		if (fmt3 && !split_cols) {
			const unsigned tiles = grid_for(E, BLOCK);
			const int64_t stride = ((int64_t)tiles + 63) & ~63ll;
			CHECK(ensure(c, C.tile_sums, (size_t)stride * 3 * 8));
			TileSums ts;
			ts.clusters = P<uint64_t>(C.tile_sums); ts.cig = ts.clusters + stride; ts.bytes = ts.cig + stride;
			k_cluster_tile_sums<<<tiles, BLOCK, 0, c->st>>>(pa, ts, T.wire);
			k_scan_sums_lists<uint64_t><<<3, BLOCK, 0, c->st>>>(ts.clusters, (int64_t)tiles, stride);
			k_cluster_cols3_tiles<<<tiles, BLOCK, 0, c->st>>>(pa, p3, dsc, P<uint32_t>(T.o_cig), ts, tot);
		} else {
			k_cluster_meta<<<grid_for(E, BLOCK), BLOCK, 0, c->st>>>(pa);
			exclusive_scan<uint64_t, uint64_t>(c->st, pa.slot_cnt, pa.slot_cnt, E, 0ull, P<uint64_t>(c->scan_scratch64), tot);
			exclusive_scan<uint64_t, uint64_t>(c->st, pa.slot_bytes, pa.slot_bytes, E, 0ull, P<uint64_t>(c->scan_scratch64), tot + 1);
			if (fmt3) k_cluster_cols3<<<grid_for(E, BLOCK), BLOCK, 0, c->st>>>(pa, p3, dsc, P<uint32_t>(T.o_cig));
			else k_cluster_cols<<<grid_for(E, BLOCK), BLOCK, 0, c->st>>>(pa, dsc, P<uint32_t>(T.o_cig));
		}
		if (fmt3) pack3_launch(c, T, pa, p3, dsc, reinterpret_cast<const unsigned int *>(tot), os, direct, track);
		else k_cluster_pack_ascii<<<grid_for(E, GROUPS_PER_BLOCK), BLOCK, 0, c->st>>>(pa, os);
		HIPCHECK(c, hipGetLastError());
		HIPCHECK(c, hipMemcpyAsync(c->h_totals.p, c->totals.p, 64, hipMemcpyDeviceToHost, c->st));
		if (track) HIPCHECK(c, hipMemcpyAsync(h_seen, C.qual_seen.p, 32, hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
		if (fmt3 && attempt <= 6) {
			// (rare) a cluster with more than 65535 reads: the support column as u32; more bases outside A/C/G/T than the exception list takes:
			// the base streams at 4 bits
			const uint64_t m = h_tot[5];
			if ((uint32_t)(h_tot[6] >> 32) && T.wire) { T.wire = 0; continue; } // a length of 256 or more, a support of 255 or more, a CIGAR of 64 operations or more: the columns themselves
			if ((uint32_t)m && T.support_bytes == 2) { T.support_bytes = 4; continue; }
			if ((uint32_t)(m >> 32) && T.base_bits == 2) { T.base_bits = 4; continue; }
			if ((uint32_t)h_tot[6] && T.cig_bytes == 2) { T.cig_bytes = 4; continue; } // an operation of 4096 bases or more (a long N / D)
		}
		if (track) { // the launch above met every quality value of the table's strings: that is the alphabet; pack once more with it
			memcpy(guess, h_seen, 32);
			set_alphabet(T, fmt3, guess, lut);
			track = false;
			continue;
		}
		if (fmt3 && T.qual_bits != 8 && (int)h_tot[3] != 0) {
			// the table's strings hold a quality value that the first events did not show: find out which values there are
			if (attempt > 8) { c->err = "quality alphabet did not settle"; return SSV_E_HIP; }
			track = true;
			continue;
		}
		break;
	}
	T.n_clusters = (int64_t)(uint32_t)h_tot[0]; T.wire_ops = h_tot[0] >> 32; T.cig_ops = T.wire ? (uint64_t)(uint32_t)h_tot[7] : T.wire_ops; T.str_bytes = h_tot[1];
	if (T.wire) { T.pesc_tiles = (int64_t)grid_for(E, BLOCK); T.pesc_extra = (int64_t)(h_tot[7] >> 32); }
	if (fmt3) { T.n_runs = (int64_t)(uint32_t)h_tot[4]; T.n_exc = (int64_t)(h_tot[4] >> 32); }
	return SSV_OK;
}

// ---- the helper thread: what the host makes of a compact table's small pieces, while its strings are still crossing ----

static int table_expand_columns(ssv_ctx *c, TableSet &T, int32_t n_threads, std::string &err);

// put the runs (appended by whichever thread came first) and the exception lists in order
static void table_order(TableSet &T)
{
	ssv_table_run *r = reinterpret_cast<ssv_table_run *>(T.h_runs.p);
	std::sort(r, r + T.n_runs, [](const ssv_table_run &a, const ssv_table_run &b) { return a.first < b.first; });
	uint64_t *e = P<uint64_t>(T.h_exc);
	std::sort(e, e + T.n_exc);
	if (T.wire) { // the tiles' places are in order already, with holes: close them up, then merge the few others in
		uint64_t *pe = P<uint64_t>(T.h_pesc);
		int64_t m = 0;
		for (int64_t k = 0; k < T.pesc_tiles; ++k) if (pe[k] != ~0ull) pe[m++] = pe[k];
		std::sort(pe + T.pesc_tiles, pe + T.pesc_tiles + T.pesc_extra);
		std::copy(pe + T.pesc_tiles, pe + T.pesc_tiles + T.pesc_extra, pe + m);
		std::inplace_merge(pe, pe + m, pe + m + T.pesc_extra);
		T.n_pesc = m + T.pesc_extra;
	}
	T.ordered = true;
}

// one table set's job: wait for the small pieces, order the lists, rebuild the handed-out columns from the rows, and the expanded columns if this context's caller asks for them
static void table_job(ssv_ctx *c, TableSet &T)
{
	ssv_clip_state &C = *c->clip;
	if (T.via_link) link_wait(c, T.copied_sig);
	else if (hipEventSynchronize(T.small_ev) != hipSuccess) { (void)hipGetLastError(); T.job_rc = SSV_E_HIP; T.job_err = "compact table: waiting for the copy of the small columns failed"; return; }
	table_order(T);
	std::lock_guard<std::mutex> lk(C.pool_mu);
	const int64_t n = T.n_clusters;
	const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)(T.job_expand_nt > 0 ? T.job_expand_nt : (int32_t)effective_cpus()), 64, n / 32768 + 1}));
	if (T.wire) {
		WireIn in{P<WireRow>(T.h_row), n, P<uint64_t>(T.h_pesc), T.n_pesc, T.h_cig.p, T.cig_bytes, T.wire_ops};
		WireOut out{reinterpret_cast<int32_t *>(T.r_pos.p), T.r_len.p, T.len_bytes, T.r_sup.p, T.support_bytes, T.r_nc.p, T.ncig_bytes, T.r_cig.p, T.cig_ops};
		if (wire_rebuild(in, out, nt, [&](int k, const std::function<void(int)> &f) { C.pool.run(k, f); })) {
			T.job_rc = SSV_E_HIP; T.job_err = "compact table: the wire rows do not add up to the table";
			return;
		}
	}
	if (T.job_expand_nt >= 0) T.job_rc = table_expand_columns(c, T, T.job_expand_nt, T.job_err);
}

static void table_helper_main(ssv_ctx *c)
{
	TableHelper &H = c->clip->helper;
	(void)hipSetDevice(c->device);
	for (;;) {
		int which;
		{
			std::unique_lock<std::mutex> lk(H.mu);
			H.cv_go.wait(lk, [&] { return H.quit || !H.jobs.empty(); });
			if (H.jobs.empty()) return;
			which = H.jobs.front(); H.jobs.pop_front();
		}
		table_job(c, c->clip->tab[which]);
		{ std::unique_lock<std::mutex> lk(H.mu); c->clip->tab[which].job_pending = false; }
		H.cv_done.notify_all();
	}
}

static void table_job_start(ssv_ctx *c, int which)
{
	TableHelper &H = c->clip->helper;
	if (!H.th.joinable()) H.th = std::thread(table_helper_main, c);
	{ std::unique_lock<std::mutex> lk(H.mu); c->clip->tab[which].job_pending = true; H.jobs.push_back(which); }
	H.cv_go.notify_all();
}

// the helper is done with the set (what it found is in T.job_rc / job_err)
static void table_job_join(ssv_ctx *c, TableSet &T)
{
	TableHelper &H = c->clip->helper;
	std::unique_lock<std::mutex> lk(H.mu);
	H.cv_done.wait(lk, [&] { return !T.job_pending; });
}

// (ssv_ctx_destroy) let the queued jobs end, then the thread
static void table_helper_stop(ssv_ctx *c)
{
	TableHelper &H = c->clip->helper;
	if (!H.th.joinable()) return;
	{ std::unique_lock<std::mutex> lk(H.mu); H.quit = true; }
	H.cv_go.notify_all();
	H.th.join();
}

// 5. the table goes to pinned host memory behind the pack kernels - on the named SDMA engine of the direction, else on the copy stream -, the small pieces first and on a
//    completion of their own: the helper thread works on them while the string block crosses.  ssv_clip_table_wait() waits for both
static int table_copy_out(ssv_ctx *c, int which)
{
	TableSet &T = c->clip->tab[which];
	const bool fmt3 = T.format == 3;
	const size_t nc = (size_t)T.n_clusters;
	struct CopyItem { HBuf *h; const void *d; size_t bytes; int piece; };
	std::vector<CopyItem> cp;
	const CopyItem str{&T.h_str, T.o_str.p, (size_t)T.str_bytes, 6};
	if (fmt3 && T.wire)
		cp = {{&T.h_row, T.o_row.p, nc * sizeof(WireRow), 0}, {&T.h_qmiss, T.o_qmiss.p, nc, 1}, {&T.h_cig, T.o_cig.p, (size_t)T.wire_ops * (size_t)T.cig_bytes, 2},
		      {&T.h_runs, T.o_runs.p, (size_t)T.n_runs * sizeof(TableRun), 3}, {&T.h_exc, T.o_exc.p, (size_t)T.n_exc * 8, 4},
		      {&T.h_pesc, T.o_pesc.p, (size_t)(T.pesc_tiles + T.pesc_extra) * 8, 5}, str}; // (the tiles' places and the list behind them are one piece of memory)
	else if (fmt3)
		cp = {{&T.h_pos, T.o_pos.p, nc * 4, 0}, {&T.h_len, T.o_len.p, nc * 2 * (size_t)T.len_bytes, 0}, {&T.h_sup, T.o_sup.p, nc * (size_t)T.support_bytes, 0},
		      {&T.h_nc, T.o_nc.p, nc * (size_t)T.ncig_bytes, 0}, {&T.h_qmiss, T.o_qmiss.p, nc, 1}, {&T.h_cig, T.o_cig.p, (size_t)T.cig_ops * (size_t)T.cig_bytes, 2},
		      {&T.h_runs, T.o_runs.p, (size_t)T.n_runs * sizeof(TableRun), 3}, {&T.h_exc, T.o_exc.p, (size_t)T.n_exc * 8, 4}, str};
	else
		cp = {{&T.h_tid, T.o_tid.p, nc * 4, 0}, {&T.h_pos, T.o_pos.p, nc * 4, 0}, {&T.h_side, T.o_side.p, nc, 0}, {&T.h_support, T.o_support.p, nc * 4, 0},
		      {&T.h_ll, T.o_ll.p, nc * 4, 0}, {&T.h_lr, T.o_lr.p, nc * 4, 0}, {&T.h_qmiss, T.o_qmiss.p, nc, 1}, {&T.h_stroff, T.o_stroff.p, nc * 8, 0},
		      {&T.h_cigoff, T.o_cigoff.p, nc * 8, 0}, {&T.h_ncig, T.o_ncig.p, nc * 4, 0}, {&T.h_cig, T.o_cig.p, (size_t)T.cig_ops * 4, 2}, str};
	for (auto &x : cp) { CHECK(ensure_host(c, *x.h, x.bytes + 16)); T.wire_piece[x.piece] += x.bytes; }
	if (fmt3 && T.wire) {
		if (!T.r_pos.ensure(nc * 4 + 16) || !T.r_len.ensure(nc * 2 * (size_t)T.len_bytes + 16) || !T.r_sup.ensure(nc * (size_t)T.support_bytes + 16) || !T.r_nc.ensure(nc * (size_t)T.ncig_bytes + 16) ||
		    !T.r_cig.ensure((size_t)T.cig_ops * (size_t)T.cig_bytes + 16)) { c->err = "out of host memory for the cluster table's columns"; return SSV_E_NOMEM; }
		T.v_pos = T.r_pos.p; T.v_len = T.r_len.p; T.v_sup = T.r_sup.p; T.v_nc = T.r_nc.p; T.v_cig = T.r_cig.p;
	} else { T.v_pos = T.h_pos.p; T.v_len = T.h_len.p; T.v_sup = T.h_sup.p; T.v_nc = T.h_nc.p; T.v_cig = T.h_cig.p; }
	T.via_link = false;
	if (c->link.ok) {
		// (the pack kernels are done: cluster_pack left through a synchronisation of the stream.)  Every piece on the engine of the direction; copied_sig counts the small
		// ones down, the string block has a signal of its own (it is the one that is timed)
		const CopyItem *big = cp.back().bytes ? &cp.back() : nullptr;
		int64_t small = 0;
		for (auto &x : cp) if (x.bytes && &x != big) ++small;
		T.big_bytes = big ? big->bytes : 0;
		c->link.signal_store(T.copied_sig, small);
		c->link.signal_store(T.big_sig, big ? 1 : 0);
		const char *re = getenv("SSV_LINK_REFUSE_AFTER"); // (tests: the engine takes that many pieces of every table, then refuses)
		const int64_t refuse_after = re ? (int64_t)atoll(re) : -1;
		int64_t started_small = 0;
		bool big_started = false, refused = false;
		for (auto &x : cp) if (x.bytes) {
			if ((refuse_after >= 0 && started_small + (big_started ? 1 : 0) >= refuse_after) || !link_copy(c, x.h->p, x.d, x.bytes, true, &x == big ? T.big_sig : T.copied_sig)) { refused = true; break; }
			if (&x == big) big_started = true; else ++started_small;
		}
		if (!refused) T.via_link = true;
		else {
			// an engine that refuses: let what was started land, then copy everything the runtime's way.  The pieces under way count their signal down while we stand here:
			// it is done when it shows the number of pieces that never started, and only then is it ours to set
			while (c->link.signal_wait(T.copied_sig, HSA_SIGNAL_CONDITION_EQ, small - started_small, UINT64_MAX, HSA_WAIT_STATE_BLOCKED) != small - started_small) {}
			while (c->link.signal_wait(T.big_sig, HSA_SIGNAL_CONDITION_EQ, big && !big_started ? 1 : 0, UINT64_MAX, HSA_WAIT_STATE_BLOCKED) != (big && !big_started ? 1 : 0)) {}
			c->link.signal_store(T.copied_sig, 0); c->link.signal_store(T.big_sig, 0);
			T.big_bytes = 0;
			c->link.ok = false;
		}
	}
	if (!T.via_link) {
		HIPCHECK(c, hipEventRecord(T.packed_ev, c->st));
		HIPCHECK(c, hipStreamWaitEvent(c->st_copy, T.packed_ev, 0));
		for (auto &x : cp) if (x.bytes && &x != &cp.back()) HIPCHECK(c, hipMemcpyAsync(x.h->p, x.d, x.bytes, hipMemcpyDeviceToHost, c->st_copy));
		HIPCHECK(c, hipEventRecord(T.small_ev, c->st_copy));
		if (cp.back().bytes) HIPCHECK(c, hipMemcpyAsync(cp.back().h->p, cp.back().d, cp.back().bytes, hipMemcpyDeviceToHost, c->st_copy));
		HIPCHECK(c, hipEventRecord(T.copied, c->st_copy));
	}
	T.in_flight = true;
	static const bool timing = [] { const char *e = getenv("SSV_TIMING"); return e ? atoi(e) : 0; }() >= 2;
	if (timing) {
		const uint64_t *w = T.wire_piece;
		fprintf(stderr, "[timing] (cluster table: %lld clusters cross as %llu bytes, %.1f a cluster - %s %llu, flags %llu, CIGAR stream %llu, runs %llu, base exceptions %llu, position escapes %llu, strings %llu)\n",
		        (long long)T.n_clusters, (unsigned long long)(w[0] + w[1] + w[2] + w[3] + w[4] + w[5] + w[6]), (double)(w[0] + w[1] + w[2] + w[3] + w[4] + w[5] + w[6]) / (double)T.n_clusters,
		        T.wire ? "narrow rows" : "columns", (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2], (unsigned long long)w[3], (unsigned long long)w[4], (unsigned long long)w[5], (unsigned long long)w[6]);
	}
	if (fmt3) { T.job_expand_nt = c->clip->expand_nt; table_job_start(c, which); }
	return SSV_OK;
}

// 6. size the other table set like this one now (pinning ~2 GB of host memory takes ~100 ms: better here than in the caller's next pass)
static int table_presize(ssv_ctx *c, const TableSet &T, TableSet &O)
{
	const size_t nc = (size_t)T.n_clusters, E = (size_t)T.n_events, str_total = (size_t)T.str_bytes, cig_total = (size_t)T.cig_ops, sum_ncig = (size_t)c->clip->sum_ncig;
	struct Item { HBuf *h; DBuf *d; size_t bytes, dbytes; };
	std::vector<Item> oc;
	if (T.format == 3)
		oc = {{&O.h_pos, &O.o_pos, nc * 4, E * 4}, {&O.h_len, &O.o_len, nc * 2 * (size_t)T.len_bytes, E * 8}, {&O.h_sup, &O.o_sup, nc * (size_t)T.support_bytes, E * 4},
		      {&O.h_nc, &O.o_nc, nc * (size_t)T.ncig_bytes, E * 2}, {&O.h_qmiss, &O.o_qmiss, nc, E}, {&O.h_str, &O.o_str, str_total, T.o_str.cap - 16},
		      {&O.h_cig, &O.o_cig, cig_total * 4, sum_ncig * 4}, {&O.h_runs, &O.o_runs, (size_t)T.n_runs * sizeof(TableRun), E * sizeof(TableRun)},
		      {&O.h_exc, &O.o_exc, (size_t)T.n_exc * 8, (size_t)exc_cap_of((int64_t)E) * 8}};
	if (T.format == 3 && T.wire) {
		oc.push_back({&O.h_row, &O.o_row, nc * sizeof(WireRow), E * sizeof(WireRow)});
		oc.push_back({&O.h_pesc, &O.o_pesc, (size_t)(T.pesc_tiles + T.pesc_extra) * 8, pesc_bytes_of((int64_t)E) - 16});
	}
	if (T.format != 3)
		oc = {{&O.h_tid, &O.o_tid, nc * 4, E * 4}, {&O.h_pos, &O.o_pos, nc * 4, E * 4}, {&O.h_side, &O.o_side, nc, E}, {&O.h_support, &O.o_support, nc * 4, E * 4},
		      {&O.h_ll, &O.o_ll, nc * 4, E * 4}, {&O.h_lr, &O.o_lr, nc * 4, E * 4}, {&O.h_qmiss, &O.o_qmiss, nc, E}, {&O.h_stroff, &O.o_stroff, nc * 8, E * 8},
		      {&O.h_cigoff, &O.o_cigoff, nc * 8, E * 8}, {&O.h_ncig, &O.o_ncig, nc * 4, E * 4}, {&O.h_str, &O.o_str, str_total, T.o_str.cap - 16},
		      {&O.h_cig, &O.o_cig, cig_total * 4, sum_ncig * 4}};
	for (auto &x : oc) {
		if (x.h->cap < x.bytes + 16) CHECK(ensure_host(c, *x.h, x.bytes + 16));
		if (x.d->cap < x.dbytes + 16) { // (exactly this size, and nothing of the old contents kept: not ensure())
			DBuf nb;
			HIPCHECK(c, dev_malloc(c, &nb.p, x.dbytes + 16));
			nb.cap = x.dbytes + 16;
			HIPCHECK(c, x.d->release());
			*x.d = std::move(nb);
		}
	}
	return SSV_OK;
}

static bool probes_set(const ssv_ctx *c);                // probe_api.inc: ssv_clip_probe_set has left probes
static int probe_after_pack(ssv_ctx *c, TableSet &T);   // ... which look at every pass's table where it lies

int ssv_clip_cluster_async(ssv_ctx *c, int64_t *n_clusters, int64_t *n_events)
{
	if (!c) return SSV_E_ARG;
	ssv_clip_state &C = *c->clip;
	if (!C.active) { c->err = "ssv_clip_cluster before ssv_clip_begin"; return SSV_E_STATE; }
	if (probes_set(c) && C.table_mode != 0) { c->err = "ssv_clip_cluster: the probes of ssv_clip_probe_set read the ASCII table (ssv_clip_table_format 0), not format 3"; return SSV_E_ARG; }
	HIPCHECK(c, hipSetDevice(c->device));
	// take the table set that is not the most recent one; its previous copy (two calls ago) must have landed
	const int s_ = C.tab_cur ^ 1;
	TableSet &T = C.tab[s_];
	table_job_join(c, T); // (the helper may still be at work on the set's last table)
	if (T.in_flight) { if (T.via_link) table_link_wait(c, T); else HIPCHECK(c, hipEventSynchronize(T.copied)); T.in_flight = false; }
	C.tab_cur = s_;
	const int64_t E = C.n_events;
	table_begin(C, T, E);
	if (n_events) *n_events = E;
	if (n_clusters) *n_clusters = 0;
	if (E == 0) { if (probes_set(c)) CHECK(probe_after_pack(c, T)); HIPCHECK(c, hipStreamSynchronize(c->st)); return SSV_OK; } // (an empty pass is a pass: the probes count it)
	CHECK(ensure(c, c->totals, 128)); CHECK(ensure_host(c, c->h_totals, 128));
	CHECK(ensure(c, C.qual_seen, 32)); CHECK(ensure(c, C.qual_lut, 256)); CHECK(ensure_host(c, C.h_qual_lut, 256));
	CHECK(ensure(c, C.pair_lut, 16384)); CHECK(ensure_host(c, C.h_pair_lut, 16384)); // (pairs: 4096 halves; triples: 4096 dwords)
	int cur = 0;
	CHECK(cluster_sort(c, T.format == 3, &cur));
	ClusterArgs ca;
	CHECK(cluster_bins(c, cur, ca));
	CHECK(cluster_pack(c, T, ca));
	if (n_clusters) *n_clusters = T.n_clusters;
	if (probes_set(c)) CHECK(probe_after_pack(c, T));
	if (T.n_clusters == 0) return SSV_OK;
	CHECK(table_copy_out(c, s_));
	if (!C.tab[s_ ^ 1].in_flight) CHECK(table_presize(c, T, C.tab[s_ ^ 1]));
	return SSV_OK;
}

uint64_t ssv_table_block_bytes(int32_t left_len, int32_t right_len) { return table_block_bytes((uint64_t)left_len, (uint64_t)right_len, 0, 8); }

int ssv_clip_table_format(ssv_ctx *c, int packed)
{
	if (!c) return SSV_E_ARG;
	ssv_clip_state &C = *c->clip;
	if (packed != 0 && packed != 3) { c->err = "ssv_clip_table_format: 0 (ASCII) or 3 (compact); the four-piece packed formats 1 and 2 of ABI versions < 8 are gone"; return SSV_E_ARG; }
	C.table_mode = packed;
	return SSV_OK;
}

// ---- the columns a compact table leaves to the host ----

static void table_expanded_view(TableSet &T, ssv_cluster_table *out)
{
	out->tid = T.x_tid.data(); out->side = T.x_side.data(); out->support = T.x_support.data(); out->left_len = T.x_ll.data(); out->right_len = T.x_lr.data();
	out->qual_missing = T.x_qmiss.data(); out->n_cigar = T.x_ncig.data(); out->str_off = T.x_stroff.data(); out->cigar_off = T.x_cigoff.data();
}

static int table_wait(ssv_ctx *c, int which, ssv_cluster_table *out)
{
	HIPCHECK(c, hipSetDevice(c->device));
	TableSet &T = c->clip->tab[which];
	memset(out, 0, sizeof(*out));
	table_job_join(c, T);
	if (T.in_flight) {
		ProfScope pd(c, P_TABLE_D2H, T.n_clusters); // what is left of the copy when the caller asks for the table
		if (T.via_link) table_link_wait(c, T); else HIPCHECK(c, hipEventSynchronize(T.copied));
		T.in_flight = false;
	}
	out->n_events = T.n_events; out->n_clusters = T.n_clusters; out->seq_packed = T.packed; out->qual_bits = T.qual_bits; out->qual_group = T.qual_group; memcpy(out->qual_alphabet, T.qual_alphabet, sizeof(out->qual_alphabet));
	out->format = T.format; out->base_bits = T.base_bits;
	if (T.n_clusters == 0) return SSV_OK;
	if (T.format == 3) {
		out->len_bytes = T.len_bytes; out->support_bytes = T.support_bytes; out->ncig_bytes = T.ncig_bytes;
		if (T.job_rc != SSV_OK) { c->err = T.job_err; return T.job_rc; } // (the helper thread ordered the lists and rebuilt the columns behind the small pieces' copy)
		out->pos = static_cast<const int32_t *>(T.v_pos); out->c_len = T.v_len; out->c_support = T.v_sup; out->c_ncig = T.v_nc; out->c_flags = P<uint8_t>(T.h_qmiss);
		out->str = P<uint8_t>(T.h_str); out->cigar = T.cig_bytes == 4 ? static_cast<const uint32_t *>(T.v_cig) : nullptr; out->c_cigar = T.v_cig; out->cigar_bytes = T.cig_bytes; out->str_bytes = T.str_bytes; out->cigar_ops = T.cig_ops;
		out->runs = reinterpret_cast<const ssv_table_run *>(T.h_runs.p); out->n_runs = T.n_runs;
		out->base_exc = P<uint64_t>(T.h_exc); out->n_base_exc = T.n_exc;
		if (T.expanded) { table_expanded_view(T, out); out->support_sum = T.support_sum; }
		return SSV_OK;
	}
	out->str_bytes = T.str_bytes; out->cigar_ops = T.cig_ops;
	out->tid = P<int32_t>(T.h_tid); out->pos = P<int32_t>(T.h_pos); out->side = P<uint8_t>(T.h_side); out->support = P<int32_t>(T.h_support);
	out->left_len = P<int32_t>(T.h_ll); out->right_len = P<int32_t>(T.h_lr); out->qual_missing = P<uint8_t>(T.h_qmiss); out->str_off = P<uint64_t>(T.h_stroff);
	out->str = P<uint8_t>(T.h_str); out->cigar_off = P<uint64_t>(T.h_cigoff); out->n_cigar = P<int32_t>(T.h_ncig); out->cigar = P<uint32_t>(T.h_cig);
	out->c_cigar = T.h_cig.p; out->cigar_bytes = 4;
	return SSV_OK;
}

int ssv_clip_table_wait(ssv_ctx *c, ssv_cluster_table *out) { return c && out ? table_wait(c, c->clip->tab_cur, out) : SSV_E_ARG; }
int ssv_clip_table_wait_prev(ssv_ctx *c, ssv_cluster_table *out) { return c && out ? table_wait(c, c->clip->tab_cur ^ 1, out) : SSV_E_ARG; }

// one range of clusters: the widened columns (pass 1, also the range's string bytes / CIGAR operations / support sum), then the offsets (pass 2)
template <class LenT, class SupT, class NcT>
static void expand_range(TableSet &T, int64_t k0, int64_t k1, bool second, uint64_t &so, uint64_t &co, int64_t &ssum)
{
	const LenT *len = reinterpret_cast<const LenT *>(T.v_len);
	const SupT *sup = reinterpret_cast<const SupT *>(T.v_sup);
	const NcT *ncg = reinterpret_cast<const NcT *>(T.v_nc);
	const uint8_t *fl = P<uint8_t>(T.h_qmiss);
	const uint64_t bb = (uint64_t)T.base_bits, qb = (uint64_t)T.qual_bits, qg = (uint64_t)T.qual_group;
	int32_t *x_ll = T.x_ll.data(), *x_lr = T.x_lr.data(), *x_sup = T.x_support.data(), *x_nc = T.x_ncig.data();
	uint8_t *x_qm = T.x_qmiss.data();
	uint64_t *x_so = T.x_stroff.data(), *x_co = T.x_cigoff.data();
	if (!second) {
		int64_t sum = 0;
		for (int64_t k = k0; k < k1; ++k) {
			const uint32_t ll = len[2 * k], lr = len[2 * k + 1], nc1 = ncg[k], s1 = sup[k];
			x_ll[k] = (int32_t)ll; x_lr[k] = (int32_t)lr; x_sup[k] = (int32_t)s1; x_nc[k] = (int32_t)nc1; x_qm[k] = fl[k] & 1;
			const uint64_t n = (uint64_t)ll + lr;
			so += 4ull * ((n * bb + 31) / 32 + (qual_stream_bits(n, qb, qg) + 31) / 32); co += nc1; sum += s1;
		}
		ssum = sum;
		return;
	}
	for (int64_t k = k0; k < k1; ++k) {
		x_so[k] = so; x_co[k] = co;
		const uint64_t n = (uint64_t)(uint32_t)x_ll[k] + (uint32_t)x_lr[k];
		so += 4ull * ((n * bb + 31) / 32 + (qual_stream_bits(n, qb, qg) + 31) / 32); co += (uint32_t)x_nc[k];
	}
}

// the expanded columns of a format-3 table whose small pieces have landed and whose handed-out columns stand (the caller holds pool_mu)
static int table_expand_columns(ssv_ctx *c, TableSet &T, int32_t n_threads, std::string &err)
{
	ssv_clip_state &C = *c->clip;
	const int64_t n = T.n_clusters;
	if (n == 0 || T.expanded) return SSV_OK;
	T.x_tid.resize((size_t)n); T.x_side.resize((size_t)n); T.x_support.resize((size_t)n); T.x_ll.resize((size_t)n); T.x_lr.resize((size_t)n); T.x_qmiss.resize((size_t)n);
	T.x_ncig.resize((size_t)n); T.x_stroff.resize((size_t)n); T.x_cigoff.resize((size_t)n);
	const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)(n_threads > 0 ? n_threads : (int32_t)effective_cpus()), 64, n / 32768 + 1}));
	const ssv_table_run *runs = reinterpret_cast<const ssv_table_run *>(T.h_runs.p);
	const int64_t n_runs = T.n_runs;
	std::vector<uint64_t> part_str((size_t)nt + 1, 0), part_cig((size_t)nt + 1, 0);
	std::vector<int64_t> part_sup((size_t)nt, 0);
	// pass 1 (widened columns, per-range sums, contig / side), the ranges' starting offsets, pass 2 (offsets)
	auto pass = [&](int w, int second) {
		const int64_t k0 = n * w / nt, k1 = n * (w + 1) / nt;
		uint64_t so = second ? part_str[(size_t)w] : 0, co = second ? part_cig[(size_t)w] : 0;
		int64_t ssum = 0;
		if (T.len_bytes == 2) {
			if (T.support_bytes == 2) { if (T.ncig_bytes == 1) expand_range<uint16_t, uint16_t, uint8_t>(T, k0, k1, second, so, co, ssum); else expand_range<uint16_t, uint16_t, uint16_t>(T, k0, k1, second, so, co, ssum); }
			else { if (T.ncig_bytes == 1) expand_range<uint16_t, uint32_t, uint8_t>(T, k0, k1, second, so, co, ssum); else expand_range<uint16_t, uint32_t, uint16_t>(T, k0, k1, second, so, co, ssum); }
		} else {
			if (T.support_bytes == 2) { if (T.ncig_bytes == 1) expand_range<uint32_t, uint16_t, uint8_t>(T, k0, k1, second, so, co, ssum); else expand_range<uint32_t, uint16_t, uint16_t>(T, k0, k1, second, so, co, ssum); }
			else { if (T.ncig_bytes == 1) expand_range<uint32_t, uint32_t, uint8_t>(T, k0, k1, second, so, co, ssum); else expand_range<uint32_t, uint32_t, uint16_t>(T, k0, k1, second, so, co, ssum); }
		}
		if (second) return;
		part_str[(size_t)w + 1] = so; part_cig[(size_t)w + 1] = co; part_sup[(size_t)w] = ssum;
		// contig / side of the range: whole runs at a time
		int64_t lo = 0, hi = n_runs;
		while (hi - lo > 1) { const int64_t m = (lo + hi) / 2; if (runs[m].first <= k0) lo = m; else hi = m; }
		for (int64_t r = lo; r < n_runs && runs[r].first < k1; ++r) {
			const int64_t a = std::max(k0, runs[r].first), b = std::min(k1, r + 1 < n_runs ? runs[r + 1].first : n);
			if (b > a) { std::fill(T.x_tid.begin() + a, T.x_tid.begin() + b, runs[r].tid); std::fill(T.x_side.begin() + a, T.x_side.begin() + b, runs[r].side); }
		}
	};
	C.pool.run(nt, [&](int w) { pass(w, 0); });
	for (int v = 0; v < nt; ++v) { part_str[(size_t)v + 1] += part_str[(size_t)v]; part_cig[(size_t)v + 1] += part_cig[(size_t)v]; }
	C.pool.run(nt, [&](int w) { pass(w, 1); });
	if (part_str[(size_t)nt] != T.str_bytes || part_cig[(size_t)nt] != T.cig_ops) { err = "compact table: the rebuilt offsets do not add up to the blob sizes"; return SSV_E_HIP; }
	T.support_sum = 0;
	for (int64_t v : part_sup) T.support_sum += v;
	T.expanded = true;
	return SSV_OK;
}

int ssv_clip_table_expand(ssv_ctx *c, ssv_cluster_table *t, int32_t n_threads)
{
	if (!c || !t) return SSV_E_ARG;
	ssv_clip_state &C = *c->clip;
	TableSet *Tp = nullptr;
	for (auto &x : C.tab) if (x.format == 3 && !x.in_flight && x.n_clusters == t->n_clusters && (t->n_clusters == 0 || t->pos == static_cast<const int32_t *>(x.v_pos))) Tp = &x;
	if (t->format != 3 || !Tp) { c->err = "ssv_clip_table_expand takes a compact (format 3) table handed out by ssv_clip_table_wait"; return SSV_E_ARG; }
	TableSet &T = *Tp;
	C.expand_nt = std::max(0, n_threads); // this context's caller wants the expanded columns: from now on the helper thread builds them with the others
	if (T.n_clusters && !T.expanded) {
		std::lock_guard<std::mutex> lk(C.pool_mu); // (the helper may be at work on the other table set)
		CHECK(table_expand_columns(c, T, n_threads, c->err));
	}
	if (T.n_clusters) table_expanded_view(T, t);
	t->support_sum = T.support_sum;
	return SSV_OK;
}

int ssv_clip_table_wire_bytes(ssv_ctx *c, const ssv_cluster_table *t, ssv_table_wire *out)
{
	if (!c || !t || !out) return SSV_E_ARG;
	memset(out, 0, sizeof(*out));
	if (t->n_clusters == 0) return SSV_OK;
	const TableSet *Tp = nullptr;
	for (auto &x : c->clip->tab) if (!x.in_flight && x.format == t->format && x.n_clusters == t->n_clusters && t->pos == static_cast<const int32_t *>(x.v_pos)) Tp = &x;
	if (!Tp) { c->err = "ssv_clip_table_wire_bytes takes a table handed out by ssv_clip_table_wait"; return SSV_E_ARG; }
	const uint64_t *w = Tp->wire_piece;
	out->narrow = Tp->wire;
	out->rows = w[0]; out->flags = w[1]; out->cigar = w[2]; out->runs = w[3]; out->base_exc = w[4]; out->pos_esc = w[5]; out->str = w[6];
	for (int k = 0; k < 7; ++k) out->total += w[k];
	return SSV_OK;
}

uint64_t ssv_table_block_bytes3(int64_t n_bases, int32_t base_bits, int32_t qual_bits) { return table3_block_bytes((uint64_t)n_bases, base_bits, qual_bits); }
uint64_t ssv_table_block_bytes3g(int64_t n_bases, int32_t base_bits, int32_t qual_bits, int32_t qual_group) { return table3_block_bytes((uint64_t)n_bases, base_bits, qual_bits, qual_group > 1 ? qual_group : 1); }

int ssv_clip_cluster(ssv_ctx *c, ssv_cluster_table *out)
{
	if (!c || !out) return SSV_E_ARG;
	CHECK(ssv_clip_cluster_async(c, nullptr, nullptr));
	return ssv_clip_table_wait(c, out);
}

