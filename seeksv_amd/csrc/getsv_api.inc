// getsv_api.inc - C ABI of getsv's discordant tally + depth pass (included by seeksv_hip.hip; kernels in getsv_kernels.h)

struct ssv_getsv_state {
	bool active = false;
	ssv_getsv_params p{};
	std::vector<DevJunction> junc;
	std::vector<ssv_interval> win;
	std::vector<int32_t> tlen;
	std::vector<int64_t> ctg_tile_off;
	int32_t map_span = -1;
	int32_t wmax = 0;
	int64_t diff_len = 0;
	DBuf djunc, counts, wtid, wbeg, wend, woff, diff, tilemap, tile_win, tile_junc, ctgoff, maxdepth, span;
	DBuf q_tid, q_out64;
	// read cap of the reference's pileup (k_cap_*): flags, per-tile marks, carried sweep state + ring, the stream's last records (ping-pong)
	DBuf dense_list, cap_flags, cap_deep, cap_carry, cap_ring, cap_ring_tmp, cap_tail[2][4];
	int32_t cap_tail_n = 0, cap_tail_cur = 0, cap_ring_mask = 0;
	HBuf h_q;
};

// ssv_batch_t.tid_runs -> the kernel's table (checked: a wrong run list would silently move records to another contig)
static int fill_runs(ssv_ctx *c, const ssv_batch_t *b, RunTab &R)
{
	memset(&R, 0, sizeof(R));
	if (!b->tid_runs || b->n_tid_runs <= 0 || b->n_tid_runs > RUN_MAX || getenv("SSV_NO_TID_RUNS")) return SSV_OK;
	const int64_t k = b->n_tid_runs;
	if (b->tid_runs[0].first != 0) { c->err = "tid_runs must start at record 0"; return SSV_E_ARG; }
	for (int64_t i = 0; i < k; ++i) {
		if (i && b->tid_runs[i].first <= b->tid_runs[i - 1].first) { c->err = "tid_runs must be strictly increasing"; return SSV_E_ARG; }
		if (b->tid_runs[i].first >= b->n) { c->err = "tid_runs reach past the batch"; return SSV_E_ARG; }
		R.first[i] = b->tid_runs[i].first; R.tid[i] = b->tid_runs[i].tid;
	}
	R.first[k] = b->n; R.n = (int32_t)k;
	return SSV_OK;
}

static int gs_build_tilemap(ssv_ctx *c, int32_t span)
{
	ssv_getsv_state &G = *c->getsv;
	// which 512-bp tiles can hold the start (0-based pos) of a record that overlaps a depth window / is a candidate of a junction window,
	// and where such a record's look-up starts: marked by the windows and junctions themselves, on the device
	const size_t ntile = (size_t)G.ctg_tile_off.back();
	CHECK(ensure(c, G.tilemap, ntile + 16)); CHECK(ensure(c, G.tile_win, ntile * 4 + 16)); CHECK(ensure(c, G.tile_junc, ntile * 4 + 16));
	HIPCHECK(c, hipMemsetAsync(G.tilemap.p, 0, ntile + 16, c->st));
	const int64_t nw = (int64_t)G.win.size(), nj = (int64_t)G.junc.size();
	if (nw) k_tile_mark_windows<<<grid_for(nw, BLOCK), BLOCK, 0, c->st>>>(P<int32_t>(G.wtid), P<int32_t>(G.wbeg), P<int32_t>(G.wend), nw, span, P<int64_t>(G.ctgoff),
	                                                                        G.p.n_targets, P<uint32_t>(G.tilemap), P<uint32_t>(G.tile_win));
	if (nj) k_tile_mark_junctions<<<grid_for(nj, BLOCK), BLOCK, 0, c->st>>>(P<DevJunction>(G.djunc), nj, span, G.wmax, P<int64_t>(G.ctgoff), G.p.n_targets,
	                                                                          P<uint32_t>(G.tilemap), P<uint32_t>(G.tile_junc));
	HIPCHECK(c, hipGetLastError());
	G.map_span = span;
	return SSV_OK;
}

int ssv_getsv_begin(ssv_ctx *c, const ssv_getsv_params *p)
{
	if (!c || !p || p->n_targets < 0 || p->n_junctions < 0 || p->n_windows < 0) return SSV_E_ARG;
	ssv_getsv_state &G = *c->getsv;
	if ((p->n_targets && !p->target_len) || (p->n_junctions && !p->junctions) || (p->n_windows && !p->windows)) return SSV_E_ARG;
	c->pf.clear();
	HIPCHECK(c, hipSetDevice(c->device));
	G.p = *p;
	G.tlen.assign(p->target_len, p->target_len + p->n_targets);
	G.ctg_tile_off.assign((size_t)p->n_targets + 1, 0);
	for (int t = 0; t < p->n_targets; ++t) G.ctg_tile_off[(size_t)t + 1] = G.ctg_tile_off[(size_t)t] + ((int64_t)std::max(0, G.tlen[(size_t)t]) >> TILE_SHIFT) + 1;
	G.map_span = -1;
	// junctions sorted by (up_tid, beg); the window test itself is repeated exactly on the device
	G.junc.clear();
	G.wmax = 0;
	for (int64_t k = 0; k < p->n_junctions; ++k) {
		const ssv_junction &s = p->junctions[k];
		DevJunction j;
		j.up_tid = s.up_tid; j.down_tid = s.down_tid; j.up_pos = s.up_pos; j.down_pos = s.down_pos; j.beg = s.beg; j.end = s.end;
		j.up_strand = s.up_strand; j.down_strand = s.down_strand; j.pad = 0; j.orig = (int32_t)k;
		G.junc.push_back(j);
		if ((int64_t)s.end - s.beg > G.wmax) G.wmax = (int32_t)std::min<int64_t>((int64_t)s.end - s.beg, 0x7fffffff);
	}
	std::stable_sort(G.junc.begin(), G.junc.end(), [](const DevJunction &a, const DevJunction &b) { return a.up_tid != b.up_tid ? a.up_tid < b.up_tid : a.beg < b.beg; });
	G.win.assign(p->windows, p->windows + p->n_windows);
	for (size_t k = 0; k < G.win.size(); ++k) {
		const ssv_interval &w = G.win[k];
		if (w.end < w.beg || (k && (G.win[k - 1].tid > w.tid || (G.win[k - 1].tid == w.tid && G.win[k - 1].end >= w.beg)))) {
			c->err = "depth windows must be sorted, disjoint and non-empty"; return SSV_E_ARG;
		}
	}
	const size_t nj = G.junc.size(), nw = G.win.size();
	std::vector<int32_t> wt(nw), wb(nw), we(nw);
	std::vector<int64_t> wo(nw + 1, 0);
	for (size_t k = 0; k < nw; ++k) { wt[k] = G.win[k].tid; wb[k] = G.win[k].beg; we[k] = G.win[k].end; wo[k + 1] = wo[k] + ((int64_t)we[k] - wb[k] + 1) + 1; }
	G.diff_len = wo[nw];
	CHECK(ensure(c, G.djunc, nj * sizeof(DevJunction) + 16)); CHECK(ensure(c, G.counts, nj * 4 + 16));
	CHECK(ensure(c, G.wtid, nw * 4 + 16)); CHECK(ensure(c, G.wbeg, nw * 4 + 16)); CHECK(ensure(c, G.wend, nw * 4 + 16)); CHECK(ensure(c, G.woff, (nw + 1) * 8));
	CHECK(ensure(c, G.diff, (size_t)G.diff_len * 4 + 16)); CHECK(ensure(c, G.ctgoff, G.ctg_tile_off.size() * 8)); CHECK(ensure(c, G.maxdepth, 16));
	CHECK(ensure(c, G.span, 16));
	if (nj) HIPCHECK(c, hipMemcpyAsync(G.djunc.p, G.junc.data(), nj * sizeof(DevJunction), hipMemcpyHostToDevice, c->st));
	if (nw) {
		HIPCHECK(c, hipMemcpyAsync(G.wtid.p, wt.data(), nw * 4, hipMemcpyHostToDevice, c->st));
		HIPCHECK(c, hipMemcpyAsync(G.wbeg.p, wb.data(), nw * 4, hipMemcpyHostToDevice, c->st));
		HIPCHECK(c, hipMemcpyAsync(G.wend.p, we.data(), nw * 4, hipMemcpyHostToDevice, c->st));
	}
	HIPCHECK(c, hipMemcpyAsync(G.woff.p, wo.data(), (nw + 1) * 8, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemcpyAsync(G.ctgoff.p, G.ctg_tile_off.data(), G.ctg_tile_off.size() * 8, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemsetAsync(G.counts.p, 0, nj * 4 + 16, c->st));
	HIPCHECK(c, hipMemsetAsync(G.diff.p, 0, (size_t)G.diff_len * 4 + 16, c->st));
	HIPCHECK(c, hipMemsetAsync(G.maxdepth.p, 0, 16, c->st));
	CHECK(ensure(c, G.cap_carry, sizeof(CapCarry))); CHECK(ensure(c, G.cap_flags, 16));
	HIPCHECK(c, hipMemsetAsync(G.cap_carry.p, 0, sizeof(CapCarry), c->st));
	G.cap_tail_n = 0; G.cap_tail_cur = 0; G.cap_ring_mask = 0;
	HIPCHECK(c, hipStreamSynchronize(c->st)); // the host vectors above go out of scope
	G.active = true;
	return SSV_OK;
}

// the read cap of the reference's pileup: three small launches that leave at once unless >= 8000 reads can be alive somewhere.
// prime != 0 (ssv_getsv_prime): the batch only rebuilds the bookkeeping (ring of read ends, live count, the stream's last records).
static int cap_launches(ssv_ctx *c, const GetsvArgs &a, const DevBatch &d, int64_t ntiles, int prime)
{
	ssv_getsv_state &G = *c->getsv;
	ProfScope ps(c, P_GETSV_CAND, 0);
	// the ring of read ends covers one reference span; a later batch with a longer read (a long N skip or deletion) makes it grow: the
	// live entries of a sweep that is carried across the batch boundary move to their slots in the larger ring
	if (G.cap_ring_mask == 0 || (int64_t)G.map_span + 2 > (int64_t)G.cap_ring_mask + 1) {
		int64_t e = CAP_LDS_RING;
		while (e < (int64_t)G.map_span + 2) e <<= 1;
		if (e > (1ll << 30)) { c->err = "reference span of a read beyond 2^30"; return SSV_E_RANGE; }
		if (G.cap_ring_mask == 0) CHECK(ensure(c, G.cap_ring, (size_t)e * 4));
		else {
			CHECK(ensure(c, G.cap_ring_tmp, (size_t)e * 4));
			HIPCHECK(c, hipMemsetAsync(G.cap_ring_tmp.p, 0, (size_t)e * 4, c->st));
			k_cap_regrow<<<64, BLOCK, 0, c->st>>>(P<CapCarry>(G.cap_carry), P<int32_t>(G.cap_ring), G.cap_ring_mask, P<int32_t>(G.cap_ring_tmp), (int32_t)(e - 1));
			HIPCHECK(c, hipGetLastError());
			std::swap(G.cap_ring, G.cap_ring_tmp);
		}
		G.cap_ring_mask = (int32_t)(e - 1);
	}
	CHECK(ensure(c, G.cap_deep, (size_t)ntiles + 16));
	for (int s_ = 0; s_ < 2; ++s_) { CHECK(ensure(c, G.cap_tail[s_][0], CAP_TAIL * 4)); CHECK(ensure(c, G.cap_tail[s_][1], CAP_TAIL * 4)); CHECK(ensure(c, G.cap_tail[s_][2], CAP_TAIL * 4)); CHECK(ensure(c, G.cap_tail[s_][3], CAP_TAIL)); }
	CapArgs ca;
	ca.g = a; ca.span = G.map_span; ca.prime = prime;
	DBuf *ot = G.cap_tail[G.cap_tail_cur], *nt = G.cap_tail[G.cap_tail_cur ^ 1];
	ca.tail_tid = P<int32_t>(ot[0]); ca.tail_pos = P<int32_t>(ot[1]); ca.tail_end = P<int32_t>(ot[2]); ca.tail_pass = P<uint8_t>(ot[3]); ca.tail_n = G.cap_tail_n;
	ca.deep = P<uint8_t>(G.cap_deep); ca.ntiles = ntiles; ca.flags = P<int>(G.cap_flags); ca.carry = P<CapCarry>(G.cap_carry);
	ca.ring = P<int32_t>(G.cap_ring); ca.ring_mask = G.cap_ring_mask;
	ca.ntail_tid = P<int32_t>(nt[0]); ca.ntail_pos = P<int32_t>(nt[1]); ca.ntail_end = P<int32_t>(nt[2]); ca.ntail_pass = P<uint8_t>(nt[3]);
	ca.ntail_n = (int32_t)std::min<int64_t>(CAP_TAIL, (int64_t)G.cap_tail_n + d.n);
	k_cap_mark<<<(unsigned)std::min<int64_t>(ntiles, 1024), BLOCK, 0, c->st>>>(ca);
	k_cap_sweep<<<1, WAVE, 0, c->st>>>(ca);
	k_cap_tail<<<grid_for(ca.ntail_n, BLOCK), BLOCK, 0, c->st>>>(ca);
	HIPCHECK(c, hipGetLastError());
	G.cap_tail_n = ca.ntail_n; G.cap_tail_cur ^= 1;
	return SSV_OK;
}

int ssv_getsv_scan(ssv_ctx *c, const ssv_batch_t *b)
{
	if (!c || !b) return SSV_E_ARG;
	ssv_getsv_state &G = *c->getsv;
	if (!G.active) { c->err = "ssv_getsv_scan before ssv_getsv_begin"; return SSV_E_STATE; }
	HIPCHECK(c, hipSetDevice(c->device));
	if (b->n == 0) return SSV_OK;
	DevBatch d;
	CHECK(stage_batch(c, b, d));
	if (!d.cigar) { c->err = "batch without cigar"; return SSV_E_ARG; }
	int32_t span = d.max_ref_span;
	if (span <= 0) { // unknown: measure it
		HIPCHECK(c, hipMemsetAsync(G.span.p, 0, 16, c->st));
		k_max_span<<<grid_for(d.n, BLOCK), BLOCK, 0, c->st>>>(d, P<int>(G.span));
		CHECK(ensure_host(c, c->h_totals, 64));
		HIPCHECK(c, hipMemcpyAsync(c->h_totals.p, G.span.p, 4, hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
		span = std::max(1, *P<int>(c->h_totals));
	}
	if (span > G.map_span) CHECK(gs_build_tilemap(c, span));
	GetsvArgs a;
	CHECK(fill_runs(c, b, a.runs));
	static const bool verify_runs = getenv("SSV_VERIFY_RUNS") && atoi(getenv("SSV_VERIFY_RUNS")) != 0;
	if (verify_runs && a.runs.n > 0) { // the run list against the column it stands for (the scan below never reads that column where a run covers a tile)
		CHECK(ensure(c, c->counters, sizeof(ClipCounters)));
		CHECK(ensure_host(c, c->h_counters, sizeof(ClipCounters)));
		HIPCHECK(c, hipMemsetAsync(c->counters.p, 0, sizeof(ClipCounters), c->st));
		k_verify_runs<<<(unsigned)std::min<int64_t>(256 * 8, (d.n + BLOCK * 4 - 1) / (BLOCK * 4)), BLOCK, 0, c->st>>>(d.tid, d.n, a.runs, &P<ClipCounters>(c->counters)->n_cand);
		HIPCHECK(c, hipGetLastError());
		HIPCHECK(c, hipMemcpyAsync(c->h_counters.p, c->counters.p, sizeof(ClipCounters), hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
		const unsigned long long badrec = P<ClipCounters>(c->h_counters)->n_cand;
		if (badrec) { c->err = "tid_runs disagree with the tid column at record " + std::to_string(badrec - 1) + " (SSV_VERIFY_RUNS)"; return SSV_E_ARG; }
	}
	a.b = d; a.tilemap = P<uint8_t>(G.tilemap); a.tile_win = P<uint32_t>(G.tile_win); a.tile_junc = P<uint32_t>(G.tile_junc); a.ctg_tile_off = P<int64_t>(G.ctgoff); a.n_targets = G.p.n_targets;
	a.junc = P<DevJunction>(G.djunc); a.n_junc = (int64_t)G.junc.size(); a.junc_wmax = G.wmax;
	a.mean = G.p.mean; a.sd = G.p.sd; a.times = G.p.times; a.disc_min_mapq = G.p.disc_min_mapq;
	a.min_ins = std::max(0, a.mean - a.sd * a.times); a.max_ins = a.mean + a.sd * a.times; // getsv.cpp:1032-1034
	a.counts = P<int32_t>(G.counts);
	a.win_tid = P<int32_t>(G.wtid); a.win_beg = P<int32_t>(G.wbeg); a.win_end = P<int32_t>(G.wend); a.win_off = P<int64_t>(G.woff);
	a.n_win = (int64_t)G.win.size(); a.depth_min_mapq = G.p.depth_min_mapq; a.diff = P<int32_t>(G.diff);
	a.cap_flag = nullptr; a.cap_span = G.map_span;
	HIPCHECK(c, hipMemsetAsync(G.cap_flags.p, 0, 16, c->st)); // ([0], [1]: the read cap's flags, [2]: the length of the dense tiles' list)
	if (a.n_win > 0) a.cap_flag = P<int>(G.cap_flags);
	const int64_t ntiles = (d.n + CS_TILE - 1) / CS_TILE;
	const unsigned grid = scan_blocks(ntiles, "SSV_GETSV_SCAN_BLOCKS", 256 * 4);
	CHECK(ensure(c, c->tile_cnt, ntiles * 4));
	CHECK(ensure(c, c->tile_off, ntiles * 4));
	CHECK(ensure(c, c->counters, sizeof(ClipCounters)));
	CHECK(ensure_host(c, c->h_counters, sizeof(ClipCounters)));
	if (c->stage_cap == 0) c->stage_cap = std::max<int64_t>(1 << 16, d.n / 8);
	ClipCounters *hc = P<ClipCounters>(c->h_counters);
	ClipCounters *dc = P<ClipCounters>(c->counters);
	GetsvStage g;
	for (int attempt = 0;; ++attempt) {
		const int64_t block_cap = (c->stage_cap + grid - 1) / grid;
		CHECK(ensure(c, c->stage, (size_t)block_cap * grid * 4));
		HIPCHECK(c, hipMemsetAsync(c->counters.p, 0, sizeof(ClipCounters), c->st));
		g.tile_cnt = P<uint32_t>(c->tile_cnt); g.tile_off = P<uint32_t>(c->tile_off); g.stage = P<uint32_t>(c->stage); g.block_cap = block_cap;
		g.overflow = &dc->overflow; g.ntiles = ntiles;
		g.dense_list = nullptr; g.dense_n = nullptr; g.n_cand = &dc->n_cand;
		{
			ProfScope ps(c, P_GETSV_SCAN, d.n);
			if (a.runs.n > 0 && d.n >= CS_TILE) k_getsv_scan_runs<<<grid, BLOCK, 0, c->st>>>(a, g); // (the tid column as runs: never read)
			else k_getsv_scan<<<grid, BLOCK, 0, c->st>>>(a, g);
		}
		HIPCHECK(c, hipGetLastError());
		HIPCHECK(c, hipMemcpyAsync(hc, c->counters.p, sizeof(ClipCounters), hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
		if (!hc->overflow) break;
		if (attempt > 6) { c->err = "getsv staging overflow"; return SSV_E_HIP; }
		c->stage_cap *= 4; // a workgroup's private region was too small for the records near its windows
	}
	{
		ProfScope ps(c, P_GETSV_CAND, d.n);
		// tiles that are dense with candidates are listed and left to the second kernel; its grid: the scan's count bounds the list's length
		const int64_t dense_max = std::min<int64_t>(ntiles, (int64_t)(hc->n_cand / GC_DENSE_MIN));
		if (dense_max > 0) {
			CHECK(ensure(c, G.dense_list, (size_t)dense_max * sizeof(DenseTile)));
			g.dense_list = P<DenseTile>(G.dense_list); g.dense_n = P<int>(G.cap_flags) + 2; // (zeroed with the cap flags above)
			k_dense_tiles<<<grid_for(ntiles, BLOCK), BLOCK, 0, c->st>>>(a, g);
		}
		k_getsv_cand<<<grid_for(ntiles, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(a, g);
		if (g.dense_list) k_getsv_cand_dense<<<(unsigned)dense_max, BLOCK, 0, c->st>>>(a, g);
	}
	HIPCHECK(c, hipGetLastError());
	if (a.n_win > 0) CHECK(cap_launches(c, a, d, ntiles, 0));
	return SSV_OK;
}

int ssv_getsv_prime(ssv_ctx *c, const ssv_batch_t *b, int32_t *sufficient)
{
	if (!c || !b || !sufficient) return SSV_E_ARG;
	ssv_getsv_state &G = *c->getsv;
	if (!G.active) { c->err = "ssv_getsv_prime before ssv_getsv_begin"; return SSV_E_STATE; }
	if (G.cap_tail_n != 0) { c->err = "ssv_getsv_prime after records were scanned"; return SSV_E_STATE; }
	HIPCHECK(c, hipSetDevice(c->device));
	*sufficient = 1;
	if (b->n == 0 || G.win.empty()) return SSV_OK; // no depth pass: nothing to rebuild
	DevBatch d;
	CHECK(stage_batch(c, b, d));
	int32_t span = d.max_ref_span;
	if (span <= 0) {
		HIPCHECK(c, hipMemsetAsync(G.span.p, 0, 16, c->st));
		k_max_span<<<grid_for(d.n, BLOCK), BLOCK, 0, c->st>>>(d, P<int>(G.span));
		CHECK(ensure_host(c, c->h_totals, 128));
		HIPCHECK(c, hipMemcpyAsync(c->h_totals.p, G.span.p, 4, hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
		span = std::max(1, *P<int>(c->h_totals));
	}
	if (span > G.map_span) CHECK(gs_build_tilemap(c, span));
	GetsvArgs a;
	memset(&a, 0, sizeof(a));
	a.b = d; a.depth_min_mapq = G.p.depth_min_mapq; a.n_targets = G.p.n_targets; a.cap_span = G.map_span;
	a.tilemap = P<uint8_t>(G.tilemap); a.tile_win = P<uint32_t>(G.tile_win); a.ctg_tile_off = P<int64_t>(G.ctgoff);
	a.win_tid = P<int32_t>(G.wtid); a.win_beg = P<int32_t>(G.wbeg); a.win_end = P<int32_t>(G.wend); a.win_off = P<int64_t>(G.woff);
	a.n_win = (int64_t)G.win.size(); a.diff = P<int32_t>(G.diff);
	// every tile is looked at (the streaming pass that usually raises this flag does not run over a replayed batch)
	int one[4] = {1, 0, 0, 0};
	HIPCHECK(c, hipMemcpyAsync(G.cap_flags.p, one, 16, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st)); // (`one` lives on this stack)
	const int64_t ntiles = (d.n + CS_TILE - 1) / CS_TILE;
	CHECK(cap_launches(c, a, d, ntiles, 1));
	// The replay leaves the right state if it started from one: a sweep that begins >= 7,999 records before the first "deep" record does
	// (getsv_kernels.h).  A record can be judged from index 7,998 of the batch on; so the records [7998, 15997) - inside tiles 1..3 - must not
	// be deep.  A batch that starts at the file's first record is exact anyway: the caller knows that case and ignores the answer.
	CHECK(ensure_host(c, c->h_totals, 128));
	const int64_t nt = std::min<int64_t>(ntiles, 4);
	HIPCHECK(c, hipMemcpyAsync(c->h_totals.p, G.cap_deep.p, (size_t)nt, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	for (int64_t t = 1; t < nt; ++t) if (P<uint8_t>(c->h_totals)[t]) *sufficient = 0;
	if (d.n < 4 * CS_TILE) *sufficient = 0; // too short to tell: the records [7998, 15997) must all be there (a partly filled fourth tile does not show them)
	return SSV_OK;
}

int ssv_getsv_finish(ssv_ctx *c, int32_t *counts, const ssv_interval *ranges, int64_t n_ranges, uint64_t *range_sum,
                     const ssv_interval *points, int64_t n_points, int32_t *point_depth, int32_t *max_depth)
{
	if (!c || n_ranges < 0 || n_points < 0 || (n_ranges && (!ranges || !range_sum)) || (n_points && (!points || !point_depth))) return SSV_E_ARG;
	ssv_getsv_state &G = *c->getsv;
	if (!G.active) { c->err = "ssv_getsv_finish before ssv_getsv_begin"; return SSV_E_STATE; }
	HIPCHECK(c, hipSetDevice(c->device));
	G.active = false;
	const int64_t nw = (int64_t)G.win.size(), nj = (int64_t)G.junc.size();
	ProfScope ps(c, P_DEPTH_FINISH, nw);
	if (nw) k_depth_prefix<<<grid_for(nw, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(P<int64_t>(G.woff), nw, P<int32_t>(G.diff), P<int32_t>(G.maxdepth));
	// queries up, answers down: one pinned buffer each way, one synchronisation
	//   up:   [range tid | range beg | range end | point tid | point beg]        (int32 each)
	//   down: [range sums u64 | point depths i32 | counts i32 | max depth i32]
	const size_t up_bytes = ((size_t)n_ranges * 3 + (size_t)n_points * 2) * 4;
	const size_t o_pd = (size_t)n_ranges * 8, o_cnt = o_pd + (size_t)n_points * 4, o_max = o_cnt + (size_t)nj * 4, down_bytes = o_max + 4;
	CHECK(ensure_host(c, G.h_q, up_bytes + down_bytes + 64));
	CHECK(ensure(c, G.q_tid, up_bytes + 16)); CHECK(ensure(c, G.q_out64, down_bytes + 16));
	int32_t *up = P<int32_t>(G.h_q);
	uint8_t *down = P<uint8_t>(G.h_q) + ((up_bytes + 15) & ~(size_t)15);
	int32_t *rt = up, *rb = rt + n_ranges, *re = rb + n_ranges, *pt = re + n_ranges, *pb = pt + n_points;
	for (int64_t k = 0; k < n_ranges; ++k) { rt[k] = ranges[k].tid; rb[k] = ranges[k].beg; re[k] = ranges[k].end; }
	for (int64_t k = 0; k < n_points; ++k) { pt[k] = points[k].tid; pb[k] = points[k].beg; }
	int32_t *d_up = P<int32_t>(G.q_tid);
	uint8_t *d_down = P<uint8_t>(G.q_out64);
	if (up_bytes) HIPCHECK(c, hipMemcpyAsync(d_up, up, up_bytes, hipMemcpyHostToDevice, c->st));
	if (n_ranges) k_range_sum<<<grid_for(n_ranges, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(P<int32_t>(G.wtid), P<int32_t>(G.wbeg), P<int32_t>(G.wend), P<int64_t>(G.woff), nw,
	                                                                                  P<int32_t>(G.diff), d_up, d_up + n_ranges, d_up + 2 * n_ranges, n_ranges,
	                                                                                  reinterpret_cast<unsigned long long *>(d_down));
	if (n_points) k_point_depth<<<grid_for(n_points, BLOCK), BLOCK, 0, c->st>>>(P<int32_t>(G.wtid), P<int32_t>(G.wbeg), P<int32_t>(G.wend), P<int64_t>(G.woff), nw,
	                                                                          P<int32_t>(G.diff), d_up + 3 * n_ranges, d_up + 3 * n_ranges + n_points, n_points,
	                                                                          reinterpret_cast<int32_t *>(d_down + o_pd));
	if (nj) HIPCHECK(c, hipMemcpyAsync(d_down + o_cnt, G.counts.p, (size_t)nj * 4, hipMemcpyDeviceToDevice, c->st));
	HIPCHECK(c, hipMemcpyAsync(d_down + o_max, G.maxdepth.p, 4, hipMemcpyDeviceToDevice, c->st));
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipMemcpyAsync(down, d_down, down_bytes, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	if (n_ranges) memcpy(range_sum, down, (size_t)n_ranges * 8);
	if (n_points) memcpy(point_depth, down + o_pd, (size_t)n_points * 4);
	if (counts && nj) memcpy(counts, down + o_cnt, (size_t)nj * 4);
	if (max_depth) memcpy(max_depth, down + o_max, 4);
	return SSV_OK;
}
