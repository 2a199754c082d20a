// isize_api.inc - C ABI of the insert-size statistics (included by seeksv_hip.hip; kernels in getsv_kernels.h)

struct ssv_isize_state {
	bool active = false, undecided = false;
	int min_mapq = 0;
	int64_t max = 0, count = 0;
	DBuf vals, acc, tmp;
};

int ssv_isize_begin(ssv_ctx *c, int32_t min_mapq, int64_t max_pairs)
{
	if (!c) return SSV_E_ARG;
	ssv_isize_state &Z = *c->isz;
	HIPCHECK(c, hipSetDevice(c->device));
	c->pf.clear();
	// cluster.cpp:68 ends the pass when the count EQUALS read_pair_used, after every record that is not skipped: a negative value is never
	// met (no cap), and 0 only by the first such record, when that one does not qualify (ssv_isize_accumulate decides it there)
	Z.active = true; Z.min_mapq = min_mapq; Z.max = max_pairs < 0 ? INT64_MAX : max_pairs; Z.count = 0; Z.undecided = max_pairs == 0;
	return SSV_OK;
}

int ssv_isize_accumulate(ssv_ctx *c, const ssv_batch_t *b, int32_t *done)
{
	if (!c || !b) return SSV_E_ARG;
	ssv_isize_state &Z = *c->isz;
	if (!Z.active) { c->err = "ssv_isize_accumulate before ssv_isize_begin"; return SSV_E_STATE; }
	HIPCHECK(c, hipSetDevice(c->device));
	if ((Z.count >= Z.max && !Z.undecided) || b->n == 0) { if (done) *done = Z.count >= Z.max && !Z.undecided; return SSV_OK; }
	DevBatch d;
	CHECK(stage_batch(c, b, d));
	if (Z.undecided) {
		// read_pair_used == 0: the first record that reaches the comparison of cluster.cpp:68 ends the pass with no pair when it does not
		// qualify; when it does, the count is 1 there and never 0 again: every qualifying record of the file is taken
		CHECK(ensure(c, c->totals, 64)); CHECK(ensure_host(c, c->h_totals, 64));
		HIPCHECK(c, hipMemsetAsync(c->totals.p, 0xff, 8, c->st));
		k_isize_first_compared<<<grid_for(d.n, BLOCK), BLOCK, 0, c->st>>>(d, Z.min_mapq, P<unsigned long long>(c->totals));
		HIPCHECK(c, hipGetLastError());
		HIPCHECK(c, hipMemcpyAsync(c->h_totals.p, c->totals.p, 8, hipMemcpyDeviceToHost, c->st));
		HIPCHECK(c, hipStreamSynchronize(c->st));
		const unsigned long long first = *P<unsigned long long>(c->h_totals);
		if (first == ~0ull) { if (done) *done = 0; return SSV_OK; } // every record skipped: the next batch decides
		Z.undecided = false;
		if (!(first & 1)) { if (done) *done = 1; return SSV_OK; }  // (Z.count == Z.max == 0 from here on)
		Z.max = INT64_MAX;
	}
	ProfScope ps(c, P_ISIZE, d.n);
	const int64_t ntiles = (d.n + ISZ_TILE - 1) / ISZ_TILE;
	CHECK(ensure(c, c->tile_cnt, ntiles * 4)); CHECK(ensure(c, c->tile_base, ntiles * 4));
	CHECK(ensure(c, c->scan_scratch, scan_scratch_elems(ntiles) * 4));
	CHECK(ensure(c, c->totals, 64)); CHECK(ensure_host(c, c->h_totals, 64));
	const int64_t need = std::min<int64_t>(Z.max, Z.count + d.n);
	CHECK(ensure(c, Z.vals, (size_t)need * 4 + 16, true, (size_t)Z.count * 4));
	CHECK(ensure(c, Z.tmp, (size_t)d.n * 4 + 16));
	k_isize_count<<<(unsigned)ntiles, BLOCK, 0, c->st>>>(d, Z.min_mapq, P<int32_t>(Z.tmp), P<uint32_t>(c->tile_cnt));
	exclusive_scan<uint32_t, uint32_t>(c->st, P<uint32_t>(c->tile_cnt), P<uint32_t>(c->tile_base), ntiles, 0u, P<uint32_t>(c->scan_scratch), P<uint32_t>(c->totals));
	k_isize_collect<<<(unsigned)ntiles, BLOCK, 0, c->st>>>(P<int32_t>(Z.tmp), d.n, P<uint32_t>(c->tile_base), Z.count, Z.max, P<int32_t>(Z.vals));
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipMemcpyAsync(c->h_totals.p, c->totals.p, 4, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	Z.count = std::min<int64_t>(Z.max, Z.count + *P<uint32_t>(c->h_totals));
	if (done) *done = Z.count >= Z.max;
	return SSV_OK;
}

int ssv_isize_finish(ssv_ctx *c, int64_t *n_pairs, int32_t *mean, int32_t *sd)
{
	if (!c || !n_pairs || !mean || !sd) return SSV_E_ARG;
	ssv_isize_state &Z = *c->isz;
	if (!Z.active) { c->err = "ssv_isize_finish before ssv_isize_begin"; return SSV_E_STATE; }
	HIPCHECK(c, hipSetDevice(c->device));
	Z.active = false;
	const int64_t n = Z.count;
	*n_pairs = n;
	if (n == 0) { HIPCHECK(c, hipStreamSynchronize(c->st)); return SSV_OK; } // cluster.cpp:71: mean / sd untouched
	ProfScope ps(c, P_ISIZE, 0);
	CHECK(ensure(c, Z.acc, 16)); CHECK(ensure_host(c, c->h_totals, 64));
	long long *acc = P<long long>(Z.acc);
	unsigned grid = (unsigned)std::min<int64_t>(1024, (n + BLOCK - 1) / BLOCK);
	HIPCHECK(c, hipMemsetAsync(acc, 0, 16, c->st));
	k_isize_reduce<<<grid, BLOCK, 0, c->st>>>(P<int32_t>(Z.vals), n, 0, nullptr, acc);
	k_isize_reduce<<<grid, BLOCK, 0, c->st>>>(P<int32_t>(Z.vals), n, 1, acc, acc + 1);
	HIPCHECK(c, hipMemcpyAsync(c->h_totals.p, acc, 16, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	const unsigned long total = (unsigned long)P<long long>(c->h_totals)[0];
	const int m = (int)(total / (unsigned long)n); // cluster.cpp:72
	// cluster.cpp:73-80 adds the (int) squares one by one into a double; the exact integer sum is the same value as long as it
	// stays below 2^53 (5e6 pairs * 2^31 is ~2^53.2: only reachable with absurd insert sizes)
	const double dsum = (double)P<long long>(c->h_totals)[1];
	*mean = m;
	*sd = (int)std::sqrt(dsum / (double)n);
	return SSV_OK;
}
