// realign_api.inc - C ABI of the clipped-sequence re-aligner (included by seeksv_hip.hip; kernels in realign_kernels.h)

struct ssv_realign_state {
	DBuf ref, ctg, table, seqs, offs, hits, dropped;
	const uint64_t *ref_p = nullptr; // device pointer used by the kernels (own copy or the caller's resident array)
	int64_t n_bases = 0;
	int32_t n_ctg = 0;
	uint64_t mask = 0;
	bool ready = false;
};

int ssv_realign_index(ssv_ctx *c, const uint64_t *ref2bit, int32_t mem, int64_t n_bases, const int64_t *target_off, int32_t n_targets, int64_t *n_dropped)
{
	if (!c || !ref2bit || !target_off || n_targets <= 0 || n_bases <= 0 || target_off[0] != 0 || target_off[n_targets] != n_bases) return SSV_E_ARG;
	if (n_bases / RA_SAMPLE >= (int64_t)0xfffffffe) { c->err = "reference too long for the re-aligner's 32-bit slots"; return SSV_E_RANGE; }
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->ra) c->ra.reset(new ssv_realign_state());
	ssv_realign_state &R = *c->ra;
	R.ready = false;
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
	const int64_t samples = (n_bases + RA_SAMPLE - 1) / RA_SAMPLE;
	uint64_t slots = 1024;
	while (slots < (uint64_t)samples * 2) slots <<= 1;
	CHECK(ensure(c, R.table, slots * 4));
	HIPCHECK(c, hipMemsetAsync(R.table.p, 0, slots * 4, c->st));
	CHECK(ensure(c, R.dropped, 8));
	HIPCHECK(c, hipMemsetAsync(R.dropped.p, 0, 8, c->st));
	R.n_bases = n_bases; R.n_ctg = n_targets; R.mask = slots - 1;
	RaIndex ix;
	ix.ref = R.ref_p; ix.n_bases = n_bases; ix.ctg_off = P<int64_t>(R.ctg); ix.n_ctg = n_targets; ix.table = P<uint32_t>(R.table); ix.mask = R.mask;
	{
		ProfScope ps(c, P_REALIGN_INDEX, samples);
		k_ra_build<<<grid_for(samples, BLOCK), BLOCK, 0, c->st>>>(ix, reinterpret_cast<unsigned long long *>(R.dropped.p));
	}
	HIPCHECK(c, hipGetLastError());
	unsigned long long d = 0;
	HIPCHECK(c, hipMemcpyAsync(&d, R.dropped.p, 8, hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	if (n_dropped) *n_dropped = (int64_t)d;
	R.ready = true;
	return SSV_OK;
}

int ssv_realign_query(ssv_ctx *c, const char *seqs, const uint64_t *seq_off, int64_t n, ssv_realign_hit *hits)
{
	if (!c || n < 0 || (n > 0 && (!seqs || !seq_off || !hits))) return SSV_E_ARG;
	if (!c->ra || !c->ra->ready) { if (c) c->err = "ssv_realign_query before ssv_realign_index"; return SSV_E_STATE; }
	if (n == 0) return SSV_OK;
	static_assert(sizeof(RaHit) == sizeof(ssv_realign_hit), "hit layout");
	HIPCHECK(c, hipSetDevice(c->device));
	ssv_realign_state &R = *c->ra;
	const uint64_t bytes = seq_off[n];
	CHECK(ensure(c, R.seqs, bytes + 16)); CHECK(ensure(c, R.offs, (size_t)(n + 1) * 8)); CHECK(ensure(c, R.hits, (size_t)n * sizeof(RaHit)));
	HIPCHECK(c, hipMemcpyAsync(R.seqs.p, seqs, bytes, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemcpyAsync(R.offs.p, seq_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->st));
	RaQueryArgs a;
	a.ix.ref = R.ref_p; a.ix.n_bases = R.n_bases; a.ix.ctg_off = P<int64_t>(R.ctg); a.ix.n_ctg = R.n_ctg; a.ix.table = P<uint32_t>(R.table); a.ix.mask = R.mask;
	a.seqs = P<char>(R.seqs); a.seq_off = P<uint64_t>(R.offs); a.n = n; a.hits = P<RaHit>(R.hits);
	{
		ProfScope ps(c, P_REALIGN_QUERY, n);
		k_ra_query<<<grid_for(n, WAVES_PER_BLOCK), BLOCK, 0, c->st>>>(a);
	}
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipMemcpyAsync(hits, R.hits.p, (size_t)n * sizeof(RaHit), hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
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
