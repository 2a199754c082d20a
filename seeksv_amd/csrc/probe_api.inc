// probe_api.inc - C ABI of the somatic look-ups (`seeksv somatic -K`; included by seeksv_hip.hip behind clip_api.inc; kernel in probe_kernels.h).
// ssv_clip_probe_set leaves probes, their text and zeroed hits in device memory; while they are set, ssv_clip_cluster[_async] runs k_somatic_probe
// against the pass's table (probe_after_pack, called between the pack kernels and the table's copy out), and ssv_clip_probe_get hands the hits back.

struct ssv_probe_state {
	DBuf probes, text, thr, hits;
	int64_t n = 0;          // 0: no probes set
	int64_t passes = 0;     // passes clustered since the set
	uint32_t min_clipped_len = 0;
};

// thr[n] = the fewest matches m out of n with (double)m / n >= rate, by that very division (the reference's, clip_reads.cpp:194-217); n == 0 and a NaN rate: never
static void probe_thresholds(double rate, std::vector<uint32_t> &thr)
{
	thr[0] = 0xffffffffu;
	for (size_t n = 1; n < thr.size(); ++n) {
		uint32_t m = 0xffffffffu;
		if (rate == rate) {
			const double g = ceil(rate * (double)n);
			int64_t k = g < 0.0 ? 0 : g > (double)(n + 1) ? (int64_t)n + 1 : (int64_t)g;
			while (k > 0 && (double)(k - 1) / (double)n >= rate) --k;
			while (k <= (int64_t)n && !((double)k / (double)n >= rate)) ++k;
			m = (uint32_t)k; // (n + 1: more than there are characters)
		}
		thr[n] = m;
	}
}

int ssv_clip_probe_set(ssv_ctx *c, const ssv_clip_probe *probes, int64_t n, const char *text, uint64_t text_bytes, double match_rate, uint32_t min_clipped_len)
{
	if (!c) return SSV_E_ARG;
	if (n < 0 || (n > 0 && (!probes || (!text && text_bytes)))) { c->err = "ssv_clip_probe_set: NULL probes or text with n > 0"; return SSV_E_ARG; }
	uint64_t longest = 0;
	for (int64_t i = 0; i < n; ++i) {
		const ssv_clip_probe &p = probes[i];
		if (p.side != '3' && p.side != '5') { c->err = "ssv_clip_probe_set: probe " + std::to_string(i) + ": side must be '3' or '5'"; return SSV_E_ARG; }
		if (p.mode > 2) { c->err = "ssv_clip_probe_set: probe " + std::to_string(i) + ": mode must be 0, 1 or 2"; return SSV_E_ARG; }
		if ((uint64_t)p.a_off + p.a_len > text_bytes || (uint64_t)p.b_off + p.b_len > text_bytes) { c->err = "ssv_clip_probe_set: probe " + std::to_string(i) + ": a string ends behind the text"; return SSV_E_ARG; }
		longest = std::max(longest, (uint64_t)p.a_len + p.b_len);
	}
	if (longest >= 0x7fffffffull) { c->err = "ssv_clip_probe_set: a probe's strings are 2 GB or more"; return SSV_E_ARG; }
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->probe) c->probe.reset(new ssv_probe_state());
	ssv_probe_state &S = *c->probe;
	HIPCHECK(c, hipStreamSynchronize(c->st)); // (a probe kernel of the set before may still read what is replaced below)
	S.n = 0; S.passes = 0;
	if (n == 0) return SSV_OK;
	std::vector<uint32_t> thr((size_t)longest + 1);
	probe_thresholds(match_rate, thr);
	CHECK(ensure(c, S.probes, (size_t)n * sizeof(ssv_clip_probe)));
	CHECK(ensure(c, S.text, (size_t)text_bytes + 16));
	CHECK(ensure(c, S.thr, thr.size() * 4));
	CHECK(ensure(c, S.hits, (size_t)n * sizeof(ssv_clip_probe_hit)));
	HIPCHECK(c, hipMemcpyAsync(S.probes.p, probes, (size_t)n * sizeof(ssv_clip_probe), hipMemcpyHostToDevice, c->st));
	if (text_bytes) HIPCHECK(c, hipMemcpyAsync(S.text.p, text, (size_t)text_bytes, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemcpyAsync(S.thr.p, thr.data(), thr.size() * 4, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemsetAsync(S.hits.p, 0, (size_t)n * sizeof(ssv_clip_probe_hit), c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st)); // (the caller's arrays, and `thr`, are its own again)
	S.n = n; S.min_clipped_len = min_clipped_len;
	return SSV_OK;
}

static bool probes_set(const ssv_ctx *c) { return c->probe && c->probe->n > 0; }

// behind the kernels that built T (cluster_pack has synchronised: T.n_clusters is known), in front of the table's copy out and of the next pass's use of the buffers; on the pass's stream
static int probe_after_pack(ssv_ctx *c, TableSet &T)
{
	ssv_probe_state &S = *c->probe;
	const int32_t pass = (int32_t)S.passes++;
	if (T.n_clusters == 0) return SSV_OK;
	ProfScope ps(c, P_SOMATIC_PROBE, S.n);
	ProbeArgs a;
	a.probes = P<ssv_clip_probe>(S.probes); a.n_probes = S.n; a.text = P<uint8_t>(S.text); a.thr = P<uint32_t>(S.thr); a.min_clipped_len = S.min_clipped_len; a.pass = pass;
	a.tid = P<int32_t>(T.o_tid); a.pos = P<int32_t>(T.o_pos); a.support = P<int32_t>(T.o_support); a.ll = P<int32_t>(T.o_ll); a.lr = P<int32_t>(T.o_lr);
	a.side = P<uint8_t>(T.o_side); a.str = P<uint8_t>(T.o_str); a.str_off = P<uint64_t>(T.o_stroff); a.n_clusters = T.n_clusters;
	a.hits = P<ssv_clip_probe_hit>(S.hits);
	for (int64_t q0 = 0; q0 < S.n; q0 += 1 << 30) { // (a grid dimension holds 2^31 - 1 workgroups)
		ProbeArgs part = a;
		part.probes += q0; part.hits += q0; part.n_probes = std::min<int64_t>(S.n - q0, 1 << 30);
		k_somatic_probe<<<(unsigned)part.n_probes, WAVE, 0, c->st>>>(part);
	}
	HIPCHECK(c, hipGetLastError());
	return SSV_OK;
}

int ssv_clip_probe_get(ssv_ctx *c, ssv_clip_probe_hit *hits, int64_t *passes)
{
	if (!c) return SSV_E_ARG;
	const int64_t n = c->probe ? c->probe->n : 0;
	if (n > 0 && !hits) { c->err = "ssv_clip_probe_get: NULL hits"; return SSV_E_ARG; }
	HIPCHECK(c, hipSetDevice(c->device));
	if (n > 0) HIPCHECK(c, hipMemcpyAsync(hits, c->probe->hits.p, (size_t)n * sizeof(ssv_clip_probe_hit), hipMemcpyDeviceToHost, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st));
	if (passes) *passes = c->probe ? c->probe->passes : 0;
	return SSV_OK;
}
