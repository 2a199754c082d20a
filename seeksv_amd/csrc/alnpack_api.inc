// alnpack_api.inc - ssv_aln_pack: a decoded batch of clipped-sequence re-alignments -> the host join's columns (included by seeksv_hip.hip inside extern "C";
// kernels in alnpack_kernels.h).  stage the batch -> k_aln_cols, k_aln_name_len -> scan -> (sync: bytes of the names) -> k_aln_pack -> one copy per column
// into page-locked memory -> (sync).

struct ssv_alnpack_state {
	DBuf flag, mapq, cigar_off, nbytes, name_off, blob, hash, hnames, hoff, small;
	HBuf h_tid, h_pos, h_flag, h_n_cigar, h_mapq, h_cigar_off, h_cigar, h_name_off, h_names, h_hash, h_small;
};

int ssv_aln_pack(ssv_ctx *c, const ssv_batch_t *b, const ssv_names_t *nm, ssv_aln_cols *out)
{
	if (!c) return SSV_E_ARG;
	if (!b || !out) { c->err = "ssv_aln_pack: no batch or no result"; return SSV_E_ARG; }
	CHECK(check_names(c, nm, b->n, "ssv_aln_pack"));
	if (b->n_cigar_total < 0 || b->n_cigar_total >= (1ll << 32)) { c->err = "ssv_aln_pack: bad n_cigar_total"; return SSV_E_ARG; }
	HIPCHECK(c, hipSetDevice(c->device));
	DevBatch d;
	CHECK(stage_batch(c, b, d));
	if (!c->ap) c->ap.reset(new ssv_alnpack_state());
	ssv_alnpack_state &A = *c->ap;
	hipStream_t st = c->st;
	const int64_t n = d.n;
	const size_t N = (size_t)n, n_ops = (size_t)b->n_cigar_total;
	memset(out, 0, sizeof(*out));
	CHECK(ensure_host(c, A.h_tid, N * 4 + 16)); CHECK(ensure_host(c, A.h_pos, N * 4 + 16)); CHECK(ensure_host(c, A.h_flag, N * 2 + 16)); CHECK(ensure_host(c, A.h_n_cigar, N * 2 + 16));
	CHECK(ensure_host(c, A.h_mapq, N + 16)); CHECK(ensure_host(c, A.h_cigar_off, N * 4 + 16)); CHECK(ensure_host(c, A.h_cigar, n_ops * 4 + 16)); CHECK(ensure_host(c, A.h_name_off, N * 8 + 16));
	CHECK(ensure_host(c, A.h_hash, N * 8 + 16)); CHECK(ensure_host(c, A.h_names, 16)); CHECK(ensure_host(c, A.h_small, 64));
	uint64_t name_bytes = 0;
	if (n > 0) {
		DevNames names;
		CHECK(stage_names(c, nm, n, A.hnames, A.hoff, names));
		CHECK(ensure(c, A.flag, N * 2 + 16)); CHECK(ensure(c, A.mapq, N + 16)); CHECK(ensure(c, A.cigar_off, N * 4 + 16)); CHECK(ensure(c, A.nbytes, N * 4 + 16));
		CHECK(ensure(c, A.name_off, N * 8 + 16)); CHECK(ensure(c, A.hash, N * 8 + 16)); CHECK(ensure(c, A.small, 64));
		CHECK(ensure(c, c->scan_scratch64, (size_t)scan_scratch_elems(n) * 8 + 64));
		k_aln_cols<<<grid_for(n, BLOCK), BLOCK, 0, st>>>(d.rec, n, P<uint16_t>(A.flag), P<uint8_t>(A.mapq), P<uint32_t>(A.cigar_off));
		k_aln_name_len<<<grid_for(n, BLOCK), BLOCK, 0, st>>>(names, n, P<uint32_t>(A.nbytes));
		HIPCHECK(c, hipGetLastError());
		exclusive_scan<uint32_t, uint64_t>(st, P<uint32_t>(A.nbytes), P<uint64_t>(A.name_off), n, 0ull, P<uint64_t>(c->scan_scratch64), P<uint64_t>(A.small));
		HIPCHECK(c, hipMemcpyAsync(A.h_small.p, A.small.p, 8, hipMemcpyDeviceToHost, st));
		HIPCHECK(c, hipStreamSynchronize(st)); // (the blob and its host copy are sized by the names' bytes; a host batch's names have been read)
		name_bytes = *P<uint64_t>(A.h_small);
		CHECK(ensure(c, A.blob, (size_t)name_bytes + 16)); CHECK(ensure_host(c, A.h_names, (size_t)name_bytes + 16));
		k_aln_pack<<<grid_for(n * 4, BLOCK), BLOCK, 0, st>>>(names, n, P<uint32_t>(A.nbytes), P<uint64_t>(A.name_off), P<char>(A.blob), P<uint64_t>(A.hash));
		HIPCHECK(c, hipGetLastError());
		struct { void *dst; const void *src; size_t bytes; } f[10] = {
			{A.h_tid.p, d.tid, N * 4}, {A.h_pos.p, d.pos, N * 4}, {A.h_n_cigar.p, d.n_cigar, N * 2}, {A.h_flag.p, A.flag.p, N * 2}, {A.h_mapq.p, A.mapq.p, N},
			{A.h_cigar_off.p, A.cigar_off.p, N * 4}, {A.h_cigar.p, d.cigar, n_ops * 4}, {A.h_name_off.p, A.name_off.p, N * 8}, {A.h_names.p, A.blob.p, (size_t)name_bytes},
			{A.h_hash.p, A.hash.p, N * 8}};
		for (const auto &x : f) if (x.bytes) HIPCHECK(c, hipMemcpyAsync(x.dst, x.src, x.bytes, hipMemcpyDeviceToHost, st));
		HIPCHECK(c, hipStreamSynchronize(st));
	}
	out->n = n; out->n_cigar_total = n > 0 ? (int64_t)n_ops : 0; out->name_bytes = (int64_t)name_bytes;
	out->tid = P<int32_t>(A.h_tid); out->pos = P<int32_t>(A.h_pos); out->flag = P<uint16_t>(A.h_flag); out->n_cigar = P<uint16_t>(A.h_n_cigar); out->mapq = P<uint8_t>(A.h_mapq);
	out->cigar_off = P<uint32_t>(A.h_cigar_off); out->cigar = P<uint32_t>(A.h_cigar); out->name_off = P<uint64_t>(A.h_name_off); out->names = P<char>(A.h_names);
	out->name_hash = P<uint64_t>(A.h_hash);
	return SSV_OK;
}
