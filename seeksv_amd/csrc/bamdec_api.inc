// bamdec_api.inc - host side of the device BGZF/BAM decoder (included by seeksv_hip.hip inside extern "C").
// Per chunk: compressed bytes H2D -> k_bgzf_inflate -> k_find_records -> k_stitch_blocks -> (sync: record count) -> k_list_records ->
// k_record_fields -> scans -> k_record_cigars -> k_record_seqs / k_raw_copy / k_tid_* -> (sync: totals) -> device batch + small host-side lists.

struct ssv_bamdec_state {
	int32_t n_targets = 0;
	uint64_t start = 0;        // position of the first record inside the next chunk's stream (header length at first, then 0)
	int32_t prev_tid = 0;      // contig of the last mapped-pair record so far (clip_reads.h:407: starts at 0)
	uint64_t carry = 0;        // bytes of the unfinished record carried over from the previous chunk
	std::vector<uint64_t> htokoff;
	uint64_t limit = UINT64_MAX; // ssv_bamdec_limit: where the next chunk's records end (inflated bytes into its blocks)
	bool verify_crc = false;      // ssv_bamdec_verify_crc
	bool any_order = false;       // ssv_bamdec_any_order: chunks with more contig changes than the list holds go through without the list
	DBuf crc_tab;
	uint64_t expect_inflated = 0; // ssv_bamdec_expect: the largest chunk that will come (buffers are sized for it by the first, smaller one)
	DBuf inf_scratch, inf_dbg, tokens, tok_off, n_tok, carrybuf, comp, blocks, u_off, stream, status, chain, count, base, rec_off, stitch, small;
	TidLists tl; // the contig changes, and the batch's tid column as runs (ssv_batch_t.tid_runs)
	DBuf tlen; bool have_tlen = false; // contig lengths (optional: ssv_bamdec_target_lens)
	DecodedColumns cols; // the batch handed out
	DBuf rel, stash, seq_list, raw_bytes, raw_off, raw;
	DBuf aux_off, aux_len; // ssv_bamdec_aux: where each record's optional fields lie (only when asked for)
	HBuf h_stage[3], h_small, h_raw[2], h_status; // h_raw: two in turn - a chunk's UNMAP|MUNMAP records stay valid while the next chunk is decoded (a thread beside the decoder pairs them up)
	int raw_flip = 0;
	// chunks announced ahead (ssv_bamdec_prefetch): their compressed bytes travel on the upload stream into one of two slots while the chunk before is inflated
	struct CompSlot {
		DBuf buf;
		const void *host = nullptr; // whose bytes the slot holds (or is receiving); nullptr = none
		size_t bytes = 0;
		hipEvent_t up = nullptr;    // the copy into the slot
		hsa_signal_t up_sig{};      // ... or its HSA signal when it went to a named SDMA engine (LinkCopy, seeksv_hip.hip)
		bool via_link = false;
		hipEvent_t done = nullptr;  // the last kernel that read the slot
		bool read = false;          // `done` has been recorded
	} slot[2];
	int next_slot = 0;
	hsa_signal_t own_sig{};        // a chunk that was not announced ahead: copied by its decode call, which waits for it
	std::vector<ssv::BgzfBlock> hblocks;
	std::vector<uint64_t> huoff;
	ssv_bamdec_info info{};
};

// before the context's buffers go (ssv_ctx_destroy): a copy still on its way into a slot lands, and the events and HSA signals are destroyed while c->link is valid
static void bamdec_release_handles(ssv_ctx *c)
{
	ssv_bamdec_state *d = c->bd.get();
	if (!d) return;
	for (auto &sl : d->slot) {
		if (sl.via_link && sl.host) link_wait(c, sl.up_sig); // (a copy still on its way into the slot)
		if (sl.up) (void)hipEventDestroy(sl.up); if (sl.done) (void)hipEventDestroy(sl.done);
		if (c->link.signal_destroy && sl.up_sig.handle) (void)c->link.signal_destroy(sl.up_sig);
	}
	if (c->link.signal_destroy && d->own_sig.handle) (void)c->link.signal_destroy(d->own_sig);
}

int ssv_bamdec_begin(ssv_ctx *c, int32_t n_targets, uint64_t first_record_offset)
{
	if (!c || n_targets < 0) return SSV_E_ARG;
	if (!c->bd) c->bd.reset(new ssv_bamdec_state());
	c->bd->have_tlen = false;
	c->bd->n_targets = n_targets; c->bd->start = first_record_offset; c->bd->prev_tid = 0; c->bd->carry = 0; c->bd->limit = UINT64_MAX; c->bd->expect_inflated = 0; c->bd->verify_crc = false;
	c->bd->any_order = false;
	for (auto &sl : c->bd->slot) sl.host = nullptr; // (a copy still on its way lands in a slot nobody asks for)
	memset(&c->bd->info, 0, sizeof(c->bd->info));
	return SSV_OK;
}

// optional, after ssv_bamdec_begin: the contigs' lengths (n_targets of them) sharpen the speculation of record starts - a position must lie inside its contig
int ssv_bamdec_target_lens(ssv_ctx *c, const int32_t *lens)
{
	if (!c || !c->bd || (!lens && c->bd->n_targets)) return SSV_E_ARG;
	ssv_bamdec_state &d = *c->bd;
	if (d.n_targets == 0) return SSV_OK;
	CHECK(ensure(c, d.tlen, (size_t)d.n_targets * 4 + 16));
	HIPCHECK(c, hipMemcpyAsync(d.tlen.p, lens, (size_t)d.n_targets * 4, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipStreamSynchronize(c->st)); // (the caller's array need not outlive the call)
	d.have_tlen = true;
	return SSV_OK;
}

// Optional, after ssv_bamdec_begin: chunks of up to `inflated_bytes` will follow.  A driver starts a file with a small chunk (the GPU gets to work
// while the rest is read); sized for that one, every buffer of the decoder would be freed and allocated again - each time behind a stream
// synchronisation - when the first full-size chunk arrives (0.2 s on a 2 GB chunk).  With the hint the first decode sizes them for the large one.
int ssv_bamdec_expect(ssv_ctx *c, uint64_t inflated_bytes)
{
	if (!c || !c->bd) return SSV_E_ARG;
	c->bd->expect_inflated = inflated_bytes;
	return SSV_OK;
}

// Optional, after ssv_bamdec_begin: a file in any record order (getsv -F: split alignments in read order).  A chunk with more than 65536 contig
// changes among its mapped-pair records is then decoded like any other; only its contig-change list (ssv_bamdec_info.n_tid_runs) is not handed out.
int ssv_bamdec_any_order(ssv_ctx *c, int on)
{
	if (!c || !c->bd) return SSV_E_ARG;
	c->bd->any_order = on != 0;
	return SSV_OK;
}

// Optional: check every inflated block's CRC32 against its BGZF trailer (one more pass over bytes that are in HBM anyway).  Off by default: libbam 0.1.16,
// the reference's reader, checks none, and a block whose deflate structure is valid but whose bytes are damaged decodes silently there too.
int ssv_bamdec_verify_crc(ssv_ctx *c, int on)
{
	if (!c || !c->bd) return SSV_E_ARG;
	c->bd->verify_crc = on != 0;
	return SSV_OK;
}

// a run that starts inside the file: the contig of the last mapped-pair record before it (the decoder's contig-change list continues from there)
int ssv_bamdec_prev_tid(ssv_ctx *c, int32_t tid)
{
	if (!c || !c->bd) return SSV_E_ARG;
	c->bd->prev_tid = tid;
	return SSV_OK;
}

// the records of the next chunk end `inflated_bytes` into its blocks (a run of records that ends inside the chunk's last block: ssvh_bam_raw_limit)
int ssv_bamdec_limit(ssv_ctx *c, uint64_t inflated_bytes)
{
	if (!c || !c->bd) return SSV_E_ARG;
	c->bd->limit = inflated_bytes;
	return SSV_OK;
}

int ssv_bamdec_staging(ssv_ctx *c, int which, size_t bytes, void **host_ptr)
{
	if (!c || !c->bd || !host_ptr || which < 0 || which > 2) return SSV_E_ARG;
	HIPCHECK(c, hipSetDevice(c->device)); // (a reader thread of its own may be the caller: the two buffers are independent of each other and of a decode in flight)
	CHECK(ensure_host(c, c->bd->h_stage[which], bytes + 64));
	*host_ptr = c->bd->h_stage[which].p;
	return SSV_OK;
}

int ssv_bamdec_prefetch(ssv_ctx *c, const void *comp, size_t comp_bytes)
{
	if (!c || !c->bd || !comp || !comp_bytes) return SSV_E_ARG;
	ssv_bamdec_state &d = *c->bd;
	for (auto &sl : d.slot) if (sl.host == comp) return SSV_OK; // announced already
	auto &sl = d.slot[d.next_slot];
	if (sl.host) return SSV_OK; // both slots hold chunks that have not been decoded yet: this one is copied by its decode call
	d.next_slot ^= 1;
	if (!sl.up) { HIPCHECK(c, hipEventCreateWithFlags(&sl.up, hipEventDisableTiming)); HIPCHECK(c, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming)); }
	if (sl.buf.cap < comp_bytes + 64 && sl.read) HIPCHECK(c, hipEventSynchronize(sl.done)); // (growing frees the old slot)
	CHECK(ensure(c, sl.buf, comp_bytes + 64));
	sl.via_link = false;
	if (c->link.ok && link_host_ok(comp) && (sl.up_sig.handle || c->link.signal_create(0, 0, nullptr, &sl.up_sig) == HSA_STATUS_SUCCESS)) {
		// on the host-to-device engine by name (LinkCopy): no stream orders it, so the slot's last reader is waited for here - its decode call returned long ago, behind its own synchronisations
		if (sl.read) HIPCHECK(c, hipEventSynchronize(sl.done));
		c->link.signal_store(sl.up_sig, 1);
		if (link_copy(c, sl.buf.p, comp, comp_bytes, false, sl.up_sig)) sl.via_link = true;
		else c->link.signal_store(sl.up_sig, 0);
	}
	if (!sl.via_link) {
		if (sl.read) HIPCHECK(c, hipStreamWaitEvent(c->st_h2d, sl.done, 0)); // the chunk that was in this slot may still be read by its inflate kernel
		HIPCHECK(c, hipMemcpyAsync(sl.buf.p, comp, comp_bytes, hipMemcpyHostToDevice, c->st_h2d));
		HIPCHECK(c, hipEventRecord(sl.up, c->st_h2d));
	}
	sl.host = comp; sl.bytes = comp_bytes; sl.read = false;
	return SSV_OK;
}

// give up the chunks that were announced and will not be decoded: returns when their copies have left the host memory
int ssv_bamdec_prefetch_drop(ssv_ctx *c)
{
	if (!c) return SSV_E_ARG;
	if (!c->bd) return SSV_OK;
	HIPCHECK(c, hipSetDevice(c->device));
	bool any = false;
	for (auto &sl : c->bd->slot) any = any || sl.host;
	if (any) HIPCHECK(c, hipStreamSynchronize(c->st_h2d));
	for (auto &sl : c->bd->slot) { if (sl.host && sl.via_link) link_wait(c, sl.up_sig); sl.host = nullptr; }
	return SSV_OK;
}

int ssv_bamdec_decode(ssv_ctx *c, const void *comp, size_t comp_bytes, const ssv_bgzf_block *blocks, int64_t n_blocks, int keep_all_seq, ssv_batch_t *out)
{
	if (!c || !c->bd || !out || n_blocks < 0 || (n_blocks && (!comp || !blocks))) return SSV_E_ARG;
	ssv_bamdec_state &d = *c->bd;
	hipStream_t st = c->st;
	memset(out, 0, sizeof(*out));
	out->mem = SSV_MEM_DEVICE;
	// ---- layout of the chunk's stream: [carry | block 0 | block 1 | ...] ----
	d.hblocks.resize((size_t)n_blocks); d.huoff.resize((size_t)n_blocks + 1);
	uint64_t total = d.carry;
	for (int64_t b = 0; b < n_blocks; ++b) {
		if (blocks[b].c_off + blocks[b].c_len + (d.verify_crc ? 8 : 0) > comp_bytes) { c->err = "BGZF block outside the chunk"; return SSV_E_ARG; } // (-C reads the trailer behind the payload: CRC32, ISIZE)
		if (blocks[b].u_len > 65536 || blocks[b].c_len > 65536 + 1024) { c->err = "BGZF block larger than the format allows (64 KB)"; return SSV_E_ARG; }
		d.hblocks[(size_t)b] = ssv::BgzfBlock{blocks[b].c_off, blocks[b].c_len, blocks[b].u_len};
		d.huoff[(size_t)b] = total;
		total += blocks[b].u_len;
	}
	d.huoff[(size_t)n_blocks] = total;
	// a run that ends inside this chunk: the stream is over there (a record boundary), whatever the blocks hold behind it
	const uint64_t stream_end = d.limit != UINT64_MAX && d.carry + d.limit < total ? d.carry + d.limit : total;
	d.limit = UINT64_MAX;
	if (total >= (1ull << 36)) { c->err = "chunk inflates to more than 64 GB"; return SSV_E_ARG; }
	// every buffer below is sized as if this chunk were as large as the largest one announced (ssv_bamdec_expect): in proportion
	const double up = total > d.carry && d.expect_inflated > total - d.carry ? std::min(64.0, (double)d.expect_inflated / (double)(total - d.carry)) : 1.0;
	if (total > d.carry) d.expect_inflated = 0; // the hint serves the FIRST decode behind it: a later, smaller chunk of another mix (a file's tail of unmapped reads) must not multiply its needs again
	auto ensure_up = [&](DBuf &buf, size_t bytes) { return ensure(c, buf, grown(bytes, up)); };
	CHECK(ensure_up(d.stream, (size_t)total + 64));
	if (d.carry) HIPCHECK(c, hipMemcpyAsync(d.stream.p, d.carrybuf.p, d.carry, hipMemcpyDeviceToDevice, st)); // the unfinished record of the previous chunk
	if (n_blocks) {
		ssv_bamdec_state::CompSlot *from = nullptr; // the chunk was announced ahead: its bytes are in (or on their way into) a slot
		for (auto &sl : d.slot) if (sl.host == comp && sl.bytes == comp_bytes) from = &sl;
		if (!from) CHECK(ensure_up(d.comp, comp_bytes + 64));
		const uint8_t *comp_dev = from ? static_cast<const uint8_t *>(from->buf.p) : static_cast<const uint8_t *>(d.comp.p);
		CHECK(ensure_up(d.blocks, (size_t)n_blocks * sizeof(ssv::BgzfBlock)));
		CHECK(ensure_up(d.u_off, ((size_t)n_blocks + 1) * 8));
		CHECK(ensure_up(d.status, (size_t)n_blocks * 4));
		{
			ProfScope up(c, P_BAM_UPLOAD, (int64_t)comp_bytes); // the compressed bytes' way over PCIe, apart from the kernels' time
			if (from) { if (from->via_link) { link_wait(c, from->up_sig); link_timed(c, from->up_sig, from->bytes, false); } else HIPCHECK(c, hipStreamWaitEvent(st, from->up, 0)); }
			else {
				bool done = false;
				if (c->link.ok && link_host_ok(comp) && (d.own_sig.handle || c->link.signal_create(0, 0, nullptr, &d.own_sig) == HSA_STATUS_SUCCESS)) {
					HIPCHECK(c, hipStreamSynchronize(st)); // (d.comp's last reader: the chunk before)
					c->link.signal_store(d.own_sig, 1);
					if (link_copy(c, d.comp.p, comp, comp_bytes, false, d.own_sig)) { link_wait(c, d.own_sig); link_timed(c, d.own_sig, comp_bytes, false); done = true; }
					else c->link.signal_store(d.own_sig, 0);
				}
				if (!done) HIPCHECK(c, hipMemcpyAsync(d.comp.p, comp, comp_bytes, hipMemcpyHostToDevice, st));
			}
			HIPCHECK(c, hipMemcpyAsync(d.blocks.p, d.hblocks.data(), (size_t)n_blocks * sizeof(ssv::BgzfBlock), hipMemcpyHostToDevice, st));
			HIPCHECK(c, hipMemcpyAsync(d.u_off.p, d.huoff.data(), ((size_t)n_blocks + 1) * 8, hipMemcpyHostToDevice, st));
		}
		ProfScope ps(c, P_BAM_INFLATE, (int64_t)(total - d.carry));
		const size_t n_waves = (size_t)((n_blocks + WAVE - 1) / WAVE);
		CHECK(ensure_up(d.inf_scratch, (n_waves + 8) * ssv::INFLATE_SCRATCH_BYTES)); // (per lane: the same bytes whatever the wavefront width)
		{
			// decode and copy as two passes: pass 1 leaves a token per match, pass 2 fills the holes (k_bgzf_tokens, k_bgzf_resolve)
			d.htokoff.resize((size_t)n_blocks + 1);
			uint64_t words = 0;
			for (int64_t b = 0; b < n_blocks; ++b) { d.htokoff[(size_t)b] = words; words += ssv::token_capacity(blocks[b].u_len); }
			d.htokoff[(size_t)n_blocks] = words;
			CHECK(ensure_up(d.tokens, (size_t)words * 4 + 64)); CHECK(ensure_up(d.tok_off, ((size_t)n_blocks + 1) * 8)); CHECK(ensure_up(d.n_tok, (size_t)n_blocks * 4 + 16));
			HIPCHECK(c, hipMemcpyAsync(d.tok_off.p, d.htokoff.data(), ((size_t)n_blocks + 1) * 8, hipMemcpyHostToDevice, st));
			const size_t lds = ((size_t)ssv::INFLATE_LDS_BYTES / 64 + ssv::TOKENS_WINDOW + ssv::TOKENS_BASE_BYTES) * (size_t)WAVE;
			// Pass 1 has two forms with the same output.  A lane per block (k_bgzf_tokens) needs tens of thousands of blocks in flight: its rate is blocks x 1 /
			// latency.  A wavefront per block with a speculative parallel decode (k_bgzf_tokens_wave, inflate_wave.h) keeps its rate down to a few hundred
			// blocks: 250 MB of real reads 11.2 -> 1.8 ms, 1 GB 11.2 -> 4.2 ms, 4 GB 13.3 -> 14.3 ms; 4 GB of the realistic synthetic file 20.2 -> 17.0 ms.
			// So: the wavefront form up to 64 K blocks (4 GB inflated), the lane form above; SSV_TOKENS=wave | lanes forces one.
			static const int tokens_mode = []() { const char *e = getenv("SSV_TOKENS"); return !e ? 0 : !strcmp(e, "wave") ? 1 : !strcmp(e, "lanes") ? 2 : 0; }();
			const bool tokens_wave = tokens_mode == 1 || (tokens_mode == 0 && n_blocks <= 65536);
			if (tokens_wave) {
				static const bool tw_phases = getenv("SSV_INFLATE_PHASES") != nullptr;
				unsigned long long *tw_dbg = nullptr;
				if (tw_phases) { CHECK(ensure_up(d.inf_dbg, 16 * 8)); HIPCHECK(c, hipMemsetAsync(d.inf_dbg.p, 0, 16 * 8, st)); tw_dbg = P<unsigned long long>(d.inf_dbg); }
				if (tw_phases)
					hipLaunchKernelGGL(ssv::k_bgzf_tokens_wave<true>, dim3((unsigned)n_blocks), dim3(WAVE), 0, st, comp_dev, P<ssv::BgzfBlock>(d.blocks), P<uint64_t>(d.u_off), P<uint64_t>(d.tok_off), n_blocks,
					                   P<uint8_t>(d.stream), P<uint32_t>(d.tokens), P<uint32_t>(d.n_tok), P<int>(d.status), tw_dbg);
				else
					hipLaunchKernelGGL(ssv::k_bgzf_tokens_wave<false>, dim3((unsigned)n_blocks), dim3(WAVE), 0, st, comp_dev, P<ssv::BgzfBlock>(d.blocks), P<uint64_t>(d.u_off), P<uint64_t>(d.tok_off), n_blocks,
					                   P<uint8_t>(d.stream), P<uint32_t>(d.tokens), P<uint32_t>(d.n_tok), P<int>(d.status), tw_dbg);
				if (tw_phases) {
					unsigned long long h[16];
					HIPCHECK(c, hipMemcpyAsync(h, tw_dbg, sizeof(h), hipMemcpyDeviceToHost, st));
					HIPCHECK(c, hipStreamSynchronize(st));
					const double nb = (double)n_blocks, win = (double)std::max<unsigned long long>(h[1], 1);
					fprintf(stderr, "[tokens wave] %lld BGZF blocks: %.2f deflate blocks and %.1f windows each; %.2f extra decode rounds per window, %.1f lanes decoding in rounds after the second per window; "
					        "most rounds in one window %llu; cycles per BGZF block: window loads %.0f, headers + tables %.0f, first round %.0f, later rounds %.0f, count + emit %.0f\n", (long long)n_blocks, h[0] / nb, h[1] / nb, h[2] / win, h[3] / win,
					        h[9], h[4] / nb, h[5] / nb, h[6] / nb, h[7] / nb, h[8] / nb);
					fprintf(stderr, "[tokens wave] symbols per lane in a window's first round: the busiest lane %.1f, the average lane %.1f\n", (double)h[10] / win, (double)h[11] / win / 64.0);
				}
			} else
				hipLaunchKernelGGL((ssv::k_bgzf_tokens<WAVE>), dim3((unsigned)n_waves), dim3(WAVE), lds, st, comp_dev, P<ssv::BgzfBlock>(d.blocks), P<uint64_t>(d.u_off), P<uint64_t>(d.tok_off), n_blocks,
				                   P<uint8_t>(d.stream), P<uint32_t>(d.tokens), P<uint32_t>(d.n_tok), P<int>(d.status), P<uint8_t>(d.inf_scratch));
			ProfScope pr(c, P_BAM_RESOLVE, (int64_t)(total - d.carry)); // (inside bam_inflate's scope: that one is both passes)
			// pass 2 with a window of the block in LDS, a wavefront per block (k_bgzf_resolve_win, the default: 8.6-8.8 ms per 5.3 GB of the realistic file);
			// SSV_RESOLVE=wave: the same mapping working in global memory (k_bgzf_resolve_wave: 13.7 ms; the reference form the tests hold the default against)
			static const bool resolve_win = []() { const char *e = getenv("SSV_RESOLVE"); return !e || strcmp(e, "wave") != 0; }();
			if (resolve_win) {
				static const bool rw_phases = getenv("SSV_INFLATE_PHASES") != nullptr;
				if (rw_phases) {
					CHECK(ensure_up(d.inf_dbg, 16 * 8)); HIPCHECK(c, hipMemsetAsync(d.inf_dbg.p, 0, 16 * 8, st));
					hipLaunchKernelGGL(ssv::k_bgzf_resolve_win<true>, dim3((unsigned)((n_blocks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)), dim3(BLOCK), 0, st, P<uint32_t>(d.tokens), P<uint64_t>(d.tok_off), P<uint32_t>(d.n_tok),
					                   P<uint64_t>(d.u_off), P<ssv::BgzfBlock>(d.blocks), n_blocks, P<uint8_t>(d.stream), P<unsigned long long>(d.inf_dbg));
					unsigned long long h[16];
					HIPCHECK(c, hipMemcpyAsync(h, d.inf_dbg.p, sizeof(h), hipMemcpyDeviceToHost, st));
					HIPCHECK(c, hipStreamSynchronize(st));
					const double r = (double)std::max<unsigned long long>(h[0], 1);
					fprintf(stderr, "[resolve win] %lld BGZF blocks, %.1f rounds each; per round: %.1f tokens, %.2f phases, %.2f all-lanes matches, %.3f window moves; cycles per round: window %.0f, dependencies %.0f, "
					        "own-lane copies %.0f, all-lanes copies %.0f, store + rest %.0f\n", (long long)n_blocks, r / (double)n_blocks, h[3] / r, h[1] / r, h[2] / r, h[4] / r, h[5] / r, h[6] / r, h[7] / r, h[8] / r, h[9] / r);
				} else
					hipLaunchKernelGGL(ssv::k_bgzf_resolve_win<false>, dim3((unsigned)((n_blocks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)), dim3(BLOCK), 0, st, P<uint32_t>(d.tokens), P<uint64_t>(d.tok_off), P<uint32_t>(d.n_tok),
					                   P<uint64_t>(d.u_off), P<ssv::BgzfBlock>(d.blocks), n_blocks, P<uint8_t>(d.stream), (unsigned long long *)nullptr);
			}
			else
				hipLaunchKernelGGL(ssv::k_bgzf_resolve_wave, dim3((unsigned)((n_blocks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)), dim3(BLOCK), 0, st, P<uint32_t>(d.tokens), P<uint64_t>(d.tok_off), P<uint32_t>(d.n_tok),
				                   P<uint64_t>(d.u_off), n_blocks, P<uint8_t>(d.stream));
		}
		if (d.verify_crc) {
			if (!d.crc_tab.p) { // the tables, once: slice-by-4, the 1024-byte advance, powers of x (zlib's crc32 arithmetic, made here)
				std::unique_ptr<ssv::CrcTab> hp(new ssv::CrcTab); // (a local: rank threads reach their first decode together)
				ssv::CrcTab &h = *hp;
				auto mult = [](uint32_t a, uint32_t b) { uint32_t m = 1u << 31, p = 0; for (;;) { if (a & m) { p ^= b; if ((a & (m - 1u)) == 0) break; } m >>= 1; b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1; } return p; };
				for (uint32_t i = 0; i < 256; ++i) { uint32_t v = i; for (int k = 0; k < 8; ++k) v = (v & 1u) ? (v >> 1) ^ 0xedb88320u : v >> 1; h.slice[0][i] = v; }
				for (int k = 1; k < 4; ++k) for (uint32_t i = 0; i < 256; ++i) h.slice[k][i] = (h.slice[k - 1][i] >> 8) ^ h.slice[0][h.slice[k - 1][i] & 0xffu];
				uint32_t p = 1u << 30; // x^1
				h.x2n[0] = p;
				for (int k = 1; k < 32; ++k) h.x2n[k] = p = mult(p, p);
				h.xr[0] = 1u << 31; // x^0
				for (int r = 1; r < 16; ++r) h.xr[r] = mult(h.xr[r - 1], h.x2n[3]);       // x^(8 r)
				h.w16[0] = 1u << 31;
				for (int m = 1; m <= 128; ++m) h.w16[m] = mult(h.w16[m - 1], h.x2n[7]);   // x^(128 m) = x^(8 x 16 m)
				const uint32_t x1k = h.w16[64];                                           // x^(8 x 1024)
				for (int k = 0; k < 4; ++k) for (uint32_t i = 0; i < 256; ++i) h.adv[k][i] = mult(x1k, i << (8 * k));
				CHECK(ensure(c, d.crc_tab, sizeof(h)));
				HIPCHECK(c, hipMemcpyAsync(d.crc_tab.p, &h, sizeof(h), hipMemcpyHostToDevice, st));
				HIPCHECK(c, hipStreamSynchronize(st));
			}
			hipLaunchKernelGGL(ssv::k_bgzf_crc, dim3((unsigned)n_blocks), dim3(WAVE), 0, st, comp_dev, P<ssv::BgzfBlock>(d.blocks), P<uint64_t>(d.u_off), n_blocks, P<uint8_t>(d.stream),
			                   P<ssv::CrcTab>(d.crc_tab), P<int>(d.status));
		}
		if (from) { HIPCHECK(c, hipEventRecord(from->done, st)); from->read = true; from->host = nullptr; }
	}
	d.info.n_records = 0; d.info.unmapped_raw = nullptr; d.info.unmapped_bytes = 0; d.info.n_tid_runs = 0; d.info.tid_run_index = nullptr; d.info.tid_run_tid = nullptr;
	d.info.inflated_bytes = total - d.carry;
	if (n_blocks == 0) {
		// end of input: whatever is carried must be nothing
		if (d.carry) { c->err = "truncated BAM record"; return SSV_E_ARG; }
		return SSV_OK;
	}
	// ---- record boundaries ----
	const int64_t n_units = n_blocks * ssv::UNITS_PER_BLOCK; // the record starts are searched per quarter block (bamdec_kernels.h)
	CHECK(ensure_up(d.chain, (size_t)n_units * sizeof(ssv::BlockChain)));
	CHECK(ensure_up(d.rel, (size_t)((n_units + 63) / 64) * ssv::REL_CAP * 64 * 2 + 64));
	CHECK(ensure_up(d.count, (size_t)n_units * 4 + 16)); CHECK(ensure_up(d.base, (size_t)n_units * 4 + 16));
	CHECK(ensure_up(d.stitch, sizeof(ssv::StitchOut))); CHECK(ensure_up(d.small, 256));
	CHECK(ensure_host(c, d.h_small, 256)); CHECK(ensure_host(c, d.h_status, (size_t)n_blocks * 4));
	CHECK(ensure_up(c->scan_scratch, (size_t)scan_scratch_elems(std::max<int64_t>(n_units, (int64_t)(total / 36 + 1))) * 8 + 64));
	CHECK(ensure_up(c->scan_scratch64, (size_t)scan_scratch_elems((int64_t)(total / 36 + 1)) * 8 + 64));
	{
		ProfScope ps(c, P_BAM_RECORDS, n_blocks);
		hipLaunchKernelGGL(ssv::k_find_records, dim3((unsigned)((n_units + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P<uint8_t>(d.stream), P<ssv::BgzfBlock>(d.blocks), P<uint64_t>(d.u_off), n_units,
		                   d.start, stream_end, d.n_targets, d.have_tlen ? P<int32_t>(d.tlen) : (const int32_t *)nullptr, P<ssv::BlockChain>(d.chain), P<uint16_t>(d.rel));
		HIPCHECK(c, hipMemsetAsync(d.stitch.p, 0, sizeof(ssv::StitchOut), st));
		hipLaunchKernelGGL(ssv::k_stitch_check, dim3((unsigned)((n_units + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P<ssv::BgzfBlock>(d.blocks), P<uint64_t>(d.u_off), n_units, d.start, stream_end, P<ssv::BlockChain>(d.chain),
		                   P<uint32_t>(d.count), P<ssv::StitchOut>(d.stitch));
		hipLaunchKernelGGL(ssv::k_stitch_blocks, dim3(1), dim3(WAVE), 0, st, P<uint8_t>(d.stream), P<ssv::BgzfBlock>(d.blocks), P<uint64_t>(d.u_off), n_units, d.start, stream_end,
		                   P<ssv::BlockChain>(d.chain), P<uint32_t>(d.count), P<ssv::StitchOut>(d.stitch));
		exclusive_scan<uint32_t, uint32_t>(st, P<uint32_t>(d.count), P<uint32_t>(d.base), n_units, 0u, P<uint32_t>(c->scan_scratch), (uint32_t *)nullptr);
	}
	HIPCHECK(c, hipMemcpyAsync(d.h_small.p, d.stitch.p, sizeof(ssv::StitchOut), hipMemcpyDeviceToHost, st));
	HIPCHECK(c, hipMemcpyAsync(d.h_status.p, d.status.p, (size_t)n_blocks * 4, hipMemcpyDeviceToHost, st));
	HIPCHECK(c, hipStreamSynchronize(st));
	for (int64_t b = 0; b < n_blocks; ++b)
		if (P<int>(d.h_status)[b] != 0) {
			c->err = P<int>(d.h_status)[b] == ssv::INF_E_CRC ? "BGZF block " + std::to_string(b) + " of the chunk: CRC32 mismatch (its bytes are not what was written)"
			                                                 : "BGZF inflate failed (block " + std::to_string(b) + " of the chunk, code " + std::to_string(P<int>(d.h_status)[b]) + ")";
			return SSV_E_ARG;
		}
	const ssv::StitchOut so = *P<ssv::StitchOut>(d.h_small);
	if (so.corrupt) { c->err = "corrupt BAM record"; return SSV_E_ARG; }
	const int64_t n = so.n_records;
	d.info.n_records = n; d.info.repaired_blocks = so.n_repaired; d.info.tail_offset = so.tail;
	d.carry = stream_end - so.tail; d.start = 0;
	if (d.carry) { // keep the head of the unfinished record for the next chunk
		CHECK(ensure_up(d.carrybuf, (size_t)d.carry + 64));
		HIPCHECK(c, hipMemcpyAsync(d.carrybuf.p, P<uint8_t>(d.stream) + so.tail, d.carry, hipMemcpyDeviceToDevice, st));
	}
	if (n == 0) return SSV_OK;
	// ---- records -> columns ----
	const size_t N = (size_t)n;
	CHECK(ensure_up(d.rec_off, N * 8 + 16));
	CHECK(d.cols.reserve(c, N, up));
	CHECK(ensure_up(d.stash, N * 8 + 16)); CHECK(ensure_up(d.seq_list, N * 4 + 16)); CHECK(ensure_up(d.raw_bytes, N * 4 + 16)); CHECK(ensure_up(d.raw_off, N * 8 + 16));
	CHECK(d.tl.reserve(c, n, up));
	// d.small: [0] max_span i32, [1] bad u32, [2] n_runs u32, [3] last_tid i32, [4..5] cigar total u32 (+pad), [6..7] seq total u64, [8..9] raw total u64, [10] records on the bases / XC list
	HIPCHECK(c, hipMemsetAsync(d.small.p, 0, 256, st));
	uint32_t *sm = P<uint32_t>(d.small);
	{
		ProfScope ps(c, P_BAM_DECODE, n);
		hipLaunchKernelGGL(ssv::k_list_records, dim3((unsigned)((n_units + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P<uint8_t>(d.stream), P<ssv::BlockChain>(d.chain), P<uint32_t>(d.count),
		                   P<uint32_t>(d.base), n_units, P<uint16_t>(d.rel), P<uint64_t>(d.rec_off));
		const ssv::RecColumns rc{P<uint32_t>(d.raw_bytes), P<uint2>(d.stash), reinterpret_cast<int32_t *>(sm), sm + 1};
		hipLaunchKernelGGL(ssv::k_record_fields, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P<uint8_t>(d.stream), P<uint64_t>(d.rec_off), n, keep_all_seq, d.cols.view(), rc);
		d.cols.layout(st, n, P<uint32_t>(c->scan_scratch), P<uint64_t>(c->scan_scratch64), sm + 4, reinterpret_cast<uint64_t *>(sm + 6));
		exclusive_scan<uint32_t, uint64_t>(st, P<uint32_t>(d.raw_bytes), P<uint64_t>(d.raw_off), n, 0ull, P<uint64_t>(c->scan_scratch64), reinterpret_cast<uint64_t *>(sm + 8));
	}
	// sizes of the variable parts, then exactly sized buffers
	HIPCHECK(c, hipMemcpyAsync(d.h_small.p, d.small.p, 64, hipMemcpyDeviceToHost, st));
	HIPCHECK(c, hipStreamSynchronize(st));
	uint64_t seq_total, raw_total;
	const uint32_t cigar_total = P<uint32_t>(d.h_small)[4];
	memcpy(&seq_total, P<uint32_t>(d.h_small) + 6, 8); memcpy(&raw_total, P<uint32_t>(d.h_small) + 8, 8);
	if (P<uint32_t>(d.h_small)[1]) { c->err = "corrupt BAM record"; return SSV_E_ARG; }
	CHECK(d.cols.reserve_variable(c, cigar_total, (size_t)seq_total, up)); CHECK(ensure_up(d.raw, (size_t)raw_total + 64));
	const ssv::DecodedCols col = d.cols.view();
	{
		ProfScope ps(c, P_BAM_DECODE, n);
		hipLaunchKernelGGL(ssv::k_record_cigars, dim3((unsigned)((n + BLOCK * ssv::CIGARS_PER_THREAD - 1) / (BLOCK * ssv::CIGARS_PER_THREAD))), dim3(BLOCK), 0, st, P<uint8_t>(d.stream), P<uint64_t>(d.rec_off), n, col.n_cigar,
		                   col.cigar_off, P<uint2>(d.stash), col.seq_bytes, col.xc, col.seq_off, col.cigar, P<uint32_t>(d.seq_list), sm + 10);
		hipLaunchKernelGGL(ssv::k_record_seqs, dim3((unsigned)std::min<int64_t>((n * 16 + BLOCK - 1) / BLOCK, 2048)), dim3(BLOCK), 0, st, P<uint8_t>(d.stream), P<uint64_t>(d.rec_off),
		                   col.n_cigar, col.seq_bytes, col.seq_off, P<uint32_t>(d.seq_list), sm + 10, col.seqqual, col.xc);
		hipLaunchKernelGGL(ssv::k_raw_copy, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, P<uint8_t>(d.stream), P<uint64_t>(d.rec_off), n, P<uint32_t>(d.raw_bytes), P<uint64_t>(d.raw_off), P<uint8_t>(d.raw));
		CHECK(d.tl.launch(c, st, col.tid, col.flag, n, d.prev_tid, sm + 2, reinterpret_cast<int32_t *>(sm + 3), sm + 11));
	}
	HIPCHECK(c, hipMemcpyAsync(d.h_small.p, d.small.p, 64, hipMemcpyDeviceToHost, st));
	HIPCHECK(c, hipStreamSynchronize(st));
	const uint32_t *hs = P<uint32_t>(d.h_small);
	uint32_t n_runs = hs[2];
	if (n_runs > TidLists::RUN_CAP) {
		if (!d.any_order) { c->err = "more than 65536 contig changes in one chunk: the BAM is not coordinate sorted"; return SSV_E_ARG; }
		n_runs = 0; // (ssv_bamdec_any_order: the list is incomplete - not handed out; the kernel wrote no more than run_cap entries)
	}
	d.prev_tid = (int32_t)hs[3];
	// the small host-side lists
	HBuf &h_raw = d.h_raw[d.raw_flip ^= 1];
	CHECK(ensure_host(c, h_raw, (size_t)raw_total + 64));
	CHECK(d.tl.fetch(c, st, n_runs));
	if (raw_total) HIPCHECK(c, hipMemcpyAsync(h_raw.p, d.raw.p, (size_t)raw_total, hipMemcpyDeviceToHost, st));
	if (n_runs || raw_total) HIPCHECK(c, hipStreamSynchronize(st));
	d.tl.changes(n_runs, d.info);
	d.info.unmapped_raw = P<uint8_t>(h_raw); d.info.unmapped_bytes = raw_total; d.info.last_tid = d.prev_tid;
	d.cols.fill(out, n, (int64_t)cigar_total, (int64_t)seq_total);
	out->max_ref_span = (int32_t)hs[0] > 0 ? (int32_t)hs[0] : 1;
	d.tl.batch_runs(hs[11], out);
	return SSV_OK;
}

// the names of the last decoded chunk's records: in the inflated stream, behind each record's block_size and 32-byte core
int ssv_bamdec_names(ssv_ctx *c, ssv_names_t *out)
{
	if (!c || !out) return SSV_E_ARG;
	if (!c->bd) { c->err = "ssv_bamdec_names before ssv_bamdec_begin"; return SSV_E_STATE; }
	memset(out, 0, sizeof(*out));
	out->mem = SSV_MEM_DEVICE; out->bias = 36;
	out->base = P<char>(c->bd->stream); out->off = P<uint64_t>(c->bd->rec_off);
	return SSV_OK;
}

// where the optional fields of the last decoded chunk's records lie in the inflated stream (k_bam_aux_span: computed when asked for, never by a decode)
int ssv_bamdec_aux(ssv_ctx *c, ssv_aux_t *out)
{
	if (!c || !out) return SSV_E_ARG;
	if (!c->bd) { c->err = "ssv_bamdec_aux before ssv_bamdec_begin"; return SSV_E_STATE; }
	ssv_bamdec_state &d = *c->bd;
	const int64_t n = d.info.n_records;
	memset(out, 0, sizeof(*out));
	out->mem = SSV_MEM_DEVICE; out->encoding = SSV_AUX_BAM; out->n = n;
	if (n <= 0) { out->n = 0; return SSV_OK; }
	HIPCHECK(c, hipSetDevice(c->device));
	CHECK(ensure(c, d.aux_off, (size_t)n * 8 + 16)); CHECK(ensure(c, d.aux_len, (size_t)n * 4 + 16));
	{
		ProfScope ps(c, P_SPLITREAD_SA_AUX, n);
		k_bam_aux_span<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(P<uint8_t>(d.stream), P<uint64_t>(d.rec_off), n, P<uint64_t>(d.aux_off), P<uint32_t>(d.aux_len));
		HIPCHECK(c, hipGetLastError());
	}
	out->base = P<uint8_t>(d.stream); out->off = P<uint64_t>(d.aux_off); out->len = P<uint32_t>(d.aux_len);
	return SSV_OK;
}

int ssv_bamdec_last(ssv_ctx *c, ssv_bamdec_info *info)
{
	if (!c || !c->bd || !info) return SSV_E_ARG;
	*info = c->bd->info;
	return SSV_OK;
}
