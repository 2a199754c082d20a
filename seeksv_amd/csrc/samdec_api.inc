// samdec_api.inc - host side of the device SAM-text decoder (included by seeksv_hip.hip inside extern "C"); kernels in samdec_kernels.h.
// Per chunk: [carried line | text] in one buffer -> k_sam_count -> scans of the tile sums -> (sync: separators, lines) -> k_sam_marks -> k_sam_sizes ->
// scans -> (sync: totals) -> k_sam_fields, k_sam_seqqual, the unfinished line to the side buffer -> (sync: refusals) -> device batch + names.
// After ssv_samdec_sorted (a coordinate-sorted original: what getclip and `seeksv run` read) the same two synchronisations carry more: k_sam_sizes_sorted also
// sizes the list of the lines that ship bases + qualities and the side channel's records (two more scans); behind k_sam_fields_sorted come k_sam_seqqual_list,
// k_sam_raw and the four k_tid_* kernels the BAM decoder runs (TidLists); the small host-side lists follow the refusal word (ssv_samdec_lists).

struct ssv_samdec_state {
	enum { IDLE, ACTIVE, ENDED, FAILED } phase = IDLE;
	int32_t n_targets = 0;
	uint64_t first_line = 1, lines_done = 0, carry = 0;
	uint32_t ref_mask = 15;
	DBuf ref_slots, ref_off, ref_blob;
	DBuf text, carrybuf, tile_sep, tile_nl, sep, nlidx, small;
	DecodedColumns cols; // the batch handed out
	DBuf name_off, rec;
	DBuf aux_off, aux_len; // ssv_samdec_aux: where each line's optional fields lie (only when asked for)
	HBuf h_small;
	// chunks announced ahead (ssv_samdec_prefetch): on the upload stream into one of two slots, moved behind the carried line by the decode call
	struct Slot { DBuf buf; const void *host = nullptr; size_t bytes = 0; hipEvent_t up = nullptr, done = nullptr; bool read = false; } slot[2];
	int next_slot = 0;
	bool have_batch = false;
	uint64_t text_bytes = 0;
	ssv_samdec_info info{};
	// ssv_samdec_sorted: a coordinate-sorted original
	bool sorted = false, keep_all_seq = false, decoded = false, have_lists = false;
	bool any_order = false; // ssv_samdec_any_order: chunks with more contig changes than the list holds go through without the list
	int32_t prev_tid = 0; // contig of the last mapped-pair record so far (clip_reads.h:407: starts at 0)
	DBuf ship, ship_idx, seq_list, raw_bytes, raw_off, raw;
	HBuf h_raw[2]; // two in turn, as the BAM decoder's: a chunk's UNMAP|MUNMAP records stay valid while the next chunk is decoded
	int raw_flip = 0;
	TidLists tl;
	ssv_bamdec_info lists{};
};

static const char *const kSamReasons[ssv::SAM_E_COUNT] = {
	"", "fewer than 11 fields", "empty line", "header line among the records", "read name is empty or longer than 254 bytes", "a number is missing, malformed or out of range",
	"invalid CIGAR character", "CIGAR operation without a length", "more than 65535 CIGAR operations", "CIGAR and sequence length are inconsistent", "sequence and quality are inconsistent",
	"quality byte below 33", "NUL byte"};

static void samdec_release_handles(ssv_ctx *c)
{
	ssv_samdec_state *d = c->sd.get();
	if (!d) return;
	for (auto &sl : d->slot) { if (sl.up) (void)hipEventDestroy(sl.up); if (sl.done) (void)hipEventDestroy(sl.done); }
}

int ssv_samdec_begin(ssv_ctx *c, const ssv_samdec_params *p)
{
	if (!c) return SSV_E_ARG;
	if (!p || p->n_targets < 0 || (p->n_targets > 0 && !p->target_names) || p->first_line < 1) { c->err = "ssv_samdec_begin: bad parameters"; return SSV_E_ARG; }
	for (int32_t t = 0; t < p->n_targets; ++t) if (!p->target_names[t]) { c->err = "ssv_samdec_begin: bad parameters"; return SSV_E_ARG; }
	HIPCHECK(c, hipSetDevice(c->device));
	if (!c->sd) c->sd.reset(new ssv_samdec_state());
	ssv_samdec_state &d = *c->sd;
	d.phase = ssv_samdec_state::IDLE;
	{ // copies still on their way into a slot land in a slot nobody asks for
		bool any = false;
		for (auto &sl : d.slot) { any = any || sl.host; sl.host = nullptr; }
		if (any) HIPCHECK(c, hipStreamSynchronize(c->st_h2d));
	}
	d.n_targets = p->n_targets; d.first_line = p->first_line; d.lines_done = 0; d.carry = 0; d.have_batch = false;
	d.sorted = d.keep_all_seq = d.decoded = d.have_lists = d.any_order = false; d.prev_tid = 0;
	memset(&d.lists, 0, sizeof(d.lists));
	memset(&d.info, 0, sizeof(d.info));
	// the contig names as a hash table: FNV-1a, linear probing, at most half full; the first of two equal names wins
	uint32_t size = 16;
	while (size < 2u * (uint32_t)p->n_targets) size <<= 1;
	std::vector<uint32_t> slots(size, 0u), off((size_t)p->n_targets + 1, 0u);
	std::string blob;
	for (int32_t t = 0; t < p->n_targets; ++t) {
		const char *z = p->target_names[t];
		const size_t len = strlen(z);
		off[(size_t)t] = (uint32_t)blob.size();
		blob.append(z, len);
		uint32_t h = 2166136261u;
		for (size_t k = 0; k < len; ++k) h = (h ^ (uint8_t)z[k]) * 16777619u;
		bool dup = false;
		uint32_t at = h & (size - 1);
		for (; slots[at]; at = (at + 1) & (size - 1)) {
			const uint32_t u = slots[at] - 1;
			if (off[u + 1] - off[u] == len && memcmp(blob.data() + off[u], z, len) == 0) { dup = true; break; }
		}
		off[(size_t)t + 1] = (uint32_t)blob.size();
		if (!dup) slots[at] = (uint32_t)t + 1;
	}
	d.ref_mask = size - 1;
	CHECK(ensure(c, d.ref_slots, (size_t)size * 4)); CHECK(ensure(c, d.ref_off, off.size() * 4)); CHECK(ensure(c, d.ref_blob, blob.size() + 16));
	HIPCHECK(c, hipMemcpyAsync(d.ref_slots.p, slots.data(), (size_t)size * 4, hipMemcpyHostToDevice, c->st));
	HIPCHECK(c, hipMemcpyAsync(d.ref_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->st));
	if (!blob.empty()) HIPCHECK(c, hipMemcpyAsync(d.ref_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, c->st));
	CHECK(ensure(c, d.small, 256)); CHECK(ensure_host(c, d.h_small, 256));
	HIPCHECK(c, hipStreamSynchronize(c->st)); // (the vectors go with the call)
	d.phase = ssv_samdec_state::ACTIVE;
	return SSV_OK;
}

int ssv_samdec_prefetch(ssv_ctx *c, const void *text, size_t bytes)
{
	if (!c) return SSV_E_ARG;
	if (!c->sd || c->sd->phase != ssv_samdec_state::ACTIVE) { c->err = "ssv_samdec_prefetch before ssv_samdec_begin"; return SSV_E_STATE; }
	if (!text || !bytes) { c->err = "ssv_samdec_prefetch: bad arguments"; return SSV_E_ARG; }
	ssv_samdec_state &d = *c->sd;
	HIPCHECK(c, hipSetDevice(c->device));
	for (auto &sl : d.slot) {
		if (sl.host == text && sl.bytes == bytes) return SSV_OK; // announced already
		if (sl.host == text) sl.host = nullptr;                    // the same memory with other contents: what was announced is given up
	}
	auto &sl = d.slot[d.next_slot];
	if (sl.host) return SSV_OK; // both slots are taken: this chunk is copied by its decode call
	d.next_slot ^= 1;
	if (!sl.up) { HIPCHECK(c, hipEventCreateWithFlags(&sl.up, hipEventDisableTiming)); HIPCHECK(c, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming)); }
	if (sl.buf.cap < bytes + 64 && sl.read) HIPCHECK(c, hipEventSynchronize(sl.done)); // (growing frees the old slot)
	CHECK(ensure(c, sl.buf, bytes + 64));
	if (sl.read) HIPCHECK(c, hipStreamWaitEvent(c->st_h2d, sl.done, 0)); // the chunk that was in this slot may still be on its way into the text buffer
	HIPCHECK(c, hipMemcpyAsync(sl.buf.p, text, bytes, hipMemcpyHostToDevice, c->st_h2d));
	HIPCHECK(c, hipEventRecord(sl.up, c->st_h2d));
	sl.host = text; sl.bytes = bytes; sl.read = false;
	return SSV_OK;
}

int ssv_samdec_sorted(ssv_ctx *c, int keep_all_seq)
{
	if (!c) return SSV_E_ARG;
	if (!c->sd || c->sd->phase != ssv_samdec_state::ACTIVE || c->sd->decoded) { c->err = "ssv_samdec_sorted belongs between ssv_samdec_begin and the first ssv_samdec_decode"; return SSV_E_ARG; }
	c->sd->sorted = true; c->sd->keep_all_seq = keep_all_seq != 0;
	return SSV_OK;
}

// Optional, after ssv_samdec_begin: text in any record order (`run -u`).  A chunk with more than 65536 contig changes among
// its mapped-pair records is then decoded like any other; only its contig-change list (ssv_samdec_lists: n_tid_runs) is not handed out.
int ssv_samdec_any_order(ssv_ctx *c, int on)
{
	if (!c) return SSV_E_ARG;
	if (!c->sd || c->sd->phase != ssv_samdec_state::ACTIVE) { c->err = "ssv_samdec_any_order before ssv_samdec_begin"; return SSV_E_ARG; }
	c->sd->any_order = on != 0;
	return SSV_OK;
}

// a chunk without a finished line: empty lists
static void samdec_no_lists(ssv_samdec_state &d, uint64_t text_bytes)
{
	memset(&d.lists, 0, sizeof(d.lists));
	d.lists.inflated_bytes = text_bytes; d.lists.last_tid = d.prev_tid;
	d.have_lists = d.sorted;
}

static int samdec_refuse(ssv_ctx *c, unsigned long long word)
{
	ssv_samdec_state &d = *c->sd;
	const uint32_t code = (uint32_t)(word & 0xffu);
	const uint64_t line = d.first_line + d.lines_done + (uint64_t)(word >> 8);
	d.info.refused_line = line;
	d.info.refused_reason = code < ssv::SAM_E_COUNT ? kSamReasons[code] : "malformed line";
	c->err = "Parse error at line " + std::to_string(line) + ": " + d.info.refused_reason;
	d.phase = ssv_samdec_state::FAILED;
	return SSV_E_ARG;
}

int ssv_samdec_decode(ssv_ctx *c, const void *text, size_t bytes, int mem, int last, ssv_batch_t *out)
{
	if (!c) return SSV_E_ARG;
	if (!c->sd || c->sd->phase != ssv_samdec_state::ACTIVE) { c->err = "ssv_samdec_decode before ssv_samdec_begin (or behind the file's end or a refused line)"; return SSV_E_STATE; }
	if (!out || (bytes && !text) || (mem != SSV_MEM_HOST && mem != SSV_MEM_DEVICE)) { c->err = "ssv_samdec_decode: bad arguments"; return SSV_E_ARG; }
	ssv_samdec_state &d = *c->sd;
	if (d.carry + (uint64_t)bytes >= 0xfffffff0ull) { c->err = "ssv_samdec_decode: the carried line and the chunk must stay below 4 GB"; return SSV_E_ARG; }
	HIPCHECK(c, hipSetDevice(c->device));
	hipStream_t st = c->st;
	memset(out, 0, sizeof(*out));
	out->mem = SSV_MEM_DEVICE;
	d.have_batch = false; d.have_lists = false; d.decoded = true;
	d.info.n_records = 0;
	const uint64_t total = d.carry + bytes;
	CHECK(ensure(c, d.text, (size_t)total + 128));
	uint8_t *tx = P<uint8_t>(d.text);
	if (d.carry) HIPCHECK(c, hipMemcpyAsync(tx, d.carrybuf.p, d.carry, hipMemcpyDeviceToDevice, st)); // the unfinished line of the chunk before, in front
	if (bytes) {
		ssv_samdec_state::Slot *from = nullptr;
		if (mem == SSV_MEM_HOST) for (auto &sl : d.slot) {
			if (sl.host == text && sl.bytes == bytes) from = &sl;
			else if (sl.host == text) sl.host = nullptr; // announced with another size: the slot is free again, this call copies the chunk itself
		}
		if (from) {
			HIPCHECK(c, hipStreamWaitEvent(st, from->up, 0));
			HIPCHECK(c, hipMemcpyAsync(tx + d.carry, from->buf.p, bytes, hipMemcpyDeviceToDevice, st));
			HIPCHECK(c, hipEventRecord(from->done, st));
			from->read = true; from->host = nullptr;
		} else HIPCHECK(c, hipMemcpyAsync(tx + d.carry, text, bytes, mem == SSV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
	}
	d.text_bytes = total;
	if (total == 0) {
		HIPCHECK(c, hipStreamSynchronize(st));
		d.info.carried_bytes = 0;
		if (last) d.phase = ssv_samdec_state::ENDED;
		d.have_batch = true;
		samdec_no_lists(d, bytes);
		return SSV_OK;
	}
	// a last line without its newline gets one (the kernels count it unless a newline stands in front of it)
	const int64_t len = (int64_t)total + (last ? 1 : 0), virt_at = last ? (int64_t)total : -1;
	if (last) HIPCHECK(c, hipMemsetAsync(tx + total, '\n', 1, st));
	const int64_t n_tiles = (len + ssv::SAM_TILE - 1) / ssv::SAM_TILE;
	CHECK(ensure(c, d.tile_sep, (size_t)n_tiles * 4 + 16)); CHECK(ensure(c, d.tile_nl, (size_t)n_tiles * 4 + 16));
	CHECK(ensure(c, c->scan_scratch, (size_t)scan_scratch_elems(n_tiles) * 8 + 64));
	// d.small: [0..1] the smallest refused (line << 8 | reason) u64, [2] separators, [3] lines, [4] CIGAR operations, [6..7] seqqual bytes u64, [8] max span i32;
	// sorted originals: [9] lines that ship, [10..11] side-channel bytes u64, [12] contig changes, [13] last contig i32, [14] runs of the tid column
	uint32_t *sm = P<uint32_t>(d.small);
	unsigned long long *errw = P<unsigned long long>(d.small);
	HIPCHECK(c, hipMemsetAsync(d.small.p, 0, 256, st));
	HIPCHECK(c, hipMemsetAsync(d.small.p, 0xff, 8, st));
	k_sam_count<<<(unsigned)n_tiles, BLOCK, 0, st>>>(tx, len, virt_at, P<uint32_t>(d.tile_sep), P<uint32_t>(d.tile_nl));
	HIPCHECK(c, hipGetLastError());
	exclusive_scan<uint32_t, uint32_t>(st, P<uint32_t>(d.tile_sep), P<uint32_t>(d.tile_sep), n_tiles, 0u, P<uint32_t>(c->scan_scratch), sm + 2);
	exclusive_scan<uint32_t, uint32_t>(st, P<uint32_t>(d.tile_nl), P<uint32_t>(d.tile_nl), n_tiles, 0u, P<uint32_t>(c->scan_scratch), sm + 3);
	HIPCHECK(c, hipMemcpyAsync(d.h_small.p, d.small.p, 64, hipMemcpyDeviceToHost, st));
	HIPCHECK(c, hipStreamSynchronize(st));
	const uint32_t *hs = P<uint32_t>(d.h_small);
	const uint32_t n_sep = hs[2];
	const int64_t n = hs[3];
	if (n == 0) { // not one finished line: everything is carried
		CHECK(ensure(c, d.carrybuf, (size_t)total + 64));
		HIPCHECK(c, hipMemcpyAsync(d.carrybuf.p, tx, total, hipMemcpyDeviceToDevice, st));
		HIPCHECK(c, hipStreamSynchronize(st));
		d.carry = total; d.info.carried_bytes = total;
		d.have_batch = true;
		samdec_no_lists(d, bytes);
		return SSV_OK;
	}
	const size_t N = (size_t)n;
	CHECK(ensure(c, d.sep, (size_t)n_sep * 4 + 16)); CHECK(ensure(c, d.nlidx, N * 4 + 16));
	CHECK(d.cols.reserve(c, N, 1.0));
	CHECK(ensure(c, d.name_off, N * 8 + 16)); CHECK(ensure(c, d.rec, N * sizeof(ssv_record) + 64));
	CHECK(ensure(c, c->scan_scratch, (size_t)scan_scratch_elems(n) * 8 + 64)); CHECK(ensure(c, c->scan_scratch64, (size_t)scan_scratch_elems(n) * 8 + 64));
	k_sam_marks<<<(unsigned)n_tiles, BLOCK, 0, st>>>(tx, len, virt_at, P<uint32_t>(d.tile_sep), P<uint32_t>(d.tile_nl), (uint32_t)n, P<uint32_t>(d.sep), P<uint32_t>(d.nlidx), errw);
	ssv::SamSortedCols srt{};
	if (d.sorted) {
		CHECK(ensure(c, d.ship, N * 4 + 16)); CHECK(ensure(c, d.ship_idx, N * 4 + 16)); CHECK(ensure(c, d.raw_bytes, N * 4 + 16)); CHECK(ensure(c, d.raw_off, N * 8 + 16));
		CHECK(d.tl.reserve(c, n, 1.0));
		srt = ssv::SamSortedCols{P<uint32_t>(d.ship), P<uint32_t>(d.raw_bytes), P<uint32_t>(d.ship_idx), nullptr, d.keep_all_seq ? 1 : 0};
		k_sam_sizes_sorted<<<grid_for(n, BLOCK), BLOCK, 0, st>>>(tx, P<uint32_t>(d.sep), P<uint32_t>(d.nlidx), n, d.cols.view(), srt, errw);
	} else
		k_sam_sizes<<<grid_for(n, BLOCK), BLOCK, 0, st>>>(tx, P<uint32_t>(d.sep), P<uint32_t>(d.nlidx), n, d.cols.view(), errw);
	HIPCHECK(c, hipGetLastError());
	d.cols.layout(st, n, P<uint32_t>(c->scan_scratch), P<uint64_t>(c->scan_scratch64), sm + 4, reinterpret_cast<uint64_t *>(sm + 6));
	if (d.sorted) {
		exclusive_scan<uint32_t, uint32_t>(st, srt.ship, P<uint32_t>(d.ship_idx), n, 0u, P<uint32_t>(c->scan_scratch), sm + 9);
		exclusive_scan<uint32_t, uint64_t>(st, srt.raw_bytes, P<uint64_t>(d.raw_off), n, 0ull, P<uint64_t>(c->scan_scratch64), reinterpret_cast<uint64_t *>(sm + 10));
	}
	HIPCHECK(c, hipMemcpyAsync(d.h_small.p, d.small.p, 64, hipMemcpyDeviceToHost, st));
	HIPCHECK(c, hipMemcpyAsync(P<uint32_t>(d.h_small) + 16, P<uint32_t>(d.nlidx) + (n - 1), 4, hipMemcpyDeviceToHost, st));
	HIPCHECK(c, hipStreamSynchronize(st));
	// (a line k_sam_sizes refused has sizes of zero: the kernels below still run, so that the FIRST refused line is named whichever kernel refuses it)
	unsigned long long werr;
	const uint32_t cigar_total = hs[4], last_nl_sep = hs[16];
	uint64_t seq_total;
	memcpy(&seq_total, hs + 6, 8);
	CHECK(d.cols.reserve_variable(c, cigar_total, (size_t)seq_total, 1.0));
	const uint32_t n_ship = d.sorted ? hs[9] : 0u;
	uint64_t raw_total = 0;
	if (d.sorted) {
		memcpy(&raw_total, hs + 10, 8);
		CHECK(ensure(c, d.seq_list, (size_t)n_ship * 4 + 16)); CHECK(ensure(c, d.raw, (size_t)raw_total + 64));
		srt.list = P<uint32_t>(d.seq_list);
	}
	const ssv::DecodedCols col = d.cols.view();
	const ssv::SamLineCols lines{P<uint64_t>(d.name_off), P<ssv_record>(d.rec)};
	ssv::SamRefTable T{P<uint32_t>(d.ref_slots), d.ref_mask, P<uint32_t>(d.ref_off), P<uint8_t>(d.ref_blob)};
	// where the last finished line ends (k_sam_fields puts NULs over the first tabs of finished lines only: the unfinished one is carried as it is)
	HIPCHECK(c, hipMemcpyAsync(P<uint32_t>(d.h_small) + 17, P<uint32_t>(d.sep) + last_nl_sep, 4, hipMemcpyDeviceToHost, st));
	if (d.sorted) {
		k_sam_fields_sorted<<<grid_for(n, BLOCK), BLOCK, 0, st>>>(tx, P<uint32_t>(d.sep), P<uint32_t>(d.nlidx), n, T, col, lines, srt, reinterpret_cast<int32_t *>(sm + 8), errw);
		if (n_ship)
			k_sam_seqqual_list<<<(unsigned)std::min<int64_t>(((int64_t)n_ship + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 8192), BLOCK, 0, st>>>(tx, P<uint32_t>(d.sep), P<uint32_t>(d.nlidx), srt.list, n_ship,
			                                                                                                                                col.l_qseq, col.seq_off, col.seqqual, errw);
		if (raw_total) k_sam_raw<<<grid_for(n, BLOCK), BLOCK, 0, st>>>(tx, P<uint32_t>(d.sep), P<uint32_t>(d.nlidx), n, col, srt.raw_bytes, P<uint64_t>(d.raw_off), P<uint8_t>(d.raw), errw);
		HIPCHECK(c, hipGetLastError());
		CHECK(d.tl.launch(c, st, col.tid, col.flag, n, d.prev_tid, sm + 12, reinterpret_cast<int32_t *>(sm + 13), sm + 14));
	} else {
		k_sam_fields<<<grid_for(n, BLOCK), BLOCK, 0, st>>>(tx, P<uint32_t>(d.sep), P<uint32_t>(d.nlidx), n, T, col, lines, reinterpret_cast<int32_t *>(sm + 8), errw);
		k_sam_seqqual<<<(unsigned)std::min<int64_t>((n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 8192), BLOCK, 0, st>>>(tx, P<uint32_t>(d.sep), P<uint32_t>(d.nlidx), n, col.l_qseq, col.seq_off,
		                                                                                                                 col.seqqual, errw);
	}
	HIPCHECK(c, hipGetLastError());
	HIPCHECK(c, hipMemcpyAsync(d.h_small.p, d.small.p, 64, hipMemcpyDeviceToHost, st));
	HIPCHECK(c, hipStreamSynchronize(st));
	memcpy(&werr, d.h_small.p, 8);
	if (werr != ssv::SAM_NO_ERROR) return samdec_refuse(c, werr);
	uint32_t n_runs = d.sorted ? hs[12] : 0u;
	const uint32_t n_raw_runs = d.sorted ? hs[14] : 0u;
	const int32_t last_tid = (int32_t)hs[13];
	if (n_runs > TidLists::RUN_CAP && d.any_order) n_runs = 0; // (the list is incomplete - not handed out; the kernel wrote no more than RUN_CAP entries)
	if (n_runs > TidLists::RUN_CAP) {
		c->err = "more than 65536 contig changes in one chunk: the SAM text is not coordinate sorted";
		d.phase = ssv_samdec_state::FAILED;
		return SSV_E_ARG;
	}
	// the unfinished last line: kept aside, moved in front of the next chunk's bytes by the next decode
	const uint64_t consumed = last ? total : (uint64_t)hs[17] + 1u;
	const uint64_t carry = total - consumed;
	if (carry) {
		CHECK(ensure(c, d.carrybuf, (size_t)carry + 64));
		HIPCHECK(c, hipMemcpyAsync(d.carrybuf.p, tx + consumed, carry, hipMemcpyDeviceToDevice, st));
	}
	if (d.sorted) { // the small host-side lists
		HBuf &h_raw = d.h_raw[d.raw_flip ^= 1];
		CHECK(ensure_host(c, h_raw, (size_t)raw_total + 64));
		CHECK(d.tl.fetch(c, st, n_runs));
		if (raw_total) HIPCHECK(c, hipMemcpyAsync(h_raw.p, d.raw.p, (size_t)raw_total, hipMemcpyDeviceToHost, st));
		if (carry || n_runs || raw_total) HIPCHECK(c, hipStreamSynchronize(st));
		memset(&d.lists, 0, sizeof(d.lists));
		d.prev_tid = last_tid;
		d.tl.changes(n_runs, d.lists);
		d.lists.n_records = n; d.lists.inflated_bytes = bytes; d.lists.last_tid = last_tid;
		d.lists.unmapped_raw = P<uint8_t>(h_raw); d.lists.unmapped_bytes = raw_total;
		d.have_lists = true;
	} else if (carry) HIPCHECK(c, hipStreamSynchronize(st));
	d.carry = carry;
	d.lines_done += (uint64_t)n;
	d.info.n_records = n; d.info.lines_consumed = d.lines_done; d.info.carried_bytes = carry;
	if (last) d.phase = ssv_samdec_state::ENDED;
	d.have_batch = true;
	d.cols.fill(out, n, (int64_t)cigar_total, (int64_t)seq_total);
	out->max_ref_span = (int32_t)hs[8] > 0 ? (int32_t)hs[8] : 1;
	out->rec = lines.rec;
	out->tid_runs = nullptr; out->n_tid_runs = 0;
	if (d.sorted) d.tl.batch_runs(n_raw_runs, out);
	return SSV_OK;
}

int ssv_samdec_names(ssv_ctx *c, ssv_names_t *out)
{
	if (!c || !out) return SSV_E_ARG;
	if (!c->sd || !c->sd->have_batch) { c->err = "ssv_samdec_names before a successful ssv_samdec_decode"; return SSV_E_STATE; }
	memset(out, 0, sizeof(*out));
	out->mem = SSV_MEM_DEVICE; out->bias = 0;
	out->base = P<char>(c->sd->text); out->off = P<uint64_t>(c->sd->name_off); out->bytes = (int64_t)c->sd->text_bytes;
	return SSV_OK;
}

// where the optional fields of the last decoded batch's lines lie in the context's copy of the text: field 12 to the line's end (k_sam_aux_span over the
// separators the decode left; computed when asked for, never by a decode)
int ssv_samdec_aux(ssv_ctx *c, ssv_aux_t *out)
{
	if (!c || !out) return SSV_E_ARG;
	if (!c->sd || !c->sd->have_batch) { c->err = "ssv_samdec_aux before a successful ssv_samdec_decode"; return SSV_E_STATE; }
	ssv_samdec_state &d = *c->sd;
	const int64_t n = d.info.n_records;
	memset(out, 0, sizeof(*out));
	out->mem = SSV_MEM_DEVICE; out->encoding = SSV_AUX_SAM; out->n = n;
	if (n <= 0) { out->n = 0; return SSV_OK; }
	HIPCHECK(c, hipSetDevice(c->device));
	CHECK(ensure(c, d.aux_off, (size_t)n * 8 + 16)); CHECK(ensure(c, d.aux_len, (size_t)n * 4 + 16));
	{
		ProfScope ps(c, P_SPLITREAD_SA_AUX, n);
		k_sam_aux_span<<<grid_for(n, BLOCK), BLOCK, 0, c->st>>>(P<uint8_t>(d.text), P<uint32_t>(d.sep), P<uint32_t>(d.nlidx), n, P<uint64_t>(d.aux_off), P<uint32_t>(d.aux_len));
		HIPCHECK(c, hipGetLastError());
	}
	out->base = P<uint8_t>(d.text); out->off = P<uint64_t>(d.aux_off); out->len = P<uint32_t>(d.aux_len);
	return SSV_OK;
}

int ssv_samdec_last(ssv_ctx *c, ssv_samdec_info *info)
{
	if (!c || !info) return SSV_E_ARG;
	if (!c->sd || c->sd->phase == ssv_samdec_state::IDLE) { c->err = "ssv_samdec_last before ssv_samdec_begin"; return SSV_E_STATE; }
	*info = c->sd->info;
	return SSV_OK;
}

int ssv_samdec_lists(ssv_ctx *c, ssv_bamdec_info *out)
{
	if (!c || !out) return SSV_E_ARG;
	if (!c->sd || !c->sd->have_lists) { c->err = "ssv_samdec_lists before a successful ssv_samdec_decode behind ssv_samdec_sorted"; return SSV_E_STATE; }
	*out = c->sd->lists;
	return SSV_OK;
}
