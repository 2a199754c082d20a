// splitread_sa_kernels.h - `seeksv run -A -S`: virtual candidates from the SA tag of a split read whose other record is absent (the rule:
// include/seeksv_hip.h at ssv_rt_begin_original_sa).  Beside the stages of splitread_kernels.h, for a session of that mode only:
// k_bam_aux_span / k_sam_aux_span (where each record's optional fields lie: the descriptor, asked for per batch) -> select and place as they are ->
// k_sa_parse (one lane per candidate: only a record that carries the read has its fields walked; SA value -> entry -> contig -> geometry; 1 or 2 store slots)
// -> scan -> k_sa_measure / k_sa_gather (k_sr_measure / k_sr_gather writing by slot, the virtual candidate right behind its source: no name copy, no bases,
// its non-clip operations decoded from the entry's text) -> at finish k_sa_pair (k_sr_pair over the real candidates alone, then the sources left without a
// partner against their virtual candidate).  Streaming byte and integer work: no LDS, plain vector stores, one atomic per wavefront and counter at the most.
#pragma once

#include "splitread_kernels.h"
#include "splitread_sa_parse.h"
#include "bamdec_kernels.h"
#include "samdec_kernels.h"

namespace ssv {

// RtCand::pad of a virtual candidate: never SR_CARRIES; its seq_off holds the store index of its source
enum : uint32_t { SR_VIRTUAL = 4u };
// the mode's statistics, in device memory beside SR_N_*: one 64-bit counter each
enum : int { SA_N_TAGS = 0, SA_N_MULTI = 1, SA_N_REFUSED = 2, SA_N_VIRTUALS = 3, SA_N_REDUNDANT = 4, SA_N_PAIRS = 5, SA_N_LENGTH = 6, SA_N_STATS = 8 };

// where the optional fields of record i lie: base + off[i], len[i] bytes, BAM's typed fields or SAM text
struct DevAux { const uint8_t *base; const uint64_t *off; const uint32_t *len; int enc; };

// BAM: behind the core, name, operations, bases and qualities, up to block_size; nothing for a record whose fields overrun it (the decoder flagged that one)
__global__ __launch_bounds__(BLOCK) void k_bam_aux_span(const uint8_t *__restrict__ u, const uint64_t *__restrict__ rec_off, int64_t n, uint64_t *__restrict__ off, uint32_t *__restrict__ len)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n) return;
	const uint8_t *rp = u + rec_off[i], *r = rp + 4;
	const uint64_t bs = ld_u32(rp);
	const int32_t l_seq = ld_i32(r + 16);
	const uint64_t l = l_seq < 0 ? 0 : (uint64_t)l_seq;
	const uint64_t at = 32ull + r[8] + 4ull * ld_u16(r + 12) + (l + 1) / 2 + l;
	const bool ok = l_seq >= 0 && at <= bs;
	off[i] = rec_off[i] + 4 + (ok ? at : bs);
	len[i] = ok ? (uint32_t)(bs - at) : 0u;
}

// SAM text: from the start of the line's field 12 to the line's end (without the newline and a '\r' in front of it); nothing for a line of eleven fields
__global__ __launch_bounds__(BLOCK) void k_sam_aux_span(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, int64_t n,
                                                        uint64_t *__restrict__ off, uint32_t *__restrict__ len)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n) return;
	const SamLine L = sam_line(text, sep, nlidx, i);
	const bool has = L.ntabs >= 11;
	const uint32_t s = has ? L.fs(sep, 11) : L.end;
	off[i] = s;
	len[i] = L.end - s;
}

// what k_sa_parse leaves for the gather: the virtual candidate's fields and where the entry's CIGAR text lies
struct SaVirt {
	int32_t tid, pos, lq, left, right;
	uint32_t n_keep, cig_len;
	uint8_t side, strand; uint16_t pad;
	const uint8_t *cig;
};

// one lane per candidate: slots[k] = 1, or 2 when it is a source whose SA value gives a virtual candidate (virt[k])
__global__ __launch_bounds__(BLOCK) void k_sa_parse(DevBatch b, DevAux ax, SaContigs T, const uint32_t *__restrict__ cand, int64_t m, int min_mapq,
                                                    SaVirt *__restrict__ virt, uint32_t *__restrict__ slots, unsigned long long *__restrict__ stats)
{
	const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	uint32_t tags = 0, multi = 0, refused = 0, made = 0;
	if (k < m) {
		const int64_t i = cand[k];
		const RecLine r = rec_load(b.rec, i);
		if (sr_carries(r, sr_shape(r, b.cigar))) { // a source: the only records whose optional fields are looked at
			const uint8_t *p = ax.base + ax.off[i];
			SaEntry e;
			const int st = sa_entry_of(p, p + ax.len[i], ax.enc, &e);
			if (st >= 0) {
				tags = 1;
				SaGeometry g;
				int32_t tid = -1;
				if (st == SA_MULTI) multi = 1;
				else if (st == SA_OK && e.mapq >= min_mapq && sa_geometry(e, &g) && (tid = sa_contig_find(T, e.rname, e.rname_len)) >= 0) {
					SaVirt v;
					v.tid = tid; v.pos = g.pos; v.lq = g.lq; v.left = g.left; v.right = g.right;
					v.n_keep = e.n_keep; v.cig_len = e.cigar_len; v.side = g.side; v.strand = e.strand; v.pad = 0; v.cig = e.cigar;
					virt[k] = v;
					made = 1;
				} else refused = 1;
			}
		}
		slots[k] = 1u + made;
	}
	tags = wave_sum(tags); multi = wave_sum(multi); refused = wave_sum(refused); made = wave_sum(made);
	if (lane_id() == 0) {
		if (tags) atomicAdd(stats + SA_N_TAGS, (unsigned long long)tags);
		if (multi) atomicAdd(stats + SA_N_MULTI, (unsigned long long)multi);
		if (refused) atomicAdd(stats + SA_N_REFUSED, (unsigned long long)refused);
		if (made) atomicAdd(stats + SA_N_VIRTUALS, (unsigned long long)made);
	}
}

// k_sr_measure writing at the candidate's slot; a virtual candidate behind it: no name bytes, no bases, its non-clip operations, its source's hash
__global__ __launch_bounds__(BLOCK) void k_sa_measure(DevBatch b, DevNames nm, const uint32_t *__restrict__ cand, int64_t m, const uint32_t *__restrict__ slot_at,
                                                      const uint32_t *__restrict__ slots, const SaVirt *__restrict__ virt, uint64_t hash_mask,
                                                      uint64_t *__restrict__ name_bytes, uint64_t *__restrict__ seq_bytes, uint64_t *__restrict__ cig_ops, uint64_t *__restrict__ hash)
{
	const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (k >= m) return;
	const int64_t i = cand[k];
	const uint32_t s = slot_at[k];
	const RecLine r = rec_load(b.rec, i);
	const char *p = name_addr(nm, i);
	uint64_t h = 1469598103934665603ull;
	uint32_t len = 0;
	while (len < 255) {
		const uint8_t ch = (uint8_t)p[len];
		if (!ch) break;
		h = (h ^ ch) * 1099511628211ull;
		++len;
	}
	h = (h ^ (uint64_t)(r.flag() & (int)SR_MATE)) * 1099511628211ull;
	const SrShape sh = sr_shape(r, b.cigar);
	name_bytes[s] = len + 1;
	seq_bytes[s] = sr_carries(r, sh) ? (uint64_t)(sh.R + 1) / 2 : 0;
	cig_ops[s] = sh.ops;
	hash[s] = h & hash_mask;
	if (slots[k] == 2u) {
		name_bytes[s + 1] = 0; seq_bytes[s + 1] = 0;
		cig_ops[s + 1] = virt[k].n_keep;
		hash[s + 1] = h & hash_mask;
	}
}

// one wavefront per candidate: k_sr_gather's line and copies at the candidate's slot; the virtual candidate's line behind it (lane 0 decodes the entry's
// CIGAR text: tens of bytes).  store_base: the store index of this batch's slot 0 - a virtual candidate's seq_off is its source's index.
__global__ __launch_bounds__(BLOCK) void k_sa_gather(DevBatch b, DevNames nm, const uint32_t *__restrict__ cand, int64_t m, const uint32_t *__restrict__ slot_at,
                                                     const uint32_t *__restrict__ slots, const SaVirt *__restrict__ virt, uint64_t rec_base, uint64_t store_base,
                                                     const uint64_t *__restrict__ name_at, const uint64_t *__restrict__ seq_at, const uint64_t *__restrict__ cig_at,
                                                     RtCand *__restrict__ out, char *__restrict__ names, uint8_t *__restrict__ seqs, uint32_t *__restrict__ cigs,
                                                     unsigned long long *__restrict__ stats)
{
	const int64_t k = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave_id();
	if (k >= m) return;
	const int lane = lane_id();
	const int64_t i = cand[k];
	const uint32_t s = slot_at[k];
	const RecLine r = rec_load(b.rec, i);
	const int nc = r.n_cigar();
	const SrShape sh = sr_shape(r, b.cigar);
	int ref_len = 0;
	for (int j = 0; j < nc; ++j) {
		const uint32_t x = r.op(b.cigar, j);
		const int op = (int)(x & 15u);
		if (op == C_M || op == C_D || op == C_EQ || op == C_N) ref_len += (int)(x >> 4);
	}
	RtCand c;
	c.tid = r.tid();
	const int R = sh.R > 0x3fffffff ? -1 : (int)sh.R;
	int clip = 0;
	if (sr_clip((int)(r.op(b.cigar, 0) & 15u))) {
		for (int j = 0; j < nc; ++j) { const uint32_t x = r.op(b.cigar, j); if (!sr_clip((int)(x & 15u))) break; clip += (int)(x >> 4); }
		c.side = '5'; c.left = clip; c.right = R - clip; c.pos = r.pos() + 1;
	} else {
		for (int j = nc - 1; j >= 0; --j) { const uint32_t x = r.op(b.cigar, j); if (!sr_clip((int)(x & 15u))) break; clip += (int)(x >> 4); }
		c.side = '3'; c.right = clip; c.left = R - clip; c.pos = r.pos() + ref_len;
	}
	const bool carries = sr_carries(r, sh);
	c.strand = (r.flag() & F_REV) ? '-' : '+';
	c.lq = R;
	c.rec = rec_base + (uint64_t)i;
	c.name_off = name_at[s]; c.seq_off = seq_at[s]; c.cig_off = cig_at[s];
	c.name_len = (uint32_t)(name_at[s + 1] - name_at[s] - 1);
	c.ncig = (uint16_t)(cig_at[s + 1] - cig_at[s]);
	c.pad = ((uint32_t)r.flag() & SR_MATE) | (carries ? SR_CARRIES : 0u) | (sh.has_h ? SR_HAS_H : 0u);
	if (lane == 0) {
		out[s] = c;
		if (sh.has_h) atomicAdd(stats + SR_N_HARD, 1ull);
		if (slots[k] == 2u) {
			const SaVirt v = virt[k];
			RtCand w;
			w.tid = v.tid; w.pos = v.pos; w.lq = v.lq; w.left = v.left; w.right = v.right;
			w.ncig = (uint16_t)v.n_keep; w.side = v.side; w.strand = v.strand;
			w.name_len = c.name_len; w.pad = (c.pad & SR_MATE) | SR_VIRTUAL;
			w.rec = c.rec; w.name_off = c.name_off; w.seq_off = store_base + s; w.cig_off = cig_at[s + 1];
			out[s + 1] = w;
			const uint8_t *q = v.cig, *const qe = v.cig + v.cig_len;
			uint64_t at = w.cig_off;
			while (q < qe) { const uint32_t x = sa_cigar_next(&q); if (!sr_clip((int)(x & 15u))) cigs[at++] = x; }
		}
	}
	const char *pn = name_addr(nm, i);
	for (uint32_t j = (uint32_t)lane; j < c.name_len; j += WAVE) names[c.name_off + j] = pn[j];
	if (lane == 0) names[c.name_off + c.name_len] = 0;
	const uint32_t sb = (uint32_t)(seq_at[s + 1] - seq_at[s]);
	if (sb) {
		const uint8_t *ps = b.seqqual + r.seq_off();
		for (uint32_t j = (uint32_t)lane; j < sb; j += WAVE) seqs[c.seq_off + j] = ps[j];
	}
	uint32_t done = 0;
	for (int j0 = 0; j0 < nc; j0 += WAVE) {
		const int j = j0 + lane;
		uint32_t x = 0; bool keep = false;
		if (j < nc) { x = r.op(b.cigar, j); keep = !sr_clip((int)(x & 15u)); }
		const uint64_t bal = __ballot(keep);
		if (keep) cigs[c.cig_off + done + (uint32_t)__popcll(bal & lanemask_lt())] = x;
		done += (uint32_t)__popcll(bal);
	}
}

// One lane per run of equal hashes, two phases.  Phase 1 is k_sr_pair over the run's real candidates: a virtual candidate is neither held nor looked at,
// so every outcome and count is what k_sr_pair gives with the virtual candidates absent - wherever the input was cut into batches.  Phase 2: a virtual
// candidate whose source has a partner or is one counts as redundant; else source (A, held) and virtual candidate (B, completing) pair when the strand /
// side test passes and R_A == R_B (unequal: dropped for the length).  The source carries the read, so a carrier is never wanting.
__global__ __launch_bounds__(BLOCK) void k_sa_pair(const uint64_t *__restrict__ hash, const uint32_t *__restrict__ order, int64_t n, const RtCand *__restrict__ cands,
                                                   const char *__restrict__ names, int32_t *__restrict__ held, int32_t *__restrict__ partner,
                                                   unsigned long long *__restrict__ stats, unsigned long long *__restrict__ sa_stats)
{
	const int64_t p0 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	uint32_t no_carrier = 0, length = 0, redundant = 0, from_sa = 0, sa_length = 0;
	if (p0 < n && (p0 == 0 || hash[p0 - 1] != hash[p0])) {
		int64_t end = p0 + 1;
		while (end < n && hash[end] == hash[p0]) ++end;
		bool any_virtual = false;
		for (int64_t p = p0; p < end; ++p) {
			const RtCand B = cands[order[p]];
			if (B.pad & SR_VIRTUAL) { held[p] = -1; any_virtual = true; continue; }
			int64_t h = -1;
			for (int64_t q = p - 1; q >= p0; --q) {
				const RtCand Q = cands[order[q]];
				if (!(Q.pad & SR_VIRTUAL) && (Q.pad & SR_MATE) == (B.pad & SR_MATE) && rt_same_name(Q, B, names)) { h = held[q]; break; }
			}
			if (h < 0) { held[p] = (int32_t)p; continue; }
			const RtCand A = cands[order[h]];
			bool pairs = (A.strand == B.strand && A.side != B.side) || (A.strand != B.strand && A.side == B.side);
			if (pairs && A.lq != B.lq) { pairs = false; ++length; }
			if (pairs && !((A.pad | B.pad) & SR_CARRIES)) { pairs = false; ++no_carrier; }
			if (pairs) { held[p] = -1; partner[order[p]] = (int32_t)order[h]; }
			else held[p] = (int32_t)h;
		}
		for (int64_t p = p0; any_virtual && p < end; ++p) {
			const uint32_t iv = order[p];
			const RtCand B = cands[iv];
			if (!(B.pad & SR_VIRTUAL)) continue;
			const uint32_t src = (uint32_t)B.seq_off;
			bool taken = partner[src] >= 0;
			for (int64_t q = p0; !taken && q < end; ++q) taken = order[q] != iv && partner[order[q]] == (int32_t)src;
			if (taken) { ++redundant; continue; }
			const RtCand A = cands[src];
			const bool pairs = (A.strand == B.strand && A.side != B.side) || (A.strand != B.strand && A.side == B.side);
			if (pairs && A.lq != B.lq) ++sa_length;
			else if (pairs) { partner[iv] = (int32_t)src; ++from_sa; }
		}
	}
	no_carrier = wave_sum(no_carrier); length = wave_sum(length); redundant = wave_sum(redundant); from_sa = wave_sum(from_sa); sa_length = wave_sum(sa_length);
	if (lane_id() == 0) {
		if (no_carrier) atomicAdd(stats + SR_N_NO_CARRIER, (unsigned long long)no_carrier);
		if (length) atomicAdd(stats + SR_N_LENGTH, (unsigned long long)length);
		if (redundant) atomicAdd(sa_stats + SA_N_REDUNDANT, (unsigned long long)redundant);
		if (from_sa) atomicAdd(sa_stats + SA_N_PAIRS, (unsigned long long)from_sa);
		if (sa_length) atomicAdd(sa_stats + SA_N_LENGTH, (unsigned long long)sa_length);
	}
}

} // namespace ssv
