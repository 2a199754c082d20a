// splitread_kernels.h - `seeksv run -A`: junctions from the supplementary alignments of the original itself (the rule: include/seeksv_hip.h at
// ssv_rt_begin_original).  The stages of readthrough_kernels.h with a selection and a key of their own: select (streaming over the 1-byte
// cigar_ends column: exactly one end S or H; the record line only behind a passing pair of ends) -> measure (the name hash takes one more byte, flag & 0xC0;
// bases are counted only for a record that carries the read) -> gather (clip runs and R from the CIGAR alone; mate bits, `carries` and `has H` in RtCand::pad)
// -> at finish: k_sr_pair (the hold / pair / drop machine keyed by (name, mate bits), with equal R and one carrier demanded of a pair) -> k_rt_keys, as it is ->
// k_sr_borrow (a seq whose source record does not carry the read is read from the partner instead) -> k_rt_emit, as it is.  Streaming integer and byte work:
// no LDS, plain vector stores, and one atomic per wavefront at the most - for the statistics.
#pragma once

#include "readthrough_kernels.h"

namespace ssv {

// RtCand::pad of a candidate of this mode (the -F mode writes 0)
enum : uint32_t { SR_CARRIES = 1u, SR_HAS_H = 2u, SR_MATE = 0xC0u };
// the statistics, in device memory: one 64-bit counter each
enum : int { SR_N_HARD = 0, SR_N_BORROWED = 1, SR_N_NO_CARRIER = 2, SR_N_LENGTH = 3, SR_N_STATS = 4 };

__device__ __forceinline__ bool sr_clip(int op) { return op == C_S || op == C_H; }

// exactly one of the two ends is S or H (a CIGAR of one operation has both ends alike: never)
__device__ __forceinline__ bool sr_ends_pass(uint8_t e)
{
	if (e == 0xff) return false; // no CIGAR
	return sr_clip(e & 15) != sr_clip(e >> 4);
}

// per record: 1 when it takes part.  The flags are the input's: this runs on the decoded chunk, in front of every mark.
__global__ __launch_bounds__(BLOCK) void k_sr_select(DevBatch b, int min_mapq, int n_targets, uint32_t *__restrict__ keep)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= b.n) return;
	uint32_t k = 0;
	if (sr_ends_pass(b.ends[i])) {
		const uint32_t fmx = reinterpret_cast<const uint32_t *>(b.rec + i)[2];
		const int flag = (int)(fmx & 0xffffu), mapq = (int)((fmx >> 16) & 0xffu);
		const int tid = b.tid[i];
		k = mapq >= min_mapq && !(flag & (F_UNMAP | F_SECONDARY | F_DUP)) && tid >= 0 && tid < n_targets;
	}
	keep[i] = k;
}

// R (M I S = X H; 64 bits: 65535 operations of up to 2^28 bases), whether an H is among the operations, and the non-clip operations of a record
struct SrShape { int64_t R; bool has_h; uint32_t ops; };
__device__ __forceinline__ SrShape sr_shape(const RecLine &r, const uint32_t *cigar)
{
	SrShape s{0, false, 0};
	const int nc = r.n_cigar();
	for (int j = 0; j < nc; ++j) {
		const uint32_t x = r.op(cigar, j);
		const int op = (int)(x & 15u);
		if (op == C_M || op == C_I || op == C_S || op == C_EQ || op == C_X || op == C_H) s.R += (int64_t)(x >> 4);
		s.has_h |= op == C_H;
		s.ops += !sr_clip(op);
	}
	return s;
}
__device__ __forceinline__ bool sr_carries(const RecLine &r, const SrShape &s) { return !s.has_h && r.seq_off() != SSV_NO_SEQ && (int64_t)r.l_qseq() == s.R; }

// per candidate: bytes of its name (with the NUL), of its packed bases (none unless it carries the read) and its operations; the 64-bit FNV-1a hash of its
// name and of one more byte, flag & 0xC0 (low hash_bits bits)
__global__ __launch_bounds__(BLOCK) void k_sr_measure(DevBatch b, DevNames nm, const uint32_t *__restrict__ cand, int64_t m, uint64_t hash_mask,
                                                      uint64_t *__restrict__ name_bytes, uint64_t *__restrict__ seq_bytes, uint64_t *__restrict__ cig_ops,
                                                      uint64_t *__restrict__ hash)
{
	const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (k >= m) return;
	const int64_t i = cand[k];
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
	const SrShape s = sr_shape(r, b.cigar);
	name_bytes[k] = len + 1;
	seq_bytes[k] = sr_carries(r, s) ? (uint64_t)(s.R + 1) / 2 : 0; // (a carrier's R is its l_qseq)
	cig_ops[k] = s.ops;
	hash[k] = h & hash_mask;
}

// one wavefront per candidate: its RtCand line and copies of its name, bases (when it carries the read) and non-clip operations
__global__ __launch_bounds__(BLOCK) void k_sr_gather(DevBatch b, DevNames nm, const uint32_t *__restrict__ cand, int64_t m, uint64_t rec_base,
                                                     const uint64_t *__restrict__ name_at, const uint64_t *__restrict__ seq_at, const uint64_t *__restrict__ cig_at,
                                                     RtCand *__restrict__ out, char *__restrict__ names, uint8_t *__restrict__ seqs, uint32_t *__restrict__ cigs,
                                                     unsigned long long *__restrict__ stats)
{
	const int64_t k = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave_id();
	if (k >= m) return;
	const int lane = lane_id();
	const int64_t i = cand[k];
	const RecLine r = rec_load(b.rec, i);
	const int nc = r.n_cigar();
	const SrShape s = sr_shape(r, b.cigar);
	int ref_len = 0; // GenerateCigar's reference length: M, D, = and N (not X)
	for (int j = 0; j < nc; ++j) {
		const uint32_t x = r.op(b.cigar, j);
		const int op = (int)(x & 15u);
		if (op == C_M || op == C_D || op == C_EQ || op == C_N) ref_len += (int)(x >> 4);
	}
	RtCand c;
	c.tid = r.tid();
	// R beyond 2^30 (no read is that long; only H can say so): lq = -1, which no carrier's R equals - such a record never pairs, its lengths are never read
	const int R = s.R > 0x3fffffff ? -1 : (int)s.R;
	int clip = 0;
	if (sr_clip((int)(r.op(b.cigar, 0) & 15u))) { // 5' clipped: the run of S / H at the front
		for (int j = 0; j < nc; ++j) { const uint32_t x = r.op(b.cigar, j); if (!sr_clip((int)(x & 15u))) break; clip += (int)(x >> 4); }
		c.side = '5'; c.left = clip; c.right = R - clip; c.pos = r.pos() + 1;
	} else {                                      // 3' clipped: the run at the back
		for (int j = nc - 1; j >= 0; --j) { const uint32_t x = r.op(b.cigar, j); if (!sr_clip((int)(x & 15u))) break; clip += (int)(x >> 4); }
		c.side = '3'; c.right = clip; c.left = R - clip; c.pos = r.pos() + ref_len;
	}
	const bool carries = sr_carries(r, s);
	c.strand = (r.flag() & F_REV) ? '-' : '+';
	c.lq = R;
	c.rec = rec_base + (uint64_t)i;
	c.name_off = name_at[k]; c.seq_off = seq_at[k]; c.cig_off = cig_at[k];
	c.name_len = (uint32_t)(name_at[k + 1] - name_at[k] - 1);
	c.ncig = (uint16_t)(cig_at[k + 1] - cig_at[k]);
	c.pad = ((uint32_t)r.flag() & SR_MATE) | (carries ? SR_CARRIES : 0u) | (s.has_h ? SR_HAS_H : 0u);
	if (lane == 0) {
		out[k] = c;
		if (s.has_h) atomicAdd(stats + SR_N_HARD, 1ull);
	}
	const char *pn = name_addr(nm, i);
	for (uint32_t j = (uint32_t)lane; j < c.name_len; j += WAVE) names[c.name_off + j] = pn[j];
	if (lane == 0) names[c.name_off + c.name_len] = 0;
	const uint32_t sb = (uint32_t)(seq_at[k + 1] - seq_at[k]); // (0 for a record that does not carry the read: seq_off may be SSV_NO_SEQ)
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

// k_rt_pair with the key (name, mate bits) and two more conditions on a pair: equal R, and a carrier among the two.  A new record that fails any of the three
// is dropped and the held one stays.  Dropped for the lengths / for want of a carrier are counted (in that order, behind the geometry): every lane sums its
// run's, the wavefront's sum goes out in one atomic per counter.
__global__ __launch_bounds__(BLOCK) void k_sr_pair(const uint64_t *__restrict__ hash, const uint32_t *__restrict__ order, int64_t n, const RtCand *__restrict__ cands,
                                                   const char *__restrict__ names, int32_t *__restrict__ held, int32_t *__restrict__ partner,
                                                   unsigned long long *__restrict__ stats)
{
	const int64_t p0 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	uint32_t no_carrier = 0, length = 0;
	if (p0 < n && (p0 == 0 || hash[p0 - 1] != hash[p0])) {
		int64_t end = p0 + 1;
		while (end < n && hash[end] == hash[p0]) ++end;
		for (int64_t p = p0; p < end; ++p) {
			const RtCand B = cands[order[p]];
			int64_t h = -1;
			for (int64_t q = p - 1; q >= p0; --q) { // the latest earlier record of the same key carries the key's state
				const RtCand Q = cands[order[q]];
				if ((Q.pad & SR_MATE) == (B.pad & SR_MATE) && rt_same_name(Q, B, names)) { h = held[q]; break; }
			}
			if (h < 0) { held[p] = (int32_t)p; continue; }
			const RtCand A = cands[order[h]];
			bool pairs = (A.strand == B.strand && A.side != B.side) || (A.strand != B.strand && A.side == B.side);
			if (pairs && A.lq != B.lq) { pairs = false; ++length; }
			if (pairs && !((A.pad | B.pad) & SR_CARRIES)) { pairs = false; ++no_carrier; }
			if (pairs) { held[p] = -1; partner[order[p]] = (int32_t)order[h]; }
			else held[p] = (int32_t)h;
		}
	}
	no_carrier = wave_sum(no_carrier); length = wave_sum(length);
	if (lane_id() == 0) {
		if (no_carrier) atomicAdd(stats + SR_N_NO_CARRIER, (unsigned long long)no_carrier);
		if (length) atomicAdd(stats + SR_N_LENGTH, (unsigned long long)length);
	}
}

// behind k_rt_keys, per pair event: a seq that k_rt_keys' case analysis reads from a record that does not carry the read is read from its partner - the
// same bases: (begin, len, rc) on the same strand, (R - begin - len, len, !rc) on opposite strands.  The CIGAR sources stay.
__global__ __launch_bounds__(BLOCK) void k_sr_borrow(const uint32_t *__restrict__ ev_b, const int32_t *__restrict__ partner, int64_t m, const RtCand *__restrict__ cands,
                                                     RtSlice *__restrict__ slices, unsigned long long *__restrict__ stats)
{
	const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	uint32_t borrowed = 0;
	if (e < m) {
		const uint32_t ib = ev_b[e], ia = (uint32_t)partner[ib];
		const bool opposite = cands[ia].strand != cands[ib].strand;
		const int R = cands[ib].lq;
		for (int s = 0; s < 2; ++s) {
			RtSlice sl = slices[2 * e + s];
			if (cands[sl.cand].pad & SR_CARRIES) continue;
			sl.cand = sl.cand == ia ? ib : ia;
			if (opposite) { sl.begin = R - sl.begin - sl.len; sl.rc = !sl.rc; }
			slices[2 * e + s] = sl;
			borrowed = 1;
		}
	}
	borrowed = wave_sum(borrowed);
	if (lane_id() == 0 && borrowed) atomicAdd(stats + SR_N_BORROWED, (unsigned long long)borrowed);
}

} // namespace ssv
