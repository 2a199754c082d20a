// readthrough_kernels.h - `getsv -F`: junctions from read-through split alignments (FindJunction, process_bwasw.cpp:5-227).
// select (streaming: the 1-byte cigar_ends column, the record line only behind a passing pair of ends) -> gather (per candidate: its fields, non-clip
// CIGAR operations, packed bases and read name into context memory) -> at finish: sort by (name hash, record index), one lane per run of equal
// hashes runs the hold / pair / drop machine on full names -> pair events in the order of their completing record -> junction key, microhomology and
// the two seqs (ASCII, reverse-complemented by GetReverseComplementSeq's rule) per event.  Applying the events to the junction map stays on the host.
#pragma once

#include "common.h"
#include "clip_kernels.h"

namespace ssv {

// a read-through candidate: one kept record of the -F file
struct RtCand {
	int32_t tid, pos;      // pos: 5' side pos + 1, 3' side pos + reference length (GenerateCigar's l: M, D, =, N)
	int32_t lq, left, right;
	uint16_t ncig;         // operations in cig (S and H dropped, GenerateCigar)
	uint8_t side, strand;  // '5' / '3', '+' / '-'
	uint32_t name_len;
	uint32_t pad;
	uint64_t rec;          // record index in file order (all batches)
	uint64_t name_off, seq_off, cig_off;
};

__device__ __forceinline__ bool rt_ends_pass(uint8_t e)
{
	if (e == 0xff) return false; // no CIGAR (the reference reads cigar[-1]: skipped here)
	const int op1 = e & 15, op2 = e >> 4;
	if (op1 == C_H || op2 == C_H) return false;
	if (op1 == C_S && op2 == C_S) return false;
	if (op1 == C_M && op2 == C_M) return false;
	return true;
}

// per record: 1 when FindJunction keeps it (process_bwasw.cpp:47-51); the line is fetched only behind a passing pair of ends
__global__ __launch_bounds__(BLOCK) void k_rt_select(DevBatch b, int min_mapq, int n_targets, uint32_t *__restrict__ keep)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= b.n) return;
	uint32_t k = 0;
	if (rt_ends_pass(b.ends[i])) {
		const uint32_t fmx = reinterpret_cast<const uint32_t *>(b.rec + i)[2];
		const int flag = (int)(fmx & 0xffffu), mapq = (int)((fmx >> 16) & 0xffu);
		const int tid = b.tid[i];
		k = mapq >= min_mapq && !(flag & F_UNMAP) && !(flag & F_DUP) && tid >= 0 && tid < n_targets;
	}
	keep[i] = k;
}

__global__ __launch_bounds__(BLOCK) void k_rt_place(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ at, int64_t n, uint32_t *__restrict__ cand)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i < n && keep[i]) cand[at[i]] = (uint32_t)i;
}

// per candidate: bytes of its name (with the NUL), packed bases and operations; the 64-bit FNV-1a hash of its name (low hash_bits bits)
__global__ __launch_bounds__(BLOCK) void k_rt_measure(DevBatch b, DevNames nm, const uint32_t *__restrict__ cand, int64_t m, uint64_t hash_mask,
                                                      uint64_t *__restrict__ name_bytes, uint64_t *__restrict__ seq_bytes, uint64_t *__restrict__ cig_ops,
                                                      uint64_t *__restrict__ hash, uint32_t *__restrict__ bad)
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
	const int nc = r.n_cigar();
	uint32_t ops = 0;
	for (int j = 0; j < nc; ++j) { const int op = (int)(r.op(b.cigar, j) & 15u); ops += op != C_S && op != C_H; }
	const int lq = r.l_qseq() > 0 ? r.l_qseq() : 0;
	if (r.seq_off() == SSV_NO_SEQ && lq > 0) atomicOr(bad, 1u);
	name_bytes[k] = len + 1;
	seq_bytes[k] = (uint64_t)(lq + 1) / 2;
	cig_ops[k] = ops;
	hash[k] = h & hash_mask;
}

// one wavefront per candidate: its RtCand line and copies of its name, bases and non-clip operations
__global__ __launch_bounds__(BLOCK) void k_rt_gather(DevBatch b, DevNames nm, const uint32_t *__restrict__ cand, int64_t m, uint64_t rec_base,
                                                     const uint64_t *__restrict__ name_at, const uint64_t *__restrict__ seq_at, const uint64_t *__restrict__ cig_at,
                                                     RtCand *__restrict__ out, char *__restrict__ names, uint8_t *__restrict__ seqs, uint32_t *__restrict__ cigs)
{
	const int64_t k = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave_id();
	if (k >= m) return;
	const int lane = lane_id();
	const int64_t i = cand[k];
	const RecLine r = rec_load(b.rec, i);
	const int nc = r.n_cigar();
	const uint32_t first = r.head(0), last = r.op(b.cigar, nc - 1);
	const int lq = r.l_qseq() > 0 ? r.l_qseq() : 0;
	// GenerateCigar's reference length: M, D, = and N (not X)
	int ref_len = 0;
	for (int j = 0; j < nc; ++j) {
		const uint32_t x = r.op(b.cigar, j);
		const int op = (int)(x & 15u);
		if (op == C_M || op == C_D || op == C_EQ || op == C_N) ref_len += (int)(x >> 4);
	}
	RtCand c;
	c.tid = r.tid();
	if ((first & 15u) == C_S) { // 5' clipped (process_bwasw.cpp:54-60); lengths clamped to the read
		c.side = '5';
		c.left = min((int)(first >> 4), lq);
		c.right = lq - c.left;
		c.pos = r.pos() + 1;
	} else {                     // everything else through the 3' branch (:61-67), records without S included
		c.side = '3';
		c.right = min((int)(last >> 4), lq);
		c.left = lq - c.right;
		c.pos = r.pos() + ref_len;
	}
	c.strand = (r.flag() & F_REV) ? '-' : '+';
	c.lq = lq;
	c.rec = rec_base + (uint64_t)i;
	c.name_off = name_at[k]; c.seq_off = seq_at[k]; c.cig_off = cig_at[k];
	c.name_len = (uint32_t)(name_at[k + 1] - name_at[k] - 1);
	c.ncig = (uint16_t)(cig_at[k + 1] - cig_at[k]);
	c.pad = 0;
	if (lane == 0) out[k] = c;
	const char *pn = name_addr(nm, i);
	for (uint32_t j = (uint32_t)lane; j < c.name_len; j += WAVE) names[c.name_off + j] = pn[j];
	if (lane == 0) names[c.name_off + c.name_len] = 0;
	const uint32_t sb = (uint32_t)(seq_at[k + 1] - seq_at[k]);
	const uint8_t *ps = b.seqqual + r.seq_off();
	for (uint32_t j = (uint32_t)lane; j < sb; j += WAVE) seqs[c.seq_off + j] = ps[j];
	// non-clip operations in order: each lane counts the kept operations before its own through a ballot per round of 64
	uint32_t done = 0;
	for (int j0 = 0; j0 < nc; j0 += WAVE) {
		const int j = j0 + lane;
		uint32_t x = 0; bool keep = false;
		if (j < nc) { x = r.op(b.cigar, j); const int op = (int)(x & 15u); keep = op != C_S && op != C_H; }
		const uint64_t bal = __ballot(keep);
		if (keep) cigs[c.cig_off + done + (uint32_t)__popcll(bal & lanemask_lt())] = x;
		done += (uint32_t)__popcll(bal);
	}
}

__device__ __forceinline__ bool rt_same_name(const RtCand &a, const RtCand &b, const char *names)
{
	if (a.name_len != b.name_len) return false;
	for (uint32_t j = 0; j < a.name_len; ++j) if (names[a.name_off + j] != names[b.name_off + j]) return false;
	return true;
}

// One lane per run of equal hashes (sorted: (hash, record index)), the reference's std::map<string, Alignment> over the run (process_bwasw.cpp:84-224):
// a record whose name is not held becomes the held one; a held A and a new B pair when (same strand, different sides) or (opposite strands, same side) -
// the pair releases the name - else B is dropped.  Names are compared in full, so a run holding several names (a hash collision) pairs exactly.
// held[p]: sorted position of the record held for p's name after p's step, -1 none.  partner[candidate] = the held record it completes, -1 none.
// Cost: one lane walks its run with a backward scan per record, O(run^2) name compares.  With a 64-bit hash a run is one name's records - 1 to 4 of
// them in a bwasw file - plus a rare collision; a file in which thousands of records share ONE name (names stripped to "*", say) serialises that name
// into one long lane - correct, but slow in proportion to the square of its count.
__global__ __launch_bounds__(BLOCK) void k_rt_pair(const uint64_t *__restrict__ hash, const uint32_t *__restrict__ order, int64_t n, const RtCand *__restrict__ cands,
                                                   const char *__restrict__ names, int32_t *__restrict__ held, int32_t *__restrict__ partner)
{
	const int64_t p0 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (p0 >= n || (p0 > 0 && hash[p0 - 1] == hash[p0])) return;
	int64_t end = p0 + 1;
	while (end < n && hash[end] == hash[p0]) ++end;
	for (int64_t p = p0; p < end; ++p) {
		const RtCand B = cands[order[p]];
		int64_t h = -1;
		for (int64_t q = p - 1; q >= p0; --q) // the latest earlier record of the same name carries the name's state
			if (rt_same_name(cands[order[q]], B, names)) { h = held[q]; break; }
		if (h < 0) { held[p] = (int32_t)p; continue; }
		const RtCand A = cands[order[h]];
		const bool pairs = (A.strand == B.strand && A.side != B.side) || (A.strand != B.strand && A.side == B.side);
		if (pairs) { held[p] = -1; partner[order[p]] = (int32_t)order[h]; }
		else held[p] = (int32_t)h;
	}
}

__global__ __launch_bounds__(BLOCK) void k_rt_flag_pairs(const int32_t *__restrict__ partner, int64_t n, uint32_t *__restrict__ flag)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i < n) flag[i] = partner[i] >= 0;
}

// a seq of a junction: bases [begin, begin + len) of a candidate, reversed and complemented when rc
struct RtSlice { uint32_t cand; int32_t begin, len, rc; };

// the ABI's result line (seeksv_hip.h ssv_rt_pair), built on the device
struct RtPairOut {
	int32_t up_tid, up_pos, down_tid, down_pos;
	int8_t up_strand, down_strand; int16_t kind;
	int32_t microhomology;
	int32_t up_left_clipped, up_right_clipped, down_left_clipped, down_right_clipped;
	int32_t up_len, down_len;
	int32_t up_cig_n, down_cig_n;
	int32_t up_cig_edit, down_cig_edit;
	uint64_t seq_off, cig_off;
	int64_t first_record, second_record;
};

// per pair event (process_bwasw.cpp:94-197): up / down, key, microhomology, the two seqs as slices, the CIGAR sources and their edits.
// rank[tid]: the contig's place in byte-wise name order (make_pair(chr, pos) < compares names as strings).
__global__ __launch_bounds__(BLOCK) void k_rt_keys(const uint32_t *__restrict__ ev_b, const int32_t *__restrict__ partner, int64_t m, const RtCand *__restrict__ cands,
                                                   const int32_t *__restrict__ rank, RtPairOut *__restrict__ out, RtSlice *__restrict__ slices,
                                                   uint32_t *__restrict__ cig_src, uint64_t *__restrict__ seq_bytes, uint64_t *__restrict__ cig_ops)
{
	const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (e >= m) return;
	const uint32_t ib = ev_b[e], ia = (uint32_t)partner[ib];
	const RtCand A = cands[ia], B = cands[ib]; // A held (earlier), B completes the pair
	uint32_t iu, id;
	RtPairOut o;
	RtSlice su, sd;
	uint32_t cu, cd; // CIGAR sources of the up and down seq infos
	int mh = 0;
	o.up_left_clipped = o.up_right_clipped = o.down_left_clipped = o.down_right_clipped = 0;
	o.up_cig_edit = o.down_cig_edit = 0;
	if (A.strand == B.strand) {
		if (A.side == '5') { iu = ib; id = ia; } else { iu = ia; id = ib; }
		const RtCand &U = cands[iu], &D = cands[id];
		su = RtSlice{id, 0, D.left, 0}; sd = RtSlice{id, D.left, D.right, 0};
		cu = iu; cd = id;
		if (U.left >= D.left) {
			mh = U.left - D.left; o.kind = 0;
			o.up_tid = U.tid; o.up_pos = U.pos - mh; o.up_strand = '+'; o.down_tid = D.tid; o.down_pos = D.pos; o.down_strand = '+';
			o.up_cig_edit = 1;
		} else {
			o.kind = 1;
			o.up_tid = U.tid; o.up_pos = U.pos; o.up_strand = '+'; o.down_tid = D.tid; o.down_pos = D.pos; o.down_strand = '+';
			o.up_right_clipped = D.left - U.left;
		}
	} else {
		const int ra = rank[A.tid], rb = rank[B.tid];
		if (ra < rb || (ra == rb && A.pos < B.pos)) { iu = ia; id = ib; } else { iu = ib; id = ia; }
		const RtCand &U = cands[iu], &D = cands[id];
		cu = iu; cd = id;
		if (B.side == '5') {
			if (U.right >= D.left) {
				mh = U.right - D.left; o.kind = 2;
				o.up_tid = U.tid; o.up_pos = U.pos; o.up_strand = '-'; o.down_tid = D.tid; o.down_pos = D.pos + mh; o.down_strand = '+';
				su = RtSlice{iu, U.left, U.right, 1}; sd = RtSlice{iu, 0, U.left, 1};
				o.down_cig_edit = 2;
			} else {
				o.kind = 3;
				o.up_tid = U.tid; o.up_pos = U.pos; o.up_strand = '-'; o.down_tid = D.tid; o.down_pos = D.pos; o.down_strand = '+';
				su = RtSlice{id, 0, D.left, 0}; sd = RtSlice{id, D.left, D.right, 0};
				o.up_right_clipped = D.left - U.right;
			}
		} else {
			if (U.left >= D.right) {
				mh = U.left - D.right; o.kind = 4;
				o.up_tid = U.tid; o.up_pos = U.pos - mh; o.up_strand = '+'; o.down_tid = D.tid; o.down_pos = D.pos; o.down_strand = '-';
				su = RtSlice{id, D.left, D.right, 1}; sd = RtSlice{id, 0, D.left, 1};
				o.up_cig_edit = 1;
			} else {
				o.kind = 5;
				o.up_tid = U.tid; o.up_pos = U.pos; o.up_strand = '+'; o.down_tid = D.tid; o.down_pos = D.pos; o.down_strand = '-';
				su = RtSlice{iu, 0, U.left, 0}; sd = RtSlice{iu, U.left, U.right, 0};
				o.down_left_clipped = D.right - U.left;
			}
		}
	}
	o.microhomology = mh;
	o.up_len = su.len; o.down_len = sd.len;
	o.up_cig_n = cands[cu].ncig; o.down_cig_n = cands[cd].ncig;
	o.seq_off = 0; o.cig_off = 0;
	o.first_record = (int64_t)A.rec; o.second_record = (int64_t)B.rec;
	out[e] = o;
	slices[2 * e] = su; slices[2 * e + 1] = sd;
	cig_src[2 * e] = cu; cig_src[2 * e + 1] = cd;
	seq_bytes[e] = (uint64_t)(su.len + sd.len);
	cig_ops[e] = (uint64_t)o.up_cig_n + (uint64_t)o.down_cig_n;
}

// GetReverseComplementSeq (clip_reads.cpp:414-466): only A C G T N are complemented (the bases here are upper case); '=' and IUPAC codes stay
__device__ __forceinline__ char rt_comp(char ch)
{
	switch (ch) { case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C'; default: return ch; }
}

__constant__ char RT_NT16[17] = "=ACMGRSVTWYHKDBN";

// one wavefront per event: the two seqs in ASCII (bam_nt16_rev_table, upper case) and the operations of the two CIGAR sources
__global__ __launch_bounds__(BLOCK) void k_rt_emit(int64_t m, const RtCand *__restrict__ cands, const uint8_t *__restrict__ bases, const uint32_t *__restrict__ cigs,
                                                   const RtSlice *__restrict__ slices, const uint32_t *__restrict__ cig_src, const uint64_t *__restrict__ seq_at,
                                                   const uint64_t *__restrict__ cig_at, RtPairOut *__restrict__ out, char *__restrict__ seq_out, uint32_t *__restrict__ cig_out)
{
	const int64_t e = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave_id();
	if (e >= m) return;
	const int lane = lane_id();
	uint64_t so = seq_at[e], co = cig_at[e];
	if (lane == 0) { out[e].seq_off = so; out[e].cig_off = co; }
	for (int s = 0; s < 2; ++s) {
		const RtSlice sl = slices[2 * e + s];
		const uint8_t *b = bases + cands[sl.cand].seq_off;
		for (int j = lane; j < sl.len; j += WAVE) {
			const int k = sl.rc ? sl.begin + sl.len - 1 - j : sl.begin + j;
			const char ch = RT_NT16[(b[k >> 1] >> ((~k & 1) << 2)) & 15];
			seq_out[so + (uint64_t)j] = sl.rc ? rt_comp(ch) : ch;
		}
		so += (uint64_t)sl.len;
		const RtCand &cc = cands[cig_src[2 * e + s]];
		for (int j = lane; j < (int)cc.ncig; j += WAVE) cig_out[co + (uint64_t)j] = cigs[cc.cig_off + (uint64_t)j];
		co += cc.ncig;
	}
}

} // namespace ssv
