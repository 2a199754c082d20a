// pairdup_kernels.h - `run -D`: duplicate read pairs by the unclipped 5' ends of both reads, in any record order (the rule: include/seeksv_hip.h, ssv_pairdup_mark).
// retain (per batch): sizes -> scans -> rows (16 lanes a record: quality sum by all, the CIGAR walk by the first, the name hash by the second) + dup_kernels.h's gather.
// mark (all batches as one sequence, a record's index in it is g): rows that take part, compacted with g -> radix_sort.h by name hash (stable: g goes up inside
// a name group) -> join (one lane a row: is my name group a pair - neighbours by shuffle, across wavefronts by a second look-up) -> pairs (one lane a pair: the
// three key words and the score) -> four stable sorts: by (score down, g up), then by the key words from the least significant one - the first pair of every run
// of equal keys is then its keeper, whatever the run's length: no pass is quadratic -> pick + scatter (one lane a pair: 0x400 into the lines of both mates).
// Every flag has one writer, a plain 16-bit store.  The only atomics are two 64-bit counts, one add a wavefront.
#pragma once

#include "common.h"
#include "clip_kernels.h"
#include "dup_kernels.h"
#include "retained.h"

namespace ssv {

// one row per record, behind the other parts of a retained batch's slab (all zero: the record takes no part)
struct PdRow { uint64_t name_hash; int64_t u; uint32_t score; uint32_t kind; };
static_assert(sizeof(PdRow) == 24, "a row is 24 bytes");

__device__ __forceinline__ bool pd_takes_part(int flag, int tid, int mtid, int n_cigar) { return dup_takes_part(flag, tid, mtid) && n_cigar > 0; }
__device__ __forceinline__ bool pd_soft_hard(uint32_t op) { return (op & 15u) == (uint32_t)C_S || (op & 15u) == (uint32_t)C_H; }

// ---- retain ----
// what record i takes in the retained batch: all operations; bases + qualities when it has them and its first or last operation is S
__global__ __launch_bounds__(BLOCK) void k_pd_sizes(DevBatch b, uint32_t *__restrict__ cig_n, uint32_t *__restrict__ seq_b)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= b.n) return;
	const uint4 *p = reinterpret_cast<const uint4 *>(b.rec + i);
	const uint4 q1 = p[1], q3 = p[3];
	const int lq = (int)q1.x > 0 ? (int)q1.x : 0;
	const bool has = ((uint64_t)q3.z | ((uint64_t)q3.w << 32)) != SSV_NO_SEQ;
	const bool clipped = ends_clipped(b.ends[i]);
	cig_n[i] = (uint32_t)b.n_cigar[i];
	seq_b[i] = has && clipped ? seq_bytes(lq) : 0u;
}

// 16 lanes per record: the row.  *bad = 1: a record that takes part came without its qualities.
__global__ __launch_bounds__(BLOCK) void k_pd_rows(DevBatch b, DevNames nm, uint64_t mask, PdRow *__restrict__ rows, uint32_t *__restrict__ bad)
{
	const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	const int64_t i = t / DUP_SUB;
	const int sub = (int)(t & (DUP_SUB - 1));
	const bool in = i < b.n;
	RecLine r{};
	bool part = false;
	if (in) {
		r = rec_load(b.rec, i);
		part = pd_takes_part(r.flag(), r.tid(), r.mtid(), r.n_cigar());
	}
	const uint32_t score = dup_score(b.seqqual, part ? r.seq_off() : SSV_NO_SEQ, part ? r.l_qseq() : 0, sub); // (every lane of the wavefront takes part in its shuffles)
	int64_t u = 0;
	if (part && sub == 0) {
		if (r.seq_off() == SSV_NO_SEQ && r.l_qseq() > 0) *bad = 1u;
		const int nc = r.n_cigar();
		int64_t lead = 0, trail = 0, span = 0;
		bool leading = true;
		for (int k = 0; k < nc; ++k) {
			const uint32_t x = r.op(b.cigar, k);
			const int op = (int)(x & 15u);
			const int64_t len = (int64_t)(x >> 4);
			if (pd_soft_hard(x)) { trail += len; if (leading) lead += len; }
			else {
				trail = 0; leading = false;
				if (op == C_M || op == C_D || op == C_N || op == C_EQ || op == C_X) span += len;
			}
		}
		u = (r.flag() & F_REV) ? (int64_t)r.pos() + span - 1 + trail : (int64_t)r.pos() - lead;
	}
	uint64_t h = 0;
	if (part && sub == 1) {
		const char *name = nm.base + nm.off[i] + nm.bias;
		h = FNV_OFFSET;
		for (int len = 0; len < 255; ++len) {
			const uint8_t ch = (uint8_t)name[len];
			if (!ch) break;
			h = (h ^ ch) * FNV_PRIME;
		}
		h &= mask;
	}
	const uint32_t hlo = __shfl((uint32_t)h, 1, DUP_SUB), hhi = __shfl((uint32_t)(h >> 32), 1, DUP_SUB);
	if (!in || sub != 0) return;
	PdRow row{0ull, 0ll, 0u, 0u};
	if (part) row = PdRow{(uint64_t)hlo | ((uint64_t)hhi << 32), u, score, 1u};
	rows[i] = row;
}

// ---- mark ----
// one batch of the call: where its records start in the sequence of all of them, its lines (the flags are written there) and its rows
struct PdSrc { int64_t start; ssv_record *rec; const PdRow *rows; };

__global__ __launch_bounds__(BLOCK) void k_pd_part(const PdSrc *__restrict__ src, int n_src, int64_t n, uint32_t *__restrict__ part)
{
	const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (g >= n) return;
	const int k = src_find(src, n_src, g);
	part[g] = src[k].rows[g - src[k].start].kind != 0u;
}

__global__ __launch_bounds__(BLOCK) void k_pd_compact(const PdSrc *__restrict__ src, int n_src, int64_t n, const uint32_t *__restrict__ part, const uint32_t *__restrict__ at,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
	const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (g >= n || !part[g]) return;
	const int k = src_find(src, n_src, g);
	keys[at[g]] = src[k].rows[g - src[k].start].name_hash;
	vals[at[g]] = (uint32_t)g;
}

// the fields of a record the pair rule reads: the first two quarters of its line
struct PdFields { int tid, pos, flag, mtid, mpos; };
__device__ __forceinline__ PdFields pd_fields(const PdSrc *__restrict__ src, int n_src, int64_t g, const PdRow **row)
{
	const int k = src_find(src, n_src, g);
	const int64_t j = g - src[k].start;
	const uint4 *p = reinterpret_cast<const uint4 *>(src[k].rec + j);
	const uint4 a = p[0], b = p[1];
	if (row) *row = src[k].rows + j;
	return PdFields{(int)a.x, (int)a.y, (int)(a.z & 0xffffu), (int)b.y, (int)b.z};
}

__device__ __forceinline__ uint64_t pd_shfl_up64(uint64_t v, int d) { return (uint64_t)__shfl_up((uint32_t)v, d, 64) | ((uint64_t)__shfl_up((uint32_t)(v >> 32), d, 64) << 32); }
__device__ __forceinline__ uint64_t pd_shfl_down64(uint64_t v, int d) { return (uint64_t)__shfl_down((uint32_t)v, d, 64) | ((uint64_t)__shfl_down((uint32_t)(v >> 32), d, 64) << 32); }

// One lane per row in name-hash order: first[k] = 1 when row k starts a name group of exactly two records that are mates by the rule.  The neighbours' hashes
// come by shuffle; the lanes at a wavefront's edges look theirs up.
__global__ __launch_bounds__(BLOCK) void k_pd_join(const PdSrc *__restrict__ src, int n_src, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, int64_t m,
                                                   uint32_t *__restrict__ first)
{
	const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	const int lane = lane_id();
	const bool in = k < m;
	const uint64_t h = in ? keys[k] : 0ull;
	uint64_t hp = pd_shfl_up64(h, 1), hn1 = pd_shfl_down64(h, 1), hn2 = pd_shfl_down64(h, 2);
	if (lane == 0 && in && k > 0) hp = keys[k - 1];
	if (lane >= 63 && k + 1 < m) hn1 = keys[k + 1];
	if (lane >= 62 && k + 2 < m) hn2 = keys[k + 2];
	if (!in) return;
	const bool has_prev = k > 0 && hp == h, has_n1 = k + 1 < m && hn1 == h, has_n2 = k + 2 < m && hn2 == h;
	bool ok = !has_prev && has_n1 && !has_n2;
	if (ok) {
		const PdFields x = pd_fields(src, n_src, vals[k], nullptr), y = pd_fields(src, n_src, vals[k + 1], nullptr);
		ok = ((x.flag & F_READ1) != 0) != ((y.flag & F_READ1) != 0) && x.mtid == y.tid && x.mpos == y.pos && y.mtid == x.tid && y.mpos == x.pos &&
		     ((x.flag & F_MREV) != 0) == ((y.flag & F_REV) != 0) && ((y.flag & F_MREV) != 0) == ((x.flag & F_REV) != 0);
	}
	first[k] = ok;
}

// One lane per pair: a = the record with the smaller (tid, u, reverse), on a tie the one with 0x40.  The key as three words - w1 = tid_a << 33 | tid_b << 2 |
// rev_a << 1 | rev_b, w2 / w3 = u_a / u_b with the sign bit turned (unsigned order = signed order) - and the word of the first sort: the score's complement
// above the pair's smaller g (the row that comes first in its name group: the name sort is stable).
__global__ __launch_bounds__(BLOCK) void k_pd_pairs(const PdSrc *__restrict__ src, int n_src, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ first,
                                                    const uint32_t *__restrict__ pat, int64_t m, uint64_t *__restrict__ w0, uint32_t *__restrict__ idx, uint64_t *__restrict__ w1,
                                                    uint64_t *__restrict__ w2, uint64_t *__restrict__ w3, uint32_t *__restrict__ g1, uint32_t *__restrict__ g2)
{
	const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (k >= m || !first[k]) return;
	const uint32_t p = pat[k], gx = vals[k], gy = vals[k + 1];
	const PdRow *rx, *ry;
	const PdFields x = pd_fields(src, n_src, gx, &rx), y = pd_fields(src, n_src, gy, &ry);
	const int64_t ux = rx->u, uy = ry->u;
	const int vx = (x.flag & F_REV) ? 1 : 0, vy = (y.flag & F_REV) ? 1 : 0;
	bool x_first;
	if (x.tid != y.tid) x_first = x.tid < y.tid;
	else if (ux != uy) x_first = ux < uy;
	else if (vx != vy) x_first = vx < vy;
	else x_first = (x.flag & F_READ1) != 0;
	const uint64_t ta = (uint64_t)(uint32_t)(x_first ? x.tid : y.tid), tb = (uint64_t)(uint32_t)(x_first ? y.tid : x.tid);
	const uint64_t va = (uint64_t)(x_first ? vx : vy), vb = (uint64_t)(x_first ? vy : vx);
	const uint64_t sign = 1ull << 63;
	w1[p] = (ta << 33) | (tb << 2) | (va << 1) | vb;
	w2[p] = (uint64_t)(x_first ? ux : uy) ^ sign;
	w3[p] = (uint64_t)(x_first ? uy : ux) ^ sign;
	w0[p] = ((uint64_t)~(rx->score + ry->score) << 32) | (uint64_t)(gx < gy ? gx : gy);
	idx[p] = p;
	g1[p] = gx; g2[p] = gy;
}

// the next sort's keys: word[perm[k]]
__global__ __launch_bounds__(BLOCK) void k_pd_load_keys(const uint64_t *__restrict__ word, const uint32_t *__restrict__ perm, int64_t n, uint64_t *__restrict__ keys)
{
	const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (k < n) keys[k] = word[perm[k]];
}

// One lane per pair in key order (inside equal keys: score down, then g up).  A pair whose key equals that of the pair before it is not its group's keeper: 0x400
// into the lines of both mates.  cnt[0] += pairs marked, cnt[1] += groups of two or more pairs (one add per wavefront).
__global__ __launch_bounds__(BLOCK) void k_pd_pick(const PdSrc *__restrict__ src, int n_src, const uint32_t *__restrict__ perm, int64_t n_pairs, const uint64_t *__restrict__ w1,
                                                   const uint64_t *__restrict__ w2, const uint64_t *__restrict__ w3, const uint32_t *__restrict__ g1, const uint32_t *__restrict__ g2,
                                                   unsigned long long *__restrict__ cnt)
{
	const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	bool dup = false, many = false;
	if (k < n_pairs) {
		const uint32_t p = perm[k];
		const uint64_t a = w1[p], b = w2[p], c = w3[p];
		if (k > 0) { const uint32_t q = perm[k - 1]; dup = w1[q] == a && w2[q] == b && w3[q] == c; }
		if (!dup && k + 1 < n_pairs) { const uint32_t q = perm[k + 1]; many = w1[q] == a && w2[q] == b && w3[q] == c; }
		if (dup) {
			const uint32_t gs[2] = {g1[p], g2[p]};
#pragma unroll
			for (int s = 0; s < 2; ++s) {
				const int bk = src_find(src, n_src, gs[s]);
				ssv_record *r = src[bk].rec + ((int64_t)gs[s] - src[bk].start);
				r->flag = (uint16_t)(r->flag | (uint16_t)F_DUP);
			}
		}
	}
	const uint64_t bd = __ballot(dup), bm = __ballot(many);
	if (lane_id() == 0) {
		if (bd) atomicAdd(&cnt[0], (unsigned long long)__popcll(bd));
		if (bm) atomicAdd(&cnt[1], (unsigned long long)__popcll(bm));
	}
}

} // namespace ssv
