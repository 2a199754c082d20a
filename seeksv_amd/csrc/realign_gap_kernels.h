// realign_gap_kernels.h - one insertion or deletion per clipped-sequence alignment (ssv_realign_query_gapped; `seeksv realign -g`).
//
// k_ra_gap runs behind the query kernel (k_ra_query_t with the candidate floor at RA_K) over its hits: one wavefront per query, and it looks at the
// winner only.  The winner is strand st, contig [c_lo, c_hi), diagonal d (reference position of query base 0), segment [q_beg, q_end) and its score.
// s(i, D) = +1 when query base i (in the hit's orientation) is a base and equals the reference at D + i, else -4; a piece covers only query positions
// whose reference position lies inside the contig.
//
//   variants   64 = {D, I} x L = 1..RA_MAX_GAP x {the winner is the left piece, the winner is the right piece}, one per lane.  g = +L (D) / -L (I).  The
//              left piece is query [b, k) on diagonal dl, the right piece [j, e) on dr = dl + g, j = k (D) or k + L (I).
//   winner left    dl = d, b = q_beg.  Every k > q_beg with j <= n - 1: left = sum of s(i, d) over [q_beg, k), right = the best segment on dr that starts
//              exactly at j, run on to n when n is reachable inside the contig and the sum over [j, n) is > best - RA_CLIP (the query kernel's end rule).
//   winner right   dr = d, e = q_end.  Every j < q_end with k >= 1: right = sum of s(i, d) over [j, q_end), left = the mirror image on dl: the best segment
//              that ends exactly at k, run on to 0 by the same rule.
//   score      J = left + right - (RA_GAP_OPEN + L).  Inside a variant the largest J, then the smallest k (the gap is left-aligned).  Across variants
//              the largest J, then the smaller L, then D before I, then winner-left before winner-right: the lane number is that order.
//   result     only when J > score: pos = the left piece's first reference base, q_beg, q_end, score = J, n_mismatch over both pieces (inserted bases
//              are not counted), mapq from the new score and the unchanged second.  tid, reverse, second and pad[0] stay.  A hit that is below
//              RA_MIN_SCORE after this (the floor let it through) is written unaligned in every field but pad[0].
//
// The sums along d are prefix sums in LDS (int16, a wave scan per 64 positions); the other piece is one pass per lane along its own diagonal: winner-left
// lanes walk j down from n - 1 with  best(j) = s(j) + max(best(j + 1), 0),  total(j) = s(j) + total(j + 1); winner-right lanes walk k up the same way.
// The lanes' diagonals lie within RA_MAX_GAP bases of d: a lane keeps its 64-bit reference word in a register and loads the next one every 32 bases.
// No atomics, no block barrier (a wavefront's LDS is its own slice), no scratch.
#pragma once

#include "common.h"
#include "realign_kernels.h"

namespace ssv {

constexpr int RA_MAX_GAP = 16;
constexpr int RA_GAP_OPEN = 6; // + 1 per base: a gap of L costs 6 + L (bwa mem's defaults)
static_assert(4 * RA_MAX_GAP == WAVE, "one lane per variant");

struct RaGap { int32_t q_at, len; }; // = ssv_realign_gap

struct RaGapArgs {
	const uint64_t *ref;
	const int64_t *ctg_off;
	const char *seqs;
	const uint64_t *seq_off;
	int64_t n;
	RaHit *hits;              // in: the query kernel's; out: refined
	RaGap *gaps;              // [n], every one written
};

__device__ __forceinline__ int ra_sval(uint32_t code, uint32_t base) { return code == base ? RA_MATCH : -RA_MISMATCH; } // (a code of 4 equals no base)

__global__ __launch_bounds__(BLOCK) void k_ra_gap(RaGapArgs a)
{
	__shared__ uint8_t s_code[WAVES_PER_BLOCK][RA_MAX_Q];
	__shared__ int16_t s_pre[WAVES_PER_BLOCK][RA_MAX_Q + 2]; // s_pre[i] = sum of s(x, d) over the query positions x < i inside the contig (|sum| <= 4 * RA_MAX_Q)
	const int w = wave_id(), lane = lane_id();
	const int64_t q = (int64_t)blockIdx.x * WAVES_PER_BLOCK + w;
	if (q >= a.n) return;
	RaHit h = a.hits[q];
	if (h.tid < 0) { if (lane == 0) a.gaps[q] = RaGap{0, 0}; return; }
	const uint64_t o0 = a.seq_off[q];
	const int n = (int)(a.seq_off[q + 1] - o0); // RA_K..RA_MAX_Q: the query kernel aligned it
	uint8_t *code = s_code[w];
	int16_t *pre = s_pre[w];
	ra_codes(a.seqs + o0, n, lane, h.reverse ? RA_REV : RA_FWD, code, code); // the hit's orientation only
	const int64_t c_lo = a.ctg_off[h.tid], c_hi = a.ctg_off[h.tid + 1];
	const int64_t d = c_lo + h.pos - h.q_beg;
	const int qb = h.q_beg, qe = h.q_end;
	const int i_lo = (int)(c_lo - d > 0 ? c_lo - d : 0), i_hi = (int)(c_hi - d < n ? c_hi - d : n); // query positions inside the contig along d
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
	// ---- prefix sums along the winner's diagonal ----
	if (lane == 0) pre[0] = 0;
	int carry = 0;
	for (int i0 = 0; i0 < n; i0 += WAVE) {
		const int i = i0 + lane;
		const int v = (i >= i_lo && i < i_hi) ? ra_sval(code[i], ra_base_at(a.ref, d + i)) : 0;
		const int inc = wave_inclusive_sum(v);
		if (i < n) pre[i + 1] = (int16_t)(carry + inc);
		carry += __shfl(inc, WAVE - 1, 64);
	}
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
	// ---- lane = variant, in the order that decides between equal scores ----
	const int L = (lane >> 2) + 1;
	const bool ins = (lane >> 1) & 1, right = lane & 1;
	const int g = ins ? -L : L, ins_len = ins ? L : 0, pen = RA_GAP_OPEN + L;
	const int64_t d2 = right ? d - g : d + g; // the other piece's diagonal: dr of a winner-left lane, dl of a winner-right lane
	const int lo2 = (int)(c_lo - d2 > 0 ? c_lo - d2 : 0), hi2 = (int)(c_hi - d2 < n ? c_hi - d2 : n);
	const bool reach = right ? lo2 == 0 : hi2 == n; // the query's end on this lane's side lies inside the contig
	const int fixed = right ? pre[qe] : pre[qb];
	int best_j = INT32_MIN, best_k = 0; // (best_j: the variant's J)
	int loc = 0, tot = 0;
	int64_t wi = -1;
	uint64_t word = 0;
	for (int t = 0; t < n; ++t) {
		const int i = right ? t : n - 1 - t;
		if (i < lo2 || i >= hi2) continue;
		const int64_t p = d2 + i; // inside [c_lo, c_hi)
		if ((p >> 5) != wi) { wi = p >> 5; word = a.ref[wi]; }
		const int v = ra_sval(code[i], (uint32_t)(word >> ((p & 31) * 2)) & 3u);
		loc = v + (loc > 0 ? loc : 0);
		tot += v;
		const int ext = (reach && tot > loc - RA_CLIP) ? tot : loc;
		if (right) { // the left piece ends at k = i + 1; k ascends: the first of equal ones stays
			const int k = i + 1, j = k + ins_len;
			if (j < qe && j >= i_lo) {
				const int sc = ext + fixed - pre[j] - pen;
				if (sc > best_j) { best_j = sc; best_k = k; }
			}
		} else { // the right piece starts at j = i; k descends: the last of equal ones stays
			const int k = i - ins_len;
			if (k > qb && k <= i_hi) {
				const int sc = pre[k] - fixed + ext - pen;
				if (sc >= best_j) { best_j = sc; best_k = k; }
			}
		}
	}
	// ---- the best variant: largest J, then the smallest lane ----
	constexpr int BIAS = 1 << 14; // J > -BIAS: two pieces of at most RA_MAX_Q bases at -4 and the gap
	const int key = wave_max(best_j == INT32_MIN ? 0 : (((best_j + BIAS) << 6) | (WAVE - 1 - lane)));
	const int win_j = (key >> 6) - BIAS, win_lane = WAVE - 1 - (key & (WAVE - 1));
	const RaHit none = ra_unaligned(h.pad[0]);
	if (key == 0 || win_j <= h.score) { // no gap pays
		if (lane == 0) {
			if (h.score < RA_MIN_SCORE) a.hits[q] = none;
			a.gaps[q] = RaGap{0, 0};
		}
		return;
	}
	if (lane != win_lane) return;
	if (win_j < RA_MIN_SCORE) { a.hits[q] = none; a.gaps[q] = RaGap{0, 0}; return; }
	// ---- the winning lane: bounds of the free piece (the shortest of equal ones, then the end rule), mismatches of both ----
	const int k = best_k, j = k + ins_len;
	const int64_t dl = right ? d2 : d, dr = right ? d : d2;
	int b = qb, e = qe;
	{
		int run = 0, top = INT32_MIN;
		if (right) {
			for (int i = k - 1; i >= lo2; --i) {
				run += ra_sval(code[i], ra_base_at(a.ref, dl + i));
				if (run > top) { top = run; b = i; }
			}
			if (reach && run > top - RA_CLIP) b = 0;
		} else {
			for (int i = j; i < hi2; ++i) {
				run += ra_sval(code[i], ra_base_at(a.ref, dr + i));
				if (run > top) { top = run; e = i + 1; }
			}
			if (reach && run > top - RA_CLIP) e = n;
		}
	}
	int mm = 0;
	for (int i = b; i < k; ++i) mm += code[i] == ra_base_at(a.ref, dl + i) ? 0 : 1;
	for (int i = j; i < e; ++i) mm += code[i] == ra_base_at(a.ref, dr + i) ? 0 : 1;
	h.pos = (int32_t)(dl + b - c_lo);
	h.q_beg = b; h.q_end = e; h.score = win_j; h.n_mismatch = mm;
	h.mapq = ra_mapq(win_j, h.second);
	a.hits[q] = h;
	a.gaps[q] = RaGap{k, g};
}

} // namespace ssv
