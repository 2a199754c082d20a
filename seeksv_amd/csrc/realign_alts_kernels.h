// realign_alts_kernels.h - a clipped sequence's other loci (ssv_realign_query_alts; `seeksv realign -S`).
//
// The query kernel (k_ra_query_t of realign_kernels.h) holds every scored candidate of its query in LDS and reduces them to a winner and `second`.  With its
// fourth template parameter set it goes on behind the winner's write (ra_alts below, found by argument-dependent look-up like ras_seeds):
//
//   rule       best = the winner's score.  A candidate is an alternate locus when its score is >= RA_MIN_SCORE and 5 * score >= 4 * best (bwa mem's XA ratio
//              of 0.8), and it is not the locus - same strand, same contig, diagonals at most 32 apart: the window of `second` - of the winner or of an
//              alternate chosen before it.  Alternates are chosen greedily by (score descending, forward strand first, diagonal ascending, contig id
//              ascending): given the candidate set and the winner the list is a function of the input on either index (the hash index leaves a
//              winner tied between two contigs to the lanes' order: the other contig's candidate is then an alternate).  At most max_alt (1..16) are kept; when a locus
//              was left, the winner's pad[0] gets RA_F_ALT_CUT.
//   selection  a lane owns candidate slots lane, lane + 64, lane + 128 and keeps one bit per slot: qualifies and not yet suppressed.  A round: every lane's
//              first slot in the order above, a butterfly over the lanes on the slot NUMBER (two slots are compared through their LDS fields), lane k keeps
//              the k-th choice, every lane clears the slots of the chosen locus.  A query without a qualifying candidate - nearly all of them - leaves
//              after one pass over its slots and one ballot.
//   walk       only a candidate's score outlived the scoring (s_ss); lanes 0 .. k - 1 walk one chosen diagonal each again, side by side: one more walk of
//              the query, not k (ra_alt_walk: a copy of k_ra_query_t's step 4, see there).
//   output     strided: alts[q * max_alt + r] and alt_n[q].  Most queries have none, so the host call scans the counts (scan.h) and k_ra_alt_compact gathers the
//              hits into one dense array: alt_off[n + 1] and alt_off[n] hits cross PCIe.
//   gapped     the alternates are the first stage's (floor RA_K) and need RA_MIN_SCORE there.  A winner that the refinement (k_ra_gap) leaves unaligned scored
//              less than RA_MIN_SCORE in the first stage - the refinement never lowers a score -, so no candidate of its query reached RA_MIN_SCORE: it has
//              no alternates without anything being taken back.
// An alternate's hit: its own tid, pos, q_beg, q_end, score, n_mismatch, reverse; second = best; mapq 0; pad[0] = the winner's; pad[1] 0.  Alternates are not
// gap-refined.  No atomics, no block barrier (a wavefront's LDS is its own slice), no scratch.
#pragma once

#include "common.h"
#include "realign_kernels.h"
#include "realign_sorted_kernels.h"

namespace ssv {

constexpr int RA_MAX_ALT = 16;
constexpr uint32_t RA_F_ALT_CUT = 4; // = SSV_RA_F_ALT_CUT
constexpr int RA_ALT_NUM = 5, RA_ALT_DEN = 4; // 5 * score >= 4 * best
static_assert(RA_MAX_CAND % WAVE == 0 && RA_MAX_ALT <= WAVE, "a lane owns RA_MAX_CAND / WAVE slots; one lane per alternate");

template <typename Base>
struct RaAltArgs : Base { // the query kernel's arguments + where the alternates go
	RaHit *alts;          // [n * max_alt]
	int32_t *alt_n;       // [n], every one written
	int32_t max_alt;
};

// does candidate slot x come before slot y in the alternates' order?  (-1: no slot)
__device__ __forceinline__ bool ra_alt_before(const uint16_t *ss, const int64_t *diag, const int32_t *tid, int x, int y)
{
	if (x < 0 || y < 0) return x >= 0 && y < 0;
	const int sx = ss[x] & 0x7fff, sy = ss[y] & 0x7fff;
	if (sx != sy) return sx > sy;
	const int tx = ss[x] >> 15, ty = ss[y] >> 15;
	if (tx != ty) return tx < ty;
	const int64_t dx = diag[x], dy = diag[y];
	if (dx != dy) return dx < dy;
	const int cx = tid[x], cy = tid[y];
	if (cx != cy) return cx < cy;
	return x < y; // (two scored slots never agree in all three: a duplicate is not scored)
}

// the query (codes of the candidate's orientation, n bases) along diagonal d inside contig t, as k_ra_query_t scores it -> score, segment, mismatches
// (A copy of that kernel's walk without its two early exits - a chosen candidate passed them.  One function for both moved the default kernels from
// 60 / 72 VGPRs to 52-54 / 66 whether the floor was a template or a plain parameter and the results references, pointers or a struct: DESIGN.md 10e.)
__device__ __forceinline__ void ra_alt_walk(const RaIndex &ix, const uint8_t *code, int n, int64_t d, int t, int *score, int *q_beg, int *q_end, int *n_mm)
{
	const int64_t c_lo = ix.ctg_off[t], c_hi = ix.ctg_off[t + 1];
	const int i_lo = (int)(c_lo - d > 0 ? c_lo - d : 0), i_hi = (int)(c_hi - d < n ? c_hi - d : n);
	int run = 0, run_beg = i_lo, bs = 0, bb = i_lo, be = i_lo;
	for (int i = i_lo; i < i_hi; ++i) {
		const bool eq = code[i] < 4 && (uint32_t)code[i] == ra_base_at(ix.ref, d + i);
		if (run <= 0) { run = 0; run_beg = i; }
		run += eq ? RA_MATCH : -RA_MISMATCH;
		if (run > bs) { bs = run; bb = run_beg; be = i + 1; }
	}
	if (bb > i_lo || be < i_hi) {
		int sc = 0;
		if (bb > 0 && i_lo == 0) {
			for (int i = bb - 1; i >= 0; --i) sc += (code[i] < 4 && (uint32_t)code[i] == ra_base_at(ix.ref, d + i)) ? RA_MATCH : -RA_MISMATCH;
			if (sc > -RA_CLIP) { bs += sc; bb = 0; }
		}
		sc = 0;
		if (be < n && i_hi == n) {
			for (int i = be; i < n; ++i) sc += (code[i] < 4 && (uint32_t)code[i] == ra_base_at(ix.ref, d + i)) ? RA_MATCH : -RA_MISMATCH;
			if (sc > -RA_CLIP) { bs += sc; be = n; }
		}
	}
	int mm = 0;
	for (int i = bb; i < be; ++i) mm += (code[i] < 4 && (uint32_t)code[i] == ra_base_at(ix.ref, d + i)) ? 0 : 1;
	*score = bs; *q_beg = bb; *q_end = be; *n_mm = mm;
}

// The alternates of query q, whose m candidates are scored (s_ss) and whose winner - strand win_st, contig win_tid, diagonal win_diag, score best, all
// wave-uniform - lane win_lane has written to a.hits[q] with the flags `flags`.  Called by all lanes of the wavefront.
template <typename Base>
__device__ __forceinline__ void ra_alts(const RaAltArgs<Base> &a, int w, int lane, int n, int m, int64_t q, const uint8_t (&s_code)[WAVES_PER_BLOCK][2][RA_MAX_Q],
                                        const int64_t (&s_diag)[WAVES_PER_BLOCK][RA_MAX_CAND], const uint16_t (&s_ss)[WAVES_PER_BLOCK][RA_MAX_CAND],
                                        const int32_t (&s_tid)[WAVES_PER_BLOCK][RA_MAX_CAND], int win_st, int win_tid, int64_t win_diag, int best, int win_lane, uint32_t flags)
{
	constexpr int SLOTS = RA_MAX_CAND / WAVE;
	const uint16_t *ss = s_ss[w];
	const int64_t *diag = s_diag[w];
	const int32_t *tid = s_tid[w];
	uint32_t alive = 0;
#pragma unroll
	for (int j = 0; j < SLOTS; ++j) {
		const int c = j * WAVE + lane;
		if (c >= m) continue;
		const int sc = ss[c] & 0x7fff;
		if (sc >= RA_MIN_SCORE && RA_ALT_NUM * sc >= RA_ALT_DEN * best && !ra_same_locus(ss[c] >> 15, tid[c], diag[c], win_st, win_tid, win_diag)) alive |= 1u << j;
	}
	int k = 0, mine = -1;
	while (k < a.max_alt && __ballot(alive != 0) != 0ull) { // (wave-uniform)
		int pick = -1;
#pragma unroll
		for (int j = 0; j < SLOTS; ++j) {
			const int c = j * WAVE + lane;
			if (((alive >> j) & 1u) && ra_alt_before(ss, diag, tid, c, pick)) pick = c;
		}
#pragma unroll
		for (int dlt = 32; dlt >= 1; dlt >>= 1) {
			const int o = __shfl_xor(pick, dlt, 64);
			if (ra_alt_before(ss, diag, tid, o, pick)) pick = o;
		}
		if (lane == k) mine = pick;
		const int p_st = ss[pick] >> 15, p_tid = tid[pick];
		const int64_t p_diag = diag[pick];
#pragma unroll
		for (int j = 0; j < SLOTS; ++j) {
			const int c = j * WAVE + lane;
			if (!((alive >> j) & 1u)) continue;
			if (ra_same_locus(ss[c] >> 15, tid[c], diag[c], p_st, p_tid, p_diag)) alive &= ~(1u << j);
		}
		++k;
	}
	if (__ballot(alive != 0) != 0ull) { // a locus was left
		flags |= RA_F_ALT_CUT;
		if (lane == win_lane) a.hits[q].pad[0] = (uint8_t)flags;
	}
	if (lane == 0) a.alt_n[q] = k;
	if (lane < k) {
		const int st = ss[mine] >> 15, t = tid[mine];
		const int64_t d = diag[mine];
		int sc, qb, qe, mm;
		ra_alt_walk(a.ix, s_code[w][st], n, d, t, &sc, &qb, &qe, &mm);
		RaHit h;
		h.tid = t; h.pos = (int32_t)(d + qb - a.ix.ctg_off[t]);
		h.q_beg = qb; h.q_end = qe; h.score = sc; h.second = best; h.n_mismatch = mm;
		h.reverse = (uint8_t)st; h.mapq = 0; h.pad[0] = (uint8_t)flags; h.pad[1] = 0;
		a.alts[q * a.max_alt + lane] = h;
	}
}

// one thread per query: its alt_n[q] strided hits -> dense[alt_off[q] ...]
__global__ __launch_bounds__(BLOCK) void k_ra_alt_compact(const RaHit *__restrict__ alts, const int32_t *__restrict__ alt_n, const int64_t *__restrict__ alt_off, int64_t n, int32_t max_alt,
                                                          RaHit *__restrict__ dense)
{
	const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (q >= n) return;
	const int k = alt_n[q];
	if (k <= 0) return;
	const int64_t o = alt_off[q];
	for (int r = 0; r < k; ++r) dense[o + r] = alts[q * max_alt + r];
}

constexpr auto k_ra_query_alts = k_ra_query_t<false, RaAltArgs<RaQueryArgs>, RA_MIN_SCORE, true>;
constexpr auto k_ra_query_floor_alts = k_ra_query_t<false, RaAltArgs<RaQueryArgs>, RA_K, true>;
constexpr auto k_ras_query_alts = k_ra_query_t<true, RaAltArgs<RasQueryArgs>, RA_MIN_SCORE, true>;
constexpr auto k_ras_query_floor_alts = k_ra_query_t<true, RaAltArgs<RasQueryArgs>, RA_K, true>;

} // namespace ssv
