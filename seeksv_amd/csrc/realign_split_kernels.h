// realign_split_kernels.h - a whole read's second piece (ssv_realign_query_split; `seeksv realign -P`).
//
// A read that crosses a breakpoint is two stretches of two loci.  The query kernel (k_ra_query_t of realign_kernels.h) scores both, reports the better one
// and counts the other against it: `second` close to `score`, MAPQ near 0.  With its fifth template parameter set it keeps every scored candidate's segment
// in LDS beside its score (s_seg: 2 x uint16 x RA_MAX_CAND a wavefront, in these instantiations only) and goes on behind the winner's write (ra_split below,
// found by argument-dependent look-up like ras_seeds and ra_alts):
//
//   intervals  in the READ's orientation: a candidate with segment [b, e) is [b, e) on the forward strand and [n - e, n - b) on the reverse strand.
//              shared(X, Y) = the length of the two intervals' intersection, 0 when they are disjoint.
//   mate       a scored candidate C with another (strand, contig, diagonal) than the primary P, with score >= RA_MIN_SCORE after its end extension, ordered
//              against P (P begins before C begins and ends before C ends, or the other way round: neither contains the other, equal begins or ends do not
//              count) and with >= RA_K bases of its own on both sides: len(P) - shared >= RA_K and len(C) - shared >= RA_K.  Overlap (microhomology) and a
//              gap between the pieces are allowed; the locus window plays no part.  Of several the first in the alternates' order (ra_alt_before: score
//              descending, forward strand first, diagonal ascending, contig id ascending).  Two pieces, never three.
//   MAPQ       with a mate, `second` of X in {P, M} = the best score among the scored candidates that are not X's locus (ra_same_locus), are not the other
//              piece and have shared(C, X) >= RA_K: a competitor for the SAME part of the read.  mapq = ra_mapq(score, second).  Without a mate the primary
//              stays as the plain query wrote it.
//   selection  a lane owns candidate slots lane, lane + 64, lane + 128: its first qualifying slot in the order, a butterfly over the lanes on the slot NUMBER,
//              two wave_max passes for the two `second` values.  Lane 0 writes mates[q]; the winner's lane rewrites second / mapq of hits[q].
//   mate's hit tid, pos, q_beg, q_end, score, reverse of its own slot; n_mismatch = (length - score) / (RA_MATCH + RA_MISMATCH) - a segment of l bases with
//              x mismatches scores l - 5 x -, so nothing is walked again; pad[0] = the primary's, pad[1] = 0.  No mate: ra_unaligned(pad[0]).
// No atomics, no block barrier (a wavefront's LDS is its own slice), no scratch.  Not combined with the floor of the gapped query or with the alternates.
#pragma once

#include "common.h"
#include "realign_kernels.h"
#include "realign_sorted_kernels.h"
#include "realign_alts_kernels.h"

namespace ssv {

static_assert(RA_MAX_Q < 65536, "a segment's ends are kept as uint16");

template <typename Base>
struct RaSplitArgs : Base { // the query kernel's arguments + where the mate pieces go
	RaHit *mates;           // [n], every one written
};

// a segment [b, e) of orientation st of an n-base query, in the read's own orientation
__device__ __forceinline__ void ra_fwd_interval(int st, int n, int b, int e, int *fb, int *fe)
{
	*fb = st ? n - e : b;
	*fe = st ? n - b : e;
}

__device__ __forceinline__ int ra_shared(int xb, int xe, int yb, int ye)
{
	const int lo = xb > yb ? xb : yb, hi = xe < ye ? xe : ye;
	return hi > lo ? hi - lo : 0;
}

// The mate piece of query q, whose m candidates are scored (s_ss) with their segments in s_seg, and whose winner - strand win_st, contig win_tid, diagonal
// win_diag, score best, segment [win_beg, win_end), all wave-uniform - lane win_lane has written to a.hits[q] with the flags `flags`.  Called by all lanes.
template <typename Base>
__device__ __forceinline__ void ra_split(const RaSplitArgs<Base> &a, int w, int lane, int n, int m, int64_t q, const int64_t (&s_diag)[WAVES_PER_BLOCK][RA_MAX_CAND],
                                         const uint16_t (&s_ss)[WAVES_PER_BLOCK][RA_MAX_CAND], const int32_t (&s_tid)[WAVES_PER_BLOCK][RA_MAX_CAND],
                                         const uint16_t (&s_seg)[WAVES_PER_BLOCK][2][RA_MAX_CAND], int win_st, int win_tid, int64_t win_diag, int best, int win_beg,
                                         int win_end, int win_lane, uint32_t flags)
{
	constexpr int SLOTS = RA_MAX_CAND / WAVE;
	const uint16_t *ss = s_ss[w];
	const int64_t *diag = s_diag[w];
	const int32_t *tid = s_tid[w];
	const uint16_t *seg_b = s_seg[w][0], *seg_e = s_seg[w][1];
	int pb, pe;
	ra_fwd_interval(win_st, n, win_beg, win_end, &pb, &pe);
	// ---- the mate: every lane's first qualifying slot, then the first over the lanes ----
	int pick = -1;
#pragma unroll
	for (int j = 0; j < SLOTS; ++j) {
		const int c = j * WAVE + lane;
		if (c >= m) continue;
		const int sc = ss[c] & 0x7fff, st = ss[c] >> 15;
		if (sc < RA_MIN_SCORE) continue; // (0: a duplicate or not scored)
		if (st == win_st && tid[c] == win_tid && diag[c] == win_diag) continue; // the primary itself
		int cb, ce;
		ra_fwd_interval(st, n, seg_b[c], seg_e[c], &cb, &ce);
		const bool ordered = (pb < cb && pe < ce) || (cb < pb && ce < pe);
		const int sh = ra_shared(pb, pe, cb, ce);
		if (ordered && pe - pb - sh >= RA_K && ce - cb - sh >= RA_K && ra_alt_before(ss, diag, tid, c, pick)) pick = c;
	}
#pragma unroll
	for (int dlt = 32; dlt >= 1; dlt >>= 1) {
		const int o = __shfl_xor(pick, dlt, 64);
		if (ra_alt_before(ss, diag, tid, o, pick)) pick = o;
	}
	if (pick < 0) { // (wave-uniform)
		if (lane == 0) a.mates[q] = ra_unaligned((uint8_t)flags);
		return;
	}
	const int m_sc = ss[pick] & 0x7fff, m_st = ss[pick] >> 15, m_tid = tid[pick], m_beg = seg_b[pick], m_end = seg_e[pick];
	const int64_t m_diag = diag[pick];
	int mb, me;
	ra_fwd_interval(m_st, n, m_beg, m_end, &mb, &me);
	// ---- each piece's competitors: another locus than the piece's, not the other piece, >= RA_K bases of the read in common with the piece ----
	int second_p = 0, second_m = 0;
#pragma unroll
	for (int j = 0; j < SLOTS; ++j) {
		const int c = j * WAVE + lane;
		if (c >= m) continue;
		const int sc = ss[c] & 0x7fff, st = ss[c] >> 15;
		if (sc == 0) continue;
		const int t = tid[c];
		const int64_t d = diag[c];
		int cb, ce;
		ra_fwd_interval(st, n, seg_b[c], seg_e[c], &cb, &ce);
		const bool is_p = st == win_st && t == win_tid && d == win_diag;
		if (sc > second_p && c != pick && !ra_same_locus(st, t, d, win_st, win_tid, win_diag) && ra_shared(cb, ce, pb, pe) >= RA_K) second_p = sc;
		if (sc > second_m && !is_p && !ra_same_locus(st, t, d, m_st, m_tid, m_diag) && ra_shared(cb, ce, mb, me) >= RA_K) second_m = sc;
	}
	second_p = wave_max(second_p);
	second_m = wave_max(second_m);
	if (lane == win_lane) {
		a.hits[q].second = second_p;
		a.hits[q].mapq = ra_mapq(best, second_p);
	}
	if (lane == 0) {
		RaHit h;
		h.tid = m_tid; h.pos = (int32_t)(m_diag + m_beg - a.ix.ctg_off[m_tid]);
		h.q_beg = m_beg; h.q_end = m_end; h.score = m_sc; h.second = second_m;
		h.n_mismatch = (m_end - m_beg - m_sc) / (RA_MATCH + RA_MISMATCH);
		h.reverse = (uint8_t)m_st; h.mapq = ra_mapq(m_sc, second_m); h.pad[0] = (uint8_t)flags; h.pad[1] = 0;
		a.mates[q] = h;
	}
}

constexpr auto k_ra_query_split = k_ra_query_t<false, RaSplitArgs<RaQueryArgs>, RA_MIN_SCORE, false, true>;
constexpr auto k_ras_query_split = k_ra_query_t<true, RaSplitArgs<RasQueryArgs>, RA_MIN_SCORE, false, true>;

} // namespace ssv
