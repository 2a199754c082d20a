// probe_kernels.h - `seeksv somatic -K`: the tumor rows' look-ups among the normal sample's clusters, against a pass's cluster table where it lies
// in device memory (format 0: o_tid / o_pos / o_side / o_support / o_ll / o_lr / o_stroff / o_str).  The rule is DESIGN.md 8a, word for word the one of
// tests/somatic_probe_model.py; the host form is probe_normal_clusters (somatic_stage.cpp), the reference's somatic.cpp:58-427 and clip_reads.cpp:194-217,333-370.
// One wavefront per probe; no barrier, no atomics, no LDS: a sample has a few ten-thousand probes, each against a handful of candidates.
#pragma once

#include "common.h"
#include "seeksv_hip.h"

namespace ssv {

struct ProbeArgs {
	const ssv_clip_probe *probes;
	int64_t n_probes;
	const uint8_t *text;
	const uint32_t *thr;      // thr[n]: the fewest equal characters out of n that reach the match rate (the host's own division); 0xffffffff: none does (n == 0, a NaN rate)
	uint32_t min_clipped_len; // unsigned compare, somatic.h:54
	int32_t pass;             // clustered passes since the set, 0-based
	// the pass's table
	const int32_t *tid, *pos, *support, *ll, *lr;
	const uint8_t *side, *str;
	const uint64_t *str_off;
	int64_t n_clusters;
	ssv_clip_probe_hit *hits;
};

// a string that is one piece of memory followed by another (s3 + s4[0..h) without the copy); one piece: n1 == 0
struct ProbeStr {
	const uint8_t *p0, *p1;
	int n0, n1;
	__device__ __forceinline__ int len() const { return n0 + n1; }
	__device__ __forceinline__ uint8_t at(int i) const { return i < n0 ? p0[i] : p1[i - n0]; }
};
__device__ __forceinline__ ProbeStr probe_str(const uint8_t *p, int n) { return ProbeStr{p, p, n, 0}; }

// CompareStringBeginFirst / CompareStringEndFirst >= match_rate: n = min(|x|, |y|) characters from the beginning (from_end: from the last characters),
// the lanes take them 64 at a time; every lane returns the same answer
__device__ __forceinline__ bool probe_match(const ProbeStr &x, const ProbeStr &y, bool from_end, const uint32_t *thr)
{
	const int lx = x.len(), ly = y.len(), n = lx < ly ? lx : ly;
	const int ox = from_end ? lx - n : 0, oy = from_end ? ly - n : 0;
	uint32_t m = 0;
	for (int i0 = 0; i0 < n; i0 += WAVE) {
		const int i = i0 + lane_id();
		const bool eq = i < n && x.at(ox + i) == y.at(oy + i);
		m += (uint32_t)__popcll(__ballot(eq));
	}
	return m >= thr[n]; // (thr[0] is 0xffffffff: 0 / 0 is NaN on the host and compares false)
}

// the first occurrence of s2[0..10) in s4 (std::string::find), -1: none.  Lane l looks at the offsets l, l + 64, ...; the lowest hit of the first round that has one
__device__ __forceinline__ int probe_anchor(const uint8_t *s2, const uint8_t *s4, int n4)
{
	const int last = n4 - 10; // the last offset at which ten characters fit
	for (int o0 = 0; o0 <= last; o0 += WAVE) {
		const int o = o0 + lane_id();
		bool hit = o <= last;
		if (hit) for (int j = 0; j < 10; ++j) hit = hit && s4[o + j] == s2[j];
		const uint64_t mask = __ballot(hit);
		if (mask) return o0 + (int)__ffsll((unsigned long long)mask) - 1;
	}
	return -1;
}

// (tid, side, pos) of cluster k against (t, s3, p) in the table's order: contigs ascending, per contig the '5' clusters before the '3' clusters, positions ascending
__device__ __forceinline__ bool probe_before(const ProbeArgs &a, int64_t k, int32_t t, bool s3, int32_t p)
{
	const int32_t kt = a.tid[k];
	if (kt != t) return kt < t;
	const bool k3 = a.side[k] == '3';
	if (k3 != s3) return !k3;
	return a.pos[k] < p;
}

__global__ __launch_bounds__(WAVE) void k_somatic_probe(ProbeArgs a)
{
	const int64_t q = (int64_t)blockIdx.x;
	if (q >= a.n_probes) return;
	const ssv_clip_probe pr = a.probes[q];
	if (pr.tid < 0) return;
	const ssv_clip_probe_hit old = a.hits[q];
	const bool s3 = pr.side == '3';
	// the first cluster of the probe's (contig, side) run at or behind lo (every lane the same bisection: uniform loads)
	int64_t lo = 0, hi = a.n_clusters;
	while (lo < hi) {
		const int64_t mid = lo + ((hi - lo) >> 1);
		if (probe_before(a, mid, pr.tid, s3, pr.lo)) lo = mid + 1; else hi = mid;
	}
	const ProbeStr pa = probe_str(a.text + pr.a_off, (int)pr.a_len), pb = probe_str(a.text + pr.b_off, (int)pr.b_len);
	for (int64_t k = lo; k < a.n_clusters; ++k) {
		if (a.tid[k] != pr.tid || (a.side[k] == '3') != s3) break;
		const int32_t pos = a.pos[k];
		if (pos > pr.hi) break;
		if (old.support != 0 && pos >= old.pos) break; // an earlier pass's match stays unless this pass has one at a strictly smaller position
		const int ll = a.ll[k], lr = a.lr[k];
		if ((uint32_t)(s3 ? lr : ll) < a.min_clipped_len) continue; // ReadsClipReads drops the row: the clipped side is too short
		const uint8_t *blk = a.str + a.str_off[k]; // seq_left, qual_left, seq_right, qual_right
		const ProbeStr cl = probe_str(blk, ll), cr = probe_str(blk + 2 * (size_t)ll, lr);
		bool ok;
		if (pr.mode == 0) ok = probe_match(pb, cr, false, a.thr) && probe_match(pa, cl, true, a.thr);
		else {
			const ProbeStr &s1 = pr.mode == 1 ? cl : pa, &s2 = pr.mode == 1 ? cr : pb, &s3_ = pr.mode == 1 ? pa : cl, &s4 = pr.mode == 1 ? pb : cr;
			ok = false;
			if (s2.n0 >= 10) {
				const int h = probe_anchor(s2.p0, s4.p0, s4.n0);
				if (h >= 0) {
					const ProbeStr head{s3_.p0, s4.p0, s3_.n0, h}, tail = probe_str(s4.p0 + h, s4.n0 - h);
					ok = probe_match(s1, head, true, a.thr) && probe_match(s2, tail, false, a.thr);
				}
			}
		}
		if (ok) {
			if (lane_id() == 0) {
				ssv_clip_probe_hit h;
				h.support = a.support[k]; h.pos = pos; h.pass = a.pass; h.pad = 0; h.cluster = k;
				a.hits[q] = h;
			}
			break;
		}
	}
}

} // namespace ssv
