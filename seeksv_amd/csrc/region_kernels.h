// region_kernels.h - `run -L`, `run -X`: the records of a batch restricted to a list of regions where they lie (the rule: include/seeksv_hip.h, ssv_regions_set).
// keep (streaming: the hot columns tid / pos, 8 bytes a record; a record's line only where its span decides; one byte a record out) -> scan -> place (the
// kept records' indices in order, what their variable parts take) -> scans -> gather (16 lanes a record, in input order, through retained.h) -> the contig
// changes of the output (sort_kernels.h's mark + place) and its tid column as runs (bamdec_kernels.h).  No atomics; every output byte has one writer.
#pragma once

#include "common.h"
#include "clip_kernels.h"
#include "retained.h"

namespace ssv {

constexpr int REGION_LDS_CAP = 2048; // regions of one contig that are staged in LDS (16 KB of the workgroup's): a longer list is searched in global memory
constexpr int REGION_TILES = 16;     // consecutive 256-record tiles of one workgroup: a staged list stays while they stay on its contig

// the list on the device: contig c's regions are [off[c], off[c + 1]) of s[] / t[], sorted, no two overlapping or abutting
struct RegionList {
	const uint32_t *off;
	const int32_t *s, *t;
	int32_t n_targets;
};

// the last of m regions with s < e, -1: none (S: where the starts lie - LDS or global memory)
template <typename S> __device__ __forceinline__ int region_last_below(S s, int m, int64_t e)
{
	int lo = 0, hi = m; // the first region with s >= e
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if ((int64_t)s[mid] < e) lo = mid + 1; else hi = mid;
	}
	return lo - 1;
}

// the rule's span, in 64 bits: from the line's five operations when the record has no more, else from cigar[]
__device__ __forceinline__ int64_t region_span(const RecLine &r, const uint32_t *__restrict__ cigar)
{
	const int nc = r.n_cigar();
	int64_t span = 0;
	for (int k = 0; k < nc; ++k) {
		const uint32_t x = nc <= 5 ? r.head(k) : cigar[r.cigar_off() + (uint32_t)k];
		const int op = (int)(x & 15u);
		if (op == C_M || op == C_D || op == C_N || op == C_EQ || op == C_X) span += (int64_t)(x >> 4);
	}
	return span;
}

// Does record i, at `pos` on a contig with the m regions s[] / t[], overlap one of them.  After merging, the last region with s < e decides.  With a bound on
// every record's span (max_span > 0) the line is fetched only where the span matters: a record whose widest possible interval [pos, pos + max_span) reaches
// no region overlaps none, and one whose first base lies in a region overlaps whatever its span - both exact, because t rises with s in a merged list.
template <typename S> __device__ __forceinline__ bool region_overlap(S s, S t, int m, int64_t pos, int32_t max_span, const ssv_record *__restrict__ rec, const uint32_t *__restrict__ cigar, int64_t i)
{
	if (m == 0 || pos < 0) return false; // (a position of -1 is the interval [-1, 0) whatever the CIGAR says: no region starts below 0)
	if (max_span > 0) {
		const int k = region_last_below(s, m, pos + (int64_t)max_span);
		if (k < 0 || (int64_t)t[k] <= pos) return false;
		if ((int64_t)s[k] <= pos) return true;
	}
	const int64_t span = region_span(rec_load(rec, i), cigar);
	const int k = region_last_below(s, m, pos + (span > 1 ? span : 1));
	return k >= 0 && (int64_t)t[k] > pos;
}

// keep[i] = 1: record i stays (include mode: it overlaps; exclude mode: it does not).  A tile whose records all lie on one contig with at most REGION_LDS_CAP
// regions searches that contig's list in LDS; every other tile - a contig change falls into it, the list is longer, the records are in any order - searches
// global memory.  A contig id outside [0, n_targets) has no regions.
__global__ __launch_bounds__(BLOCK) void k_region_keep(DevBatch b, RegionList L, int exclude, uint8_t *__restrict__ keep)
{
	__shared__ int32_t ls[REGION_LDS_CAP], lt[REGION_LDS_CAP];
	int32_t staged = -1; // (the same in every thread)
	for (int k = 0; k < REGION_TILES; ++k) {
		const int64_t base = ((int64_t)blockIdx.x * REGION_TILES + k) * BLOCK;
		if (base >= b.n) break;
		const int64_t i = base + threadIdx.x;
		const bool in = i < b.n;
		const int32_t t0 = b.tid[base];
		const int32_t tid = in ? b.tid[i] : t0;
		const int64_t pos = in ? (int64_t)b.pos[i] : -1;
		const bool placed = t0 >= 0 && t0 < L.n_targets;
		const uint32_t first0 = placed ? L.off[t0] : 0u;
		const int m0 = placed ? (int)(L.off[t0 + 1] - first0) : 0;
		const bool one = __syncthreads_and(tid == t0) && m0 > 0 && m0 <= REGION_LDS_CAP; // (the barrier: nobody searches the staged list any more)
		bool ov = false;
		if (one) {
			if (staged != t0) {
				for (int j = (int)threadIdx.x; j < m0; j += BLOCK) { ls[j] = L.s[first0 + (uint32_t)j]; lt[j] = L.t[first0 + (uint32_t)j]; }
				staged = t0;
				__syncthreads();
			}
			if (in) ov = region_overlap(ls, lt, m0, pos, b.max_ref_span, b.rec, b.cigar, i);
		} else if (in && tid >= 0 && tid < L.n_targets) {
			const uint32_t first = L.off[tid];
			ov = region_overlap(L.s + first, L.t + first, (int)(L.off[tid + 1] - first), pos, b.max_ref_span, b.rec, b.cigar, i);
		}
		if (in) keep[i] = (uint8_t)(exclude ? !ov : ov);
	}
}

// the kept records in order: idx[d] = the input record that becomes output record d, and what it takes there - its operations, the bytes of its bases +
// qualities when it has them
__global__ __launch_bounds__(BLOCK) void k_region_place(DevBatch b, const uint8_t *__restrict__ keep, const uint32_t *__restrict__ at, uint32_t *__restrict__ idx,
                                                        uint32_t *__restrict__ cig_n, uint32_t *__restrict__ seq_b)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= b.n || !keep[i]) return;
	const uint4 *p = reinterpret_cast<const uint4 *>(b.rec + i);
	const uint4 q = p[1], e = p[3];
	const int lq = (int)q.x > 0 ? (int)q.x : 0;
	const bool has = ((uint64_t)e.z | ((uint64_t)e.w << 32)) != SSV_NO_SEQ;
	const uint32_t d = at[i];
	idx[d] = (uint32_t)i;
	cig_n[d] = (uint32_t)b.n_cigar[i];
	seq_b[d] = has ? seq_bytes(lq) : 0u;
}

// 16 lanes per output record: the first lane the hot columns and the line (cigar_off / seq_off for the new batch, nothing else changed), all of them the
// operations and the bytes of bases + qualities
__global__ __launch_bounds__(BLOCK) void k_region_gather(DevBatch b, const uint32_t *__restrict__ idx, int64_t count, const uint32_t *__restrict__ cig_at, const uint64_t *__restrict__ seq_at,
                                                         const uint32_t *__restrict__ seq_b, RetDst dst)
{
	const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	const int64_t d = t / RET_SUB;
	const int sub = (int)(t & (RET_SUB - 1));
	if (d >= count) return;
	const int64_t i = idx[d];
	const RecLine r = rec_load(b.rec, i);
	const uint32_t coff = cig_at[d], sb = seq_b[d];
	const uint64_t soff = seq_at[d];
	if (sub == 0) ret_write_record(dst, d, r, b.ends + i, r.w_fmx, coff, r.seq_off() != SSV_NO_SEQ ? soff : SSV_NO_SEQ);
	ret_copy_parts(dst, r, b.cigar, b.seqqual, sub, coff, soff, sb);
}

} // namespace ssv
