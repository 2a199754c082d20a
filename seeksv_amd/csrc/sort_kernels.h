// sort_kernels.h - `run -u`: the retained batches of an original in any order, coordinate sorted where they lie (the rule: include/seeksv_hip.h, ssv_batch_sort).
// check (streaming: the hot columns tid / pos, 8 bytes a record, over all input batches as one sequence: does (t, p) ever go down, a contig beyond the header's,
// the largest p) -> keys (u64 key of the bits that can differ, u32 global index) -> radix_sort.h -> per output batch: sizes of the variable parts ->
// scans -> gather (16 lanes a record, from wherever the source lies) -> the flag-filtered contig changes (mark + scan + ordered compaction).
// A small table of the input batches maps a global index back to its batch (binary search: a few hundred entries).  No atomics but the look-first atomicMax
// of the check's largest p; every output byte has one writer.
#pragma once

#include "common.h"
#include "clip_kernels.h"
#include "bamdec_kernels.h"
#include "retained.h"

namespace ssv {

constexpr int SORT_SUB = RET_SUB;   // lanes per record in the gather

// one input batch: where its records start in the sequence of all inputs, and its arrays
struct SortSrc {
	int64_t start;
	const int32_t *tid, *pos;
	const uint16_t *n_cigar;
	const uint8_t *ends;
	const ssv_record *rec;
	const uint32_t *cigar;
	const uint8_t *seqqual;
};

__device__ __forceinline__ int2 sort_pos(const SortSrc *__restrict__ src, int n_src, int64_t g)
{
	const int k = src_find(src, n_src, g);
	const int64_t j = g - src[k].start;
	return make_int2(src[k].tid[j], src[k].pos[j]);
}

// the rule's key: unplaced records behind every contig, position -1 in front of position 0
__device__ __forceinline__ uint32_t sort_t(int tid, int n_targets) { return tid < 0 ? (uint32_t)n_targets : (uint32_t)tid; }
__device__ __forceinline__ uint32_t sort_p(int pos) { return (uint32_t)pos + 1u; }

enum SortWord { SW_DOWN, SW_BAD, SW_MAXP, SW_RAW_RUNS, SW_LAST_TID, SW_COUNT32 }; // u32 words of the small block; behind them u64 words (sort_api.inc)

// ---- check ----
// w[SW_DOWN] = 1: (t, p) goes down between two neighbours (batch seams included); w[SW_BAD] = 1: a contig id at or beyond n_targets; w[SW_MAXP] = the largest p
__global__ __launch_bounds__(BLOCK) void k_sort_check(const SortSrc *__restrict__ src, int n_src, int64_t n, int n_targets, uint32_t *__restrict__ w)
{
	const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	const bool in = g < n;
	const int2 k = in ? sort_pos(src, n_src, g) : make_int2(0, -1);
	const uint32_t t = sort_t(k.x, n_targets), p = sort_p(k.y);
	uint32_t pt = __shfl_up(t, 1, 64), pp = __shfl_up(p, 1, 64);
	if (lane_id() == 0 && in && g > 0) { const int2 q = sort_pos(src, n_src, g - 1); pt = sort_t(q.x, n_targets); pp = sort_p(q.y); }
	if (in && g > 0 && (pt > t || (pt == t && pp > p))) w[SW_DOWN] = 1u;
	if (in && k.x >= n_targets) w[SW_BAD] = 1u;
	const uint32_t mp = wave_max(in ? p : 0u);
	if (lane_id() == 0 && mp > __hip_atomic_load(&w[SW_MAXP], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&w[SW_MAXP], mp); // (look first: one address, a wavefront each)
}

// ---- keys ----
// key = t << p_bits | p (p < 2^p_bits: the check's largest p), value = the global index
__global__ __launch_bounds__(BLOCK) void k_sort_keys(const SortSrc *__restrict__ src, int n_src, int64_t n, int n_targets, int p_bits, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
	const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (g >= n) return;
	const int2 k = sort_pos(src, n_src, g);
	keys[g] = ((uint64_t)sort_t(k.x, n_targets) << p_bits) | (uint64_t)sort_p(k.y);
	vals[g] = (uint32_t)g;
}

// ---- sizes ----
// what output record first + d takes in its batch: its operations, the bytes of its bases + qualities when it has them
__global__ __launch_bounds__(BLOCK) void k_sort_sizes(const SortSrc *__restrict__ src, int n_src, const uint32_t *__restrict__ perm, int64_t first, int64_t count,
                                                      uint32_t *__restrict__ cig_n, uint32_t *__restrict__ seq_b)
{
	const int64_t d = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (d >= count) return;
	const int64_t g = perm[first + d];
	const int k = src_find(src, n_src, g);
	const int64_t j = g - src[k].start;
	const uint4 *p = reinterpret_cast<const uint4 *>(src[k].rec + j);
	const uint4 b = p[1], e = p[3];
	const int lq = (int)b.x > 0 ? (int)b.x : 0;
	const bool has = ((uint64_t)e.z | ((uint64_t)e.w << 32)) != SSV_NO_SEQ;
	cig_n[d] = (uint32_t)src[k].n_cigar[j];
	seq_b[d] = has ? seq_bytes(lq) : 0u;
}

// ---- gather ----
// 16 lanes per output record: the first lane the hot columns and the line (cigar_off / seq_off for the new batch, nothing else changed), all of them the
// operations and the bytes of bases + qualities
__global__ __launch_bounds__(BLOCK) void k_sort_gather(const SortSrc *__restrict__ src, int n_src, const uint32_t *__restrict__ perm, int64_t first, int64_t count,
                                                       const uint64_t *__restrict__ cig_at, const uint64_t *__restrict__ seq_at, const uint32_t *__restrict__ seq_b, RetDst dst)
{
	const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	const int64_t d = t / SORT_SUB;
	const int sub = (int)(t & (SORT_SUB - 1));
	if (d >= count) return;
	const int64_t g = perm[first + d];
	const int k = src_find(src, n_src, g);
	const int64_t j = g - src[k].start;
	const ssv_record *rec = src[k].rec;
	const uint32_t *cigar = src[k].cigar;
	const uint8_t *seqqual = src[k].seqqual;
	const RecLine r = rec_load(rec, j);
	const uint32_t coff = (uint32_t)cig_at[d], sb = seq_b[d];
	const uint64_t soff = seq_at[d];
	if (sub == 0) ret_write_record(dst, d, r, src[k].ends + j, r.w_fmx, coff, r.seq_off() != SSV_NO_SEQ ? soff : SSV_NO_SEQ);
	ret_copy_parts(dst, r, cigar, seqqual, sub, coff, soff, sb);
}

// ---- contig changes among the records that are not UNMAP|MUNMAP ----
// the flags of a batch's lines as a column (what k_tid_tile_last reads)
__global__ __launch_bounds__(BLOCK) void k_sort_flags(const ssv_record *__restrict__ rec, int64_t n, uint16_t *__restrict__ flag)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i < n) flag[i] = (uint16_t)(reinterpret_cast<const uint4 *>(rec + i)[0].z & 0xffffu);
}

// k_tid_runs' question, answered in place: mark[i] = 1 where record i passes the flag filter and its contig is not that of the last such record before it
// (tile_prev: k_tid_tile_last + k_tid_tile_carry)
__global__ __launch_bounds__(BLOCK) void k_sort_change_mark(const int32_t *__restrict__ tid, const uint16_t *__restrict__ flag, int64_t n, const int32_t *__restrict__ tile_prev,
                                                            uint32_t *__restrict__ mark)
{
	__shared__ int32_t wave_last[WAVES_PER_BLOCK];
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	const bool q = i < n && !(flag[i] & (F_UNMAP | F_MUNMAP));
	const int32_t mine = q ? tid[i] : TID_NONE;
	const uint64_t have = __ballot(q);
	const int32_t top = __shfl(mine, have ? 63 - __clzll((long long)have) : 0, 64); // all lanes take part in the shuffle
	if (lane_id() == 0) wave_last[wave_id()] = have ? top : TID_NONE;
	const uint64_t below = have & lanemask_lt();
	int32_t before = __shfl(mine, below ? 63 - __clzll((long long)below) : 0, 64);
	__syncthreads();
	if (!below) {
		before = tile_prev[blockIdx.x];
		for (int w = 0; w < wave_id(); ++w) if (wave_last[w] != TID_NONE) before = wave_last[w];
	}
	if (i < n) mark[i] = q && mine != before;
}

// the marked records in order: change k = (record index, its contig)
__global__ __launch_bounds__(BLOCK) void k_sort_change_place(const uint32_t *__restrict__ mark, const uint32_t *__restrict__ at, const int32_t *__restrict__ tid, int64_t n,
                                                             uint32_t *__restrict__ index, int32_t *__restrict__ ctid)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i < n && mark[i]) { index[at[i]] = (uint32_t)i; ctid[at[i]] = tid[i]; }
}

} // namespace ssv
