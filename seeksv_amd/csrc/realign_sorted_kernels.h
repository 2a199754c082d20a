// realign_sorted_kernels.h - the re-aligner's second seed index: the sampled 20-mers of the reference, sorted (ssv_realign_index_sorted; `seeksv realign -c`).
//
// The hash index of realign_kernels.h holds no key: all copies of a repeated 20-mer chain through their neighbours' slots, a position that finds no slot
// in RA_MAX_PROBE probes is dropped, and a query keeps the first RA_MAX_CAND seeds in the order an LDS atomic hands out slots.  On a reference with repeats
// that loses seeds of unique sequence and makes the hit depend on a race.  This index groups equal 20-mers instead:
//
//   keys[i], vals[i]   the 40-bit 20-mer (ra_kmer_at) and the sample number s = p / RA_SAMPLE of every sampled position, sorted by key with the library's
//                      stable radix sort (radix_sort.h): inside a run of equal 20-mers the positions ascend.  A sampled position whose 20-mer crosses a
//                      contig's end or the reference's gets the key RAS_NO_KEY = 1 << 40, which sorts behind every 20-mer: nothing is dropped, nothing else
//                      is left out, and there is no probe limit.  41 key bits: six passes of the sort.
//   dir[b]             first sorted entry whose key's top `bits` bits are >= b, b = 0 .. 2^bits (dir[2^bits] = the number of indexed positions), one thread per slot;
//                      bits = floor(log2(samples)), so a bucket holds 1-2 entries of random sequence.  A look-up reads dir[b], dir[b + 1] and finds the run
//                      by binary search inside the bucket (a bucket of real sequence can hold a whole satellite), then the run's end by doubling steps
//                      up to max_occ + 1 entries -> (first, occ), occ cut at max_occ + 1.
// The build is keys, sort, directory, statistics; none of its kernels uses an atomic.
//
// Query (k_ras_query = k_ra_query_t<true, RasQueryArgs> of realign_kernels.h: one wavefront per sequence, k_ra_query's coding and scoring).  Only the seed stage differs (ras_seeds):
//   look-up     every all-ACGT 20-mer of both orientations at every offset -> occ.  occ > max_occ: the 20-mer is MASKED (bwa mem's -c): no seed, flag
//               SSV_RA_F_MASKED.  Else occ (16 bits) stays in LDS and the 20-mer belongs to class ceil(log2(occ)).
//   admission   classes in ascending order (rare seeds first); inside a class by (strand, query offset, reference position).  A round of 64 offsets takes
//               consecutive slots of the candidate array from a wave prefix sum over the lanes' occ plus the carry of the rounds before; a lane looks its
//               run's first entry up again and copies its positions, which already ascend.  Admission stops at RA_MAX_CAND slots; seeds left out: flag
//               SSV_RA_F_OVERFLOW.  No LDS atomic orders anything: every field of every hit is a function of the input.
//   ties        candidates equal in score, strand and diagonal go to the smaller contig id.
// Still not bwa: one gap per alignment at the most (realign_gap_kernels.h), no chaining beyond a whole read's two pieces (realign_split_kernels.h); one record per query, or up to 1 + 16 when
// the other loci are asked for (realign_alts_kernels.h).
#pragma once

#include "common.h"
#include "radix_sort.h"
#include "realign_kernels.h"

namespace ssv {

constexpr uint64_t RAS_NO_KEY = 1ull << (2 * RA_K); // key of a sampled position that is not indexed: sorts last
constexpr int RAS_KEY_BITS = 2 * RA_K + 1;
constexpr int RAS_MAX_CLASS = 16;                   // ceil(log2(65535))
constexpr uint32_t RAS_F_MASKED = 1, RAS_F_OVERFLOW = 2; // = SSV_RA_F_*

struct RasIndex {
	const uint64_t *keys;     // [sampled positions] sorted; the not indexed ones are the last
	const uint32_t *vals;     // sample numbers, ascending inside a run
	const uint32_t *dir;      // [2^bits + 1]
	int32_t bits;             // directory: top bits of the 40-bit key
	int32_t max_occ;
};

struct RasStats { uint64_t n_distinct, occ_max, n_over_cap; };

// one thread per sampled position
__global__ __launch_bounds__(BLOCK) void k_ras_keys(RaIndex ix, int64_t n, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
	const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (s >= n) return;
	const int64_t p = s * RA_SAMPLE;
	uint64_t key = RAS_NO_KEY;
	if (p + RA_K <= ix.n_bases) {
		const int t = ra_contig_of(ix, p);
		if (p + RA_K <= ix.ctg_off[t + 1]) key = ra_kmer_at(ix.ref, p);
	}
	keys[s] = key;
	vals[s] = (uint32_t)s;
}

// bucket of a 20-mer: its top `bits` bits
__device__ __forceinline__ uint32_t ras_bucket(uint64_t key, int bits) { return (uint32_t)(key >> (2 * RA_K - bits)); }

// One thread per directory slot b = 0 .. 2^bits: the first sorted entry whose key is >= b << (40 - bits), by binary search over all keys (RAS_NO_KEY is
// 2^bits << (40 - bits): the last slot is the number of indexed positions).  The work of a slot does not depend on the sequence: an entry-driven fill
// (the entry that starts a bucket writes the empty slots before it) is cheaper on random sequence, but leaves one thread up to 2^bits writes on a
// low-complexity reference.  Neighbouring slots walk nearly the same keys, so a wavefront's loads fall into few lines.
__global__ __launch_bounds__(BLOCK) void k_ras_dir(const uint64_t *__restrict__ keys, int64_t n, int bits, uint32_t *__restrict__ dir)
{
	const int64_t b = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (b > ((int64_t)1 << bits)) return;
	const uint64_t low = (uint64_t)b << (2 * RA_K - bits);
	int64_t lo = 0, hi = n;
	while (lo < hi) {
		const int64_t m = (lo + hi) >> 1;
		if (keys[m] < low) lo = m + 1; else hi = m;
	}
	dir[b] = (uint32_t)lo;
}

// the end of the run of `km` that starts at `first`, looked for in [first + 1, lim): doubling steps, then a binary search between the last two
__device__ __forceinline__ int64_t ras_run_end(const uint64_t *keys, int64_t first, int64_t lim, uint64_t km)
{
	int64_t lo = first + 1, step = 1; // keys[lo - 1] == km
	while (lo + step <= lim && keys[lo + step - 1] == km) { lo += step; step <<= 1; }
	int64_t hi = lo + step - 1 < lim ? lo + step - 1 : lim; // keys[hi] != km or hi == lim
	while (lo < hi) {
		const int64_t m = (lo + hi) >> 1;
		if (keys[m] == km) lo = m + 1; else hi = m;
	}
	return lo;
}

// Statistics: a block walks RAS_STATS_TILE sorted entries, the first entry of a run measures it.  Every block leaves its sums in part[block];
// k_ras_stats_sum adds them up.
constexpr int RAS_STATS_ROUNDS = 8;
constexpr int RAS_STATS_TILE = BLOCK * RAS_STATS_ROUNDS;

// the threads' figures over the whole block (sums, and the maximum of occ) -> *out, written by thread 0; called by every thread of the block
__device__ __forceinline__ void ras_stats_block(uint64_t distinct, uint64_t occ, uint64_t over, RasStats *out)
{
	__shared__ RasStats s_w[WAVES_PER_BLOCK];
	distinct = wave_sum(distinct); occ = wave_max(occ); over = wave_sum(over);
	if (lane_id() == 0) { s_w[wave_id()].n_distinct = distinct; s_w[wave_id()].occ_max = occ; s_w[wave_id()].n_over_cap = over; }
	__syncthreads();
	if (threadIdx.x == 0) {
		RasStats t = s_w[0];
		for (int w = 1; w < WAVES_PER_BLOCK; ++w) { t.n_distinct += s_w[w].n_distinct; t.occ_max = s_w[w].occ_max > t.occ_max ? s_w[w].occ_max : t.occ_max; t.n_over_cap += s_w[w].n_over_cap; }
		*out = t;
	}
}

__global__ __launch_bounds__(BLOCK) void k_ras_stats(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ n_indexed_p, uint32_t max_occ, RasStats *__restrict__ part)
{
	const int64_t n_indexed = *n_indexed_p; // the directory's last slot: the grid covers every sampled position, the blocks behind the indexed ones leave zeros
	uint64_t distinct = 0, occ = 0, over = 0;
	for (int r = 0; r < RAS_STATS_ROUNDS; ++r) {
		const int64_t i = (int64_t)blockIdx.x * RAS_STATS_TILE + (int64_t)r * BLOCK + threadIdx.x;
		if (i >= n_indexed) break;
		const uint64_t km = keys[i];
		if (i == 0 || keys[i - 1] != km) {
			const uint64_t len = (uint64_t)(ras_run_end(keys, i, n_indexed, km) - i);
			distinct += 1;
			occ = len > occ ? len : occ;
			over += len > max_occ ? 1 : 0;
		}
	}
	ras_stats_block(distinct, occ, over, &part[blockIdx.x]);
}

// one block
__global__ __launch_bounds__(BLOCK) void k_ras_stats_sum(const RasStats *__restrict__ part, int64_t n_part, RasStats *__restrict__ out)
{
	uint64_t distinct = 0, occ = 0, over = 0;
	for (int64_t i = threadIdx.x; i < n_part; i += BLOCK) { distinct += part[i].n_distinct; occ = part[i].occ_max > occ ? part[i].occ_max : occ; over += part[i].n_over_cap; }
	ras_stats_block(distinct, occ, over, out);
}

// first sorted entry of the 20-mer km, or -1
__device__ __forceinline__ int64_t ras_first(const RasIndex &sx, uint64_t km)
{
	const uint32_t b = ras_bucket(km, sx.bits);
	int64_t lo = sx.dir[b], hi = sx.dir[b + 1];
	while (lo < hi) {
		const int64_t m = (lo + hi) >> 1;
		if (sx.keys[m] < km) lo = m + 1; else hi = m;
	}
	return lo < (int64_t)sx.dir[b + 1] && sx.keys[lo] == km ? lo : -1;
}

// occurrences of km, cut at max_occ + 1
__device__ __forceinline__ uint32_t ras_occ(const RasIndex &sx, uint64_t km)
{
	const int64_t first = ras_first(sx, km);
	if (first < 0) return 0;
	const int64_t all = sx.dir[(size_t)1 << sx.bits]; // the indexed entries
	const int64_t lim = first + sx.max_occ + 1 < all ? first + sx.max_occ + 1 : all;
	return (uint32_t)(ras_run_end(sx.keys, first, lim, km) - first);
}

__device__ __forceinline__ int ras_class(uint32_t occ) { return occ <= 1 ? 0 : 32 - __clz((int)(occ - 1)); }

struct RasQueryArgs : RaQueryArgs { // ix: the reference and its contigs (table and mask unused)
	RasIndex sx;
};
static_assert(sizeof(RasQueryArgs) == sizeof(RaQueryArgs) + sizeof(RasIndex), "the sorted index lies right behind the base's fields");

constexpr int RAS_MAX_OFF = RA_MAX_Q - RA_K + 1; // 20-mer offsets of the longest query

// The seed stage of k_ra_query_t<true> (realign_kernels.h): look-up and admission as described at the top of this file, for the query of n bases whose codes
// are in s_code[w].  Fills the wavefront's candidate arrays, sets *flags (every lane holds the same value) and returns the number of candidates.
__device__ __forceinline__ int ras_seeds(const RasQueryArgs &a, int w, int lane, int n, const uint8_t (&s_code)[WAVES_PER_BLOCK][2][RA_MAX_Q], int64_t (&s_diag)[WAVES_PER_BLOCK][RA_MAX_CAND],
                                         uint16_t (&s_ss)[WAVES_PER_BLOCK][RA_MAX_CAND], int32_t (&s_tid)[WAVES_PER_BLOCK][RA_MAX_CAND], uint8_t *flags)
{
	__shared__ uint16_t s_occ[WAVES_PER_BLOCK][2][RAS_MAX_OFF + 3]; // occurrences of the 20-mer at (strand, offset); 0: no seed (not ACGT, absent or masked)
	const RasIndex &sx = a.sx;
	// ---- look-up: occurrences of every 20-mer ----
	const int n_off = n - RA_K + 1;
	uint32_t masked = 0, classes = 0, total = 0;
	for (int st = 0; st < 2; ++st) {
		for (int o = lane; o < n_off; o += WAVE) {
			bool ok;
			const uint64_t km = ra_kmer(s_code[w][st], o, &ok);
			uint32_t occ = ok ? ras_occ(sx, km) : 0u;
			if (occ > (uint32_t)sx.max_occ) { masked = 1; occ = 0; }
			s_occ[w][st][o] = (uint16_t)occ;
			if (occ) { classes |= 1u << ras_class(occ); total += occ; }
		}
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) { masked |= __shfl_xor(masked, d, 64); classes |= __shfl_xor(classes, d, 64); }
	total = wave_sum(total);
	*flags = (uint8_t)((masked ? RAS_F_MASKED : 0u) | (total > (uint32_t)RA_MAX_CAND ? RAS_F_OVERFLOW : 0u));
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
	// ---- admission: rarest class first; (strand, offset, position) inside a class ----
	uint32_t filled = 0; // wave-uniform
	for (int cl = 0; cl <= RAS_MAX_CLASS && filled < (uint32_t)RA_MAX_CAND; ++cl) {
		if (!((classes >> cl) & 1u)) continue;
		for (int st = 0; st < 2 && filled < (uint32_t)RA_MAX_CAND; ++st) {
			for (int ob = 0; ob < n_off && filled < (uint32_t)RA_MAX_CAND; ob += WAVE) {
				const int o = ob + lane;
				uint32_t occ = o < n_off ? s_occ[w][st][o] : 0u;
				if (occ && ras_class(occ) != cl) occ = 0;
				const uint32_t inc = wave_inclusive_sum(occ);
				const uint32_t at = filled + inc - occ;
				if (occ && at < (uint32_t)RA_MAX_CAND) {
					bool ok;
					const int64_t first = ras_first(sx, ra_kmer(s_code[w][st], o, &ok));
					const uint32_t take = occ < (uint32_t)RA_MAX_CAND - at ? occ : (uint32_t)RA_MAX_CAND - at;
					for (uint32_t j = 0; j < take; ++j) {
						const int64_t p = (int64_t)sx.vals[first + j] * RA_SAMPLE;
						s_diag[w][at + j] = p - o; s_ss[w][at + j] = (uint16_t)(st << 15); s_tid[w][at + j] = ra_contig_of(a.ix, p);
					}
				}
				filled += __shfl(inc, 63, 64);
			}
		}
	}
	return filled < (uint32_t)RA_MAX_CAND ? (int)filled : RA_MAX_CAND;
}

constexpr auto k_ras_query = k_ra_query_t<true, RasQueryArgs>;
constexpr auto k_ras_query_floor = k_ra_query_t<true, RasQueryArgs, RA_K>; // the gapped query's first stage

} // namespace ssv
