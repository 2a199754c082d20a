// dup_kernels.h - `run -M`: duplicate read pairs marked while the sample is retained (the rule: include/seeksv_hip.h, ssv_dup_retain).
// select (streaming: the hot columns tid / pos, 8 bytes a record: records whose run has a neighbour; where the trailing run starts; is the input sorted) ->
// keys of the selected records (16 lanes a record: quality sum, digest of name + positions) -> groups (one wavefront per run, all pairs in tiles of 64 across
// the lanes) -> digests of the marked heads into an open-addressing set -> tails probe it -> gather: the settled records into the retained batch (bases and
// qualities of the soft-clipped ones only), the trailing run into the hold-back.  Counts are sums of per-record / per-wavefront words (scan.h): the only
// atomics are the 64-bit compare-and-swaps of the set.
#pragma once

#include "common.h"
#include "clip_kernels.h"
#include "retained.h"

namespace ssv {

enum : int { F_READ1 = 64, F_SUPPLEMENTARY = 2048 };
constexpr uint64_t FNV_OFFSET = 1469598103934665603ull, FNV_PRIME = 1099511628211ull; // (as k_rt_measure)
constexpr int DUP_SUB = RET_SUB;                  // lanes per record in the per-record kernels
constexpr int DUP_PER_BLOCK = BLOCK / DUP_SUB;

// the records a call works on: the run held back by the call before (a), then the new batch (b); n = a.n + b.n
struct DupView { DevBatch a, b; DevNames na, nb; int64_t n; };

// record i of the view: its arrays and its index in them (picked field by field: no pointer into the kernel's arguments)
struct DupRef {
	const ssv_record *rec; const uint32_t *cigar; const uint8_t *seqqual; const uint8_t *ends; const uint16_t *n_cigar;
	const char *nbase; const uint64_t *noff; int64_t nbias; int64_t j;
};
__device__ __forceinline__ DupRef dup_ref(const DupView &v, int64_t i)
{
	const bool a = i < v.a.n;
	DupRef r;
	r.rec = a ? v.a.rec : v.b.rec; r.cigar = a ? v.a.cigar : v.b.cigar; r.seqqual = a ? v.a.seqqual : v.b.seqqual; r.ends = a ? v.a.ends : v.b.ends;
	r.n_cigar = a ? v.a.n_cigar : v.b.n_cigar; r.nbase = a ? v.na.base : v.nb.base; r.noff = a ? v.na.off : v.nb.off; r.nbias = a ? v.na.bias : v.nb.bias;
	r.j = a ? i : i - v.a.n;
	return r;
}
__device__ __forceinline__ int2 dup_pos(const DupView &v, int64_t i)
{
	const bool a = i < v.a.n;
	const int64_t j = a ? i : i - v.a.n;
	return make_int2((a ? v.a.tid : v.b.tid)[j], (a ? v.a.pos : v.b.pos)[j]);
}
__device__ __forceinline__ bool same_pos(int2 x, int2 y) { return x.x == y.x && x.y == y.y; }

__device__ __forceinline__ bool dup_takes_part(int flag, int tid, int mtid)
{
	return (flag & F_PAIRED) && !(flag & (F_UNMAP | F_MUNMAP | F_SECONDARY | F_SUPPLEMENTARY | F_DUP)) && tid >= 0 && mtid >= 0;
}
__device__ __forceinline__ bool dup_is_head(int flag, int tid, int pos, int mtid, int mpos)
{
	return tid < mtid || (tid == mtid && (pos < mpos || (pos == mpos && (flag & F_READ1))));
}

// FNV-1a over the name without its NUL, then over four little-endian int32
__device__ __forceinline__ uint64_t dup_digest(const char *name, int a, int b, int c, int d, uint64_t mask)
{
	uint64_t h = FNV_OFFSET;
	for (int len = 0; len < 255; ++len) {
		const uint8_t ch = (uint8_t)name[len];
		if (!ch) break;
		h = (h ^ ch) * FNV_PRIME;
	}
	const uint32_t w[4] = {(uint32_t)a, (uint32_t)b, (uint32_t)c, (uint32_t)d};
#pragma unroll
	for (int k = 0; k < 4; ++k)
#pragma unroll
		for (int j = 0; j < 4; ++j) h = (h ^ ((w[k] >> (8 * j)) & 0xffu)) * FNV_PRIME;
	return h & mask;
}

// ---- select ----
// sel[i] = record i has tid >= 0 and its run has at least two records.  wave_break[w] = the last record of wavefront w whose (tid, pos) is not the view's last one (-1: none):
// the trailing run starts behind the last such record.  *unsorted = 1 when (tid, pos) goes down between two neighbours with tid >= 0.
__global__ __launch_bounds__(BLOCK) void k_dup_select(DupView v, uint32_t *__restrict__ sel, int32_t *__restrict__ wave_break, uint32_t *__restrict__ unsorted)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	const int lane = lane_id();
	const bool in = i < v.n;
	const int2 last = dup_pos(v, v.n - 1);
	const int2 k = in ? dup_pos(v, i) : last;
	int2 pk, nk;
	pk.x = __shfl_up(k.x, 1, 64); pk.y = __shfl_up(k.y, 1, 64);
	nk.x = __shfl_down(k.x, 1, 64); nk.y = __shfl_down(k.y, 1, 64);
	const bool has_prev = in && i > 0, has_next = i + 1 < v.n;
	if (lane == 0 && has_prev) pk = dup_pos(v, i - 1);
	if (lane == 63 && has_next) nk = dup_pos(v, i + 1);
	if (in) sel[i] = k.x >= 0 && ((has_prev && same_pos(pk, k)) || (has_next && same_pos(nk, k))); // (unplaced records take no part: the tail of a file is millions of them at (-1, -1))
	if (has_prev && k.x >= 0 && pk.x >= 0 && (k.x < pk.x || (k.x == pk.x && k.y < pk.y))) *unsorted = 1u;
	const uint64_t bal = __ballot(in && !same_pos(k, last));
	if (lane == 0) wave_break[i >> 6] = bal ? (int32_t)(i + 63 - __clzll((long long)bal)) : -1;
}

// one wavefront: out[0] = where the trailing run starts (n when the last record has tid < 0: such records take no part and are not held back)
__global__ __launch_bounds__(WAVE) void k_dup_cut(DupView v, const int32_t *__restrict__ wave_break, int64_t n_waves, uint32_t *__restrict__ out)
{
	const int lane = lane_id();
	int64_t cut = 0;
	if (dup_pos(v, v.n - 1).x < 0) cut = v.n;
	else
		for (int64_t top = n_waves; top > 0; top -= WAVE) { // from the end: the answer is in the first round unless the run is longer than 4096 records
			const int64_t w = top - 1 - lane;
			const int32_t b = w >= 0 ? wave_break[w] : -1;
			const uint64_t bal = __ballot(b >= 0);
			if (bal) { cut = (int64_t)__shfl(b, __ffsll((long long)bal) - 1, 64) + 1; break; }
		}
	if (lane == 0) out[0] = (uint32_t)cut;
}

// rs[k] = selected record k starts a run (the selected records of a run follow each other in cand[])
__global__ __launch_bounds__(BLOCK) void k_dup_run_starts(DupView v, const uint32_t *__restrict__ cand, int64_t m, uint32_t *__restrict__ rs)
{
	const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (k >= m) return;
	rs[k] = k == 0 || cand[k] != cand[k - 1] + 1u || !same_pos(dup_pos(v, cand[k]), dup_pos(v, cand[k - 1]));
}

// ---- keys ----
struct DupKey {
	int32_t mtid, mpos;
	uint32_t score;
	uint32_t kind;     // 0: takes no part (or lies in the trailing run); 1 | flag & 0x30: head; 2: tail
	uint64_t digest;
};

// the quality sum of one record, its lanes taking consecutive bytes in turn (DUP_SUB lanes; every lane gets the sum)
__device__ __forceinline__ uint32_t dup_score(const uint8_t *seqqual, uint64_t seq_off, int lq, int sub)
{
	uint32_t s = 0;
	bool none = lq <= 0 || seq_off == SSV_NO_SEQ;
	if (!none) {
		const uint8_t *q = seqqual + seq_off + (uint64_t)((lq + 1) >> 1);
		none = q[0] == 0xff;
		if (!none) for (int j = sub; j < lq; j += DUP_SUB) { const uint32_t x = q[j]; s += x >= 15u ? x : 0u; }
	}
#pragma unroll
	for (int d = DUP_SUB / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d, DUP_SUB);
	return none ? 0u : s;
}

// 16 lanes per selected record: a head's quality sum by all of them, the digest (a sequential hash) by the first
__global__ __launch_bounds__(BLOCK) void k_dup_keys(DupView v, const uint32_t *__restrict__ cand, int64_t m, int64_t cut, uint64_t mask, DupKey *__restrict__ keys)
{
	const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	const int64_t k = t / DUP_SUB;
	const int sub = (int)(t & (DUP_SUB - 1));
	const bool in = k < m && (int64_t)cand[k < m ? k : 0] < cut;
	DupKey key{0, 0, 0u, 0u, 0ull};
	const uint8_t *sq = nullptr; uint64_t so = SSV_NO_SEQ; int lq = 0;
	const char *name = nullptr;
	int tid = 0, pos = 0;
	if (in) {
		const DupRef f = dup_ref(v, cand[k]);
		const RecLine r = rec_load(f.rec, f.j);
		tid = r.tid(); pos = r.pos(); key.mtid = r.mtid(); key.mpos = r.mpos();
		if (dup_takes_part(r.flag(), tid, key.mtid)) {
			const bool head = dup_is_head(r.flag(), tid, pos, key.mtid, key.mpos);
			key.kind = head ? 1u | (uint32_t)(r.flag() & (F_REV | F_MREV)) : 2u;
			if (head) { sq = f.seqqual; so = r.seq_off(); lq = r.l_qseq(); }
			name = f.nbase + f.noff[f.j] + f.nbias;
		}
	}
	key.score = dup_score(sq, so, lq, sub); // (every lane of the wavefront takes part in its shuffles)
	if (!in || sub != 0) return;
	if (key.kind) key.digest = (key.kind & 3u) == 1u ? dup_digest(name, tid, pos, key.mtid, key.mpos, mask) : dup_digest(name, key.mtid, key.mpos, tid, pos, mask);
	keys[k] = key;
}

// ---- groups ----
// One wavefront per run of selected records [rfirst[r], rfirst[r + 1]): every head asks whether a head with an equal key has a higher score, or an equal
// score and an earlier index.  Its own 64 records sit one per lane; the others come by in tiles of 64, one per lane, and are handed round by lane index.
// All pairs among the HEADS, not a sort: tiles without a head are passed over, so a run of R records with H heads costs about R / 64 * (R / 64 + H) steps of one
// wavefront - 16 K for R = H = 1000 - and deep runs of heads are rare; 10^5 heads at one position (an amplicon) are 1.6 * 10^8 steps, seconds, on one wavefront.
// rstart[k] = the run's first record; isdup[k] / keeper[k] = 1 for a marked head / for the one head of a group that stays; mark[i] = 1 for a marked head.
__global__ __launch_bounds__(BLOCK) void k_dup_groups(const DupKey *__restrict__ keys, const uint32_t *__restrict__ cand, const uint32_t *__restrict__ rfirst, int64_t n_runs, int64_t m,
                                                      int64_t cut, uint32_t *__restrict__ rstart, uint32_t *__restrict__ isdup, uint32_t *__restrict__ keeper, uint8_t *__restrict__ mark)
{
	const int64_t r = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave_id();
	if (r >= n_runs) return;
	const int lane = lane_id();
	const int64_t r0 = rfirst[r], r1 = r + 1 < n_runs ? (int64_t)rfirst[r + 1] : m;
	const uint32_t first = cand[r0];
	if ((int64_t)first >= cut) return; // the trailing run: next call
	for (int64_t a0 = r0; a0 < r1; a0 += WAVE) {
		const int64_t ka = a0 + lane;
		const bool have = ka < r1;
		DupKey mine{0, 0, 0u, 0u, 0ull};
		if (have) mine = keys[ka];
		const bool head = (mine.kind & 3u) == 1u;
		bool beaten = false;
		// (a tile of 64 without a head asks nothing and answers nothing: a deep pile of records that take no part costs one look at each record's kind)
		const bool asks = __ballot(head) != 0ull;
		for (int64_t b0 = r0; asks && b0 < r1; b0 += WAVE) {
			const int64_t kb = b0 + lane;
			uint32_t kind_o = 0u;
			if (kb < r1) kind_o = keys[kb].kind;
			uint64_t heads = __ballot((kind_o & 3u) == 1u);
			if (heads == 0ull) continue;
			DupKey o{0, 0, 0u, 0u, 0ull};
			if (kb < r1) o = keys[kb];
			for (; heads; heads &= heads - 1ull) { // the heads of the other tile, one after the other (the same for every lane)
				const int s = __ffsll((long long)heads) - 1;
				const uint32_t okind = __shfl(o.kind, s, 64);
				const int omtid = __shfl(o.mtid, s, 64), ompos = __shfl(o.mpos, s, 64);
				const uint32_t oscore = __shfl(o.score, s, 64);
				if (head && okind == mine.kind && omtid == mine.mtid && ompos == mine.mpos && (oscore > mine.score || (oscore == mine.score && b0 + s < ka))) beaten = true;
			}
		}
		if (have) {
			rstart[ka] = first;
			isdup[ka] = head && beaten;
			keeper[ka] = head && !beaten;
			if (head && beaten) mark[cand[ka]] = 1;
		}
	}
}

// ---- the digest set: open addressing, linear probing, at most half full; keys[slots] / when[slots] stand for the digest 0 (0 is "empty" elsewhere) ----
struct DupSet { uint64_t *keys; uint64_t *when; uint64_t mask; int shift; }; // slots = mask + 1 = 2^(64 - shift); when: the earliest run (its first record, file order) that put the digest in

__device__ __forceinline__ uint64_t dup_cas(uint64_t *p, uint64_t expect, uint64_t val)
{
	return (uint64_t)atomicCAS(reinterpret_cast<unsigned long long *>(p), (unsigned long long)expect, (unsigned long long)val);
}
__device__ __forceinline__ uint64_t dup_slot(const DupSet &S, uint64_t d) { return (d * 0x9E3779B97F4A7C15ull) >> S.shift; }

// true: the digest was not there before
__device__ __forceinline__ bool dup_set_insert(const DupSet &S, uint64_t d, uint64_t when)
{
	uint64_t s;
	bool won;
	if (d == 0) { s = S.mask + 1; won = dup_cas(&S.keys[s], 0ull, 1ull) == 0ull; }
	else
		for (s = dup_slot(S, d);; s = (s + 1) & S.mask) {
			const uint64_t old = dup_cas(&S.keys[s], 0ull, d);
			won = old == 0ull;
			if (won || old == d) break;
		}
	uint64_t cur = dup_cas(&S.when[s], ~0ull, when); // the minimum, by compare-and-swap
	while (when < cur) { const uint64_t prev = dup_cas(&S.when[s], cur, when); if (prev == cur) break; cur = prev; }
	return won;
}

// (in a kernel behind the inserts: plain loads)
__device__ __forceinline__ bool dup_set_find(const DupSet &S, uint64_t d, uint64_t *when)
{
	uint64_t s;
	if (d == 0) { s = S.mask + 1; if (S.keys[s] == 0ull) return false; }
	else
		for (s = dup_slot(S, d);; s = (s + 1) & S.mask) {
			const uint64_t k = S.keys[s];
			if (k == 0ull) return false;
			if (k == d) break;
		}
	*when = S.when[s];
	return true;
}

__global__ __launch_bounds__(BLOCK) void k_dup_insert(DupSet S, const DupKey *__restrict__ keys, const uint32_t *__restrict__ isdup, const uint32_t *__restrict__ rstart, int64_t m,
                                                      uint64_t rec_base, uint32_t *__restrict__ fresh)
{
	const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (k >= m) return;
	fresh[k] = isdup[k] ? (uint32_t)dup_set_insert(S, keys[k].digest, rec_base + rstart[k]) : 0u;
}

// the set into one of twice the size
__global__ __launch_bounds__(BLOCK) void k_dup_rehash(DupSet from, DupSet to)
{
	const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (s > from.mask + 1) return;
	const uint64_t k = from.keys[s];
	if (k == 0ull) return;
	if (s == from.mask + 1) { to.keys[to.mask + 1] = 1ull; to.when[to.mask + 1] = from.when[s]; }
	else dup_set_insert(to, k, from.when[s]);
}

// ---- tails ----
// One lane per settled record (two quarters of its line): a tail that takes part computes its head's digest and asks the set; found, and put there by a run
// that is not later than its own: marked.  Runs only while the set holds something.  wave_cnt[w] = tails marked by wavefront w.
__global__ __launch_bounds__(BLOCK) void k_dup_tails(DupView v, int64_t cut, DupSet S, uint64_t mask, uint64_t rec_base, const uint32_t *__restrict__ sel, const uint32_t *__restrict__ at,
                                                     const uint32_t *__restrict__ rstart, uint8_t *__restrict__ mark, uint32_t *__restrict__ wave_cnt)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	bool hit = false;
	if (i < cut) {
		const DupRef f = dup_ref(v, i);
		const uint4 *p = reinterpret_cast<const uint4 *>(f.rec + f.j);
		const uint4 a = p[0], b = p[1];
		const int tid = (int)a.x, pos = (int)a.y, flag = (int)(a.z & 0xffffu), mtid = (int)b.y, mpos = (int)b.z;
		if (dup_takes_part(flag, tid, mtid) && !dup_is_head(flag, tid, pos, mtid, mpos)) {
			const uint64_t d = dup_digest(f.nbase + f.noff[f.j] + f.nbias, mtid, mpos, tid, pos, mask);
			uint64_t when;
			if (dup_set_find(S, d, &when)) {
				const uint64_t run = rec_base + (sel[i] ? (uint64_t)rstart[at[i]] : (uint64_t)i);
				hit = when <= run;
			}
		}
		if (hit) mark[i] = 1;
	}
	const uint64_t bal = __ballot(hit);
	if (lane_id() == 0) wave_cnt[((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6] = (uint32_t)__popcll(bal);
}

// ---- sizes and gather ----
// What record i takes in the batch it goes to - settled records (i < cut) into the retained batch: all operations, bases + qualities when the first or the
// last operation is S; the trailing run into the hold-back: all operations, its bases + qualities, its name.  *bad = 1: a record that takes part came
// without its qualities.  wave_part[w] = settled records of wavefront w that take part.
__global__ __launch_bounds__(BLOCK) void k_dup_sizes(DupView v, int64_t cut, uint32_t *__restrict__ cig_n, uint32_t *__restrict__ seq_b, uint32_t *__restrict__ name_b,
                                                     uint32_t *__restrict__ wave_part, uint32_t *__restrict__ bad)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	bool part = false;
	if (i < v.n) {
		const DupRef f = dup_ref(v, i);
		const RecLine r = rec_load(f.rec, f.j);
		const int lq = r.l_qseq() > 0 ? r.l_qseq() : 0;
		const bool has = r.seq_off() != SSV_NO_SEQ;
		part = dup_takes_part(r.flag(), r.tid(), r.mtid());
		if (part && !has && lq > 0) *bad = 1u;
		const bool clipped = ends_clipped(f.ends[f.j]);
		cig_n[i] = (uint32_t)r.n_cigar();
		seq_b[i] = has && (i >= cut || clipped) ? seq_bytes(lq) : 0u;
		uint32_t nb = 0;
		if (i >= cut) {
			const char *p = f.nbase + f.noff[f.j] + f.nbias;
			while (nb < 255 && p[nb]) ++nb;
			++nb; // the NUL
		}
		name_b[i] = nb;
		part = part && i < cut;
	}
	const uint64_t bal = __ballot(part);
	if (lane_id() == 0) wave_part[((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6] = (uint32_t)__popcll(bal);
}

struct DupDst : RetDst {
	char *names; uint64_t *name_off; // the hold-back only (NULL: no names)
};

// 16 lanes per record: records [first, first + count) of the view into dst - the first lane the hot columns and the line (flag | 0x400 where marked, offsets
// into dst's own arrays), all of them the operations, the bytes of bases + qualities, the name
__global__ __launch_bounds__(BLOCK) void k_dup_gather(DupView v, int64_t first, int64_t count, const uint8_t *__restrict__ mark, const uint32_t *__restrict__ cig_at,
                                                      const uint64_t *__restrict__ seq_at, const uint32_t *__restrict__ seq_b, const uint64_t *__restrict__ name_at,
                                                      const uint32_t *__restrict__ name_b, int seq_only_clipped, DupDst dst)
{
	const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	const int64_t d = t / DUP_SUB;
	const int sub = (int)(t & (DUP_SUB - 1));
	if (d >= count) return;
	const int64_t i = first + d;
	const DupRef f = dup_ref(v, i);
	const RecLine r = rec_load(f.rec, f.j);
	const uint32_t coff = cig_at[i], sb = seq_b[i];
	const uint64_t soff = seq_at[i];
	const uint8_t e = f.ends[f.j];
	if (sub == 0) {
		const bool keep = r.seq_off() != SSV_NO_SEQ && (!seq_only_clipped || ends_clipped(e));
		ret_write_record(dst, d, r, &e, r.w_fmx | (mark && mark[i] ? (uint32_t)F_DUP : 0u), coff, keep ? soff : SSV_NO_SEQ);
		if (dst.name_off) dst.name_off[d] = name_at[i];
	}
	ret_copy_parts(dst, r, f.cigar, f.seqqual, sub, coff, soff, sb);
	if (dst.names) {
		const char *pn = f.nbase + f.noff[f.j] + f.nbias;
		const uint32_t nb = name_b[i];
		const uint64_t no = name_at[i];
		for (uint32_t j = (uint32_t)sub; j + 1 < nb; j += DUP_SUB) dst.names[no + j] = pn[j];
		if (sub == 0) dst.names[no + nb - 1] = 0;
	}
}

} // namespace ssv
