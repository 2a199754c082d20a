// retained.h - what the kernels that write a retained batch share: the destination's seven parts, the look-up of a record's input batch,
// the two size rules, and the two routines that write one output record.  Used by dup_kernels.h, sort_kernels.h and pairdup_kernels.h; the host's side of
// the same form is RetainedSlab (seeksv_hip.hip).
#pragma once

#include "common.h"
#include "clip_kernels.h"

namespace ssv {

constexpr int RET_SUB = 16; // lanes per record in the kernels that write records

// the seven parts of a retained batch (or of any set of buffers laid out like one: ssv_dup_retain's hold-back)
struct RetDst { int32_t *tid, *pos; uint16_t *n_cigar; uint8_t *ends; ssv_record *rec; uint32_t *cigar; uint8_t *seqqual; };

// A table of batches taken as one sequence (entries with .start: where the batch's records begin in it): the batch that holds record g is the last one that
// starts at or below g (empty batches share their start with the one behind them; src[0].start == 0)
template <typename Src> __device__ __forceinline__ int src_find(const Src *__restrict__ src, int n_src, int64_t g)
{
	int lo = 0, hi = n_src;
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (src[mid].start <= g) lo = mid; else hi = mid;
	}
	return lo;
}

// bases + qualities of a read of lq >= 0 bases, packed as the decoders pack them: ceil(lq / 2) + lq bytes, no padding between records
__device__ __forceinline__ uint32_t seq_bytes(int lq) { return (uint32_t)((lq + 1) / 2 + lq); }
// the ends byte (first | last << 4 operation code, 0xff without CIGAR) says soft-clipped at either end
__device__ __forceinline__ bool ends_clipped(uint8_t e) { return e != 0xff && ((e & 15) == C_S || (e >> 4) == C_S); }

// output record d, by one lane: the hot columns, the ends byte, and the line as it was but for its flag word and its two offsets into dst's own arrays.
// (The ends byte comes by address and is loaded where it is stored: handed over as a value, k_sort_gather compiles to 48 VGPRs for the 42 it had with
// this text inline - DESIGN.md 8e.)
__device__ __forceinline__ void ret_write_record(const RetDst &dst, int64_t d, const RecLine &r, const uint8_t *ends_at, uint32_t fmx, uint32_t cigar_off, uint64_t seq_off)
{
	dst.tid[d] = r.tid(); dst.pos[d] = r.pos(); dst.n_cigar[d] = (uint16_t)r.n_cigar(); dst.ends[d] = *ends_at;
	uint4 *p = reinterpret_cast<uint4 *>(dst.rec + d);
	p[0] = make_uint4(r.w_tid, r.w_pos, fmx, r.w_nc);
	p[1] = make_uint4(r.w_lq, r.w_mtid, r.w_mpos, r.w_isize);
	p[2] = make_uint4(cigar_off, r.h0, r.h1, r.h2);
	p[3] = make_uint4(r.h3, r.h4, (uint32_t)seq_off, (uint32_t)(seq_off >> 32));
}

// the variable parts of one record, by its RET_SUB lanes in turn: its operations to dst.cigar + cigar_off, `sb` bytes of bases + qualities to dst.seqqual + seq_off
__device__ __forceinline__ void ret_copy_parts(const RetDst &dst, const RecLine &r, const uint32_t *cigar, const uint8_t *seqqual, int sub, uint32_t cigar_off, uint64_t seq_off, uint32_t sb)
{
	const int nc = r.n_cigar();
	for (int j = sub; j < nc; j += RET_SUB) dst.cigar[cigar_off + (uint32_t)j] = r.op(cigar, j);
	if (sb) {
		const uint8_t *s = seqqual + r.seq_off();
		for (uint32_t j = (uint32_t)sub; j < sb; j += RET_SUB) dst.seqqual[seq_off + j] = s[j];
	}
}

} // namespace ssv
