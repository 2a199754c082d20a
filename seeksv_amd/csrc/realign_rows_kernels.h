// realign_rows_kernels.h - the split query's reads, hits and mates as a device batch (ssv_realign_split_batch; `seeksv run -P`).
//
// `seeksv realign -P` builds its BAM records on the host, base by base, from hits it has downloaded; getsv -F then decodes them again.  Here the records are
// written where the reads and the hits lie already, in the layout the device decoders hand out (hot columns, cigar_ends, 64-byte lines, operations, packed
// bases + qualities), so that ssv_rt_scan takes them in place.
//
//   rows       read i gives one record, and a second one directly behind it when mates[i].tid >= 0; row order is read order.
//   fields     flag 0 / 16 / 4, | 2048 on the mate's record; mapq the hit's (0 unaligned); tid / pos the hit's or -1 / -1; l_qseq = L; mtid = mpos = -1;
//              isize = 0; xc = 0.  CIGAR: q_beg S (when > 0), (q_end - q_beg) M, (L - q_end) S (when > 0); none, and cigar_ends 0xff, when unaligned.
//   bases      A C G T in either case 1 2 4 8, every other byte 15; a reverse-strand record holds the reversed complement (nibble bits mirrored) and the
//              reversed qualities; an odd L leaves the last byte's low nibble 0.  Qualities: byte - 33, or 0xff throughout without a quality blob.
//   seqqual    a record's block is [ceil(L / 2) packed bytes | L qualities], zero padded to whole dwords: every block starts dword aligned.
//   k_rr_sizes a lane per read: records, operations and seqqual bytes of the read; three exclusive scans give where they go.
//   k_rr_rows  a wavefront per read.  Lane 0 writes the columns, lane 1 the line, lanes 2..4 the operations, per record.  The block is written as dwords:
//              lane d % 64 builds dword d - eight consecutive bases as nibbles, or four qualities, or (one dword per record at the most) the bytes around the
//              seam between the two.  A dword whose source bytes all lie inside the read is built from one unaligned 8- or 4-byte load; the others byte by
//              byte, under a bound: no byte outside the read is loaded.  1,024 bases are 384 dwords: six rounds of the wavefront.
// Plain C++ stores; no atomics, no LDS, no scratch.
#pragma once

#include "batch_columns.h"
#include "common.h"
#include "realign_kernels.h"
#include "seeksv_hip.h"

namespace ssv {

struct RaRowsArgs {
	const char *seqs;          // the reads, back to back (16 readable bytes behind them)
	const char *quals;         // nullptr, or their qualities at the same offsets
	const uint64_t *seq_off;   // [n + 1]
	const uint64_t *name_off;  // [n + 1] into the name blob
	const RaHit *hits, *mates; // [n]
	int64_t n;
	const uint32_t *row_at, *op_at; // [n] the read's first record / operation
	const uint64_t *sq_at;     // [n] the read's first seqqual byte
};

__device__ __forceinline__ uint32_t rr_ops(const RaHit &h, uint32_t L) { return h.tid >= 0 ? 1u + (h.q_beg > 0 ? 1u : 0u) + ((uint32_t)h.q_end < L ? 1u : 0u) : 0u; }
__device__ __forceinline__ uint32_t rr_block(uint32_t L) { return ((L + 1u) / 2u + L + 3u) & ~3u; }

__global__ __launch_bounds__(BLOCK) void k_rr_sizes(const uint64_t *__restrict__ seq_off, const RaHit *__restrict__ hits, const RaHit *__restrict__ mates, int64_t n,
                                                   uint32_t *__restrict__ n_rows, uint32_t *__restrict__ n_ops, uint32_t *__restrict__ n_bytes)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n) return;
	const uint32_t L = (uint32_t)(seq_off[i + 1] - seq_off[i]);
	const RaHit h = hits[i], m = mates[i];
	const uint32_t rows = m.tid >= 0 ? 2u : 1u;
	n_rows[i] = rows;
	n_ops[i] = rr_ops(h, L) + (rows == 2u ? rr_ops(m, L) : 0u);
	n_bytes[i] = rows * rr_block(L);
}

// BAM's 4-bit code of a base, of its complement when `rev`
__device__ __forceinline__ uint32_t rr_code(uint32_t ch, bool rev)
{
	const uint32_t u = ch & 0xdfu;
	uint32_t v = 15u;
	v = u == 'A' ? (rev ? 8u : 1u) : v;
	v = u == 'C' ? (rev ? 4u : 2u) : v;
	v = u == 'G' ? (rev ? 2u : 4u) : v;
	v = u == 'T' ? (rev ? 1u : 8u) : v;
	return v;
}

// byte k of a record's block: packed bases below nb, qualities from there, 0 behind the last one
__device__ __forceinline__ uint32_t rr_byte(const char *__restrict__ s, const char *__restrict__ q, uint32_t L, uint32_t nb, bool rev, uint32_t k)
{
	if (k < nb) {
		const uint32_t j = 2u * k;
		const uint32_t hi = rr_code((uint8_t)s[rev ? L - 1u - j : j], rev);
		const uint32_t lo = j + 1u < L ? rr_code((uint8_t)s[rev ? L - 2u - j : j + 1u], rev) : 0u;
		return hi << 4 | lo;
	}
	const uint32_t j = k - nb;
	if (j >= L) return 0u;
	return q ? ((uint32_t)(uint8_t)q[rev ? L - 1u - j : j] - 33u) & 0xffu : 0xffu;
}

__global__ __launch_bounds__(BLOCK) void k_rr_rows(RaRowsArgs a, DecodedCols c, ssv_record *__restrict__ rec, uint64_t *__restrict__ row_name)
{
	const int64_t i = (int64_t)blockIdx.x * WAVES_PER_BLOCK + __builtin_amdgcn_readfirstlane(wave_id());
	if (i >= a.n) return;
	const int lane = lane_id();
	const uint64_t so = a.seq_off[i];
	const uint32_t L = (uint32_t)(a.seq_off[i + 1] - so), nb = (L + 1u) / 2u, blk = rr_block(L);
	const char *s = a.seqs + so, *q = a.quals ? a.quals + so : nullptr;
	const RaHit h0 = a.hits[i], h1 = a.mates[i];
	const uint32_t rows = h1.tid >= 0 ? 2u : 1u, row0 = a.row_at[i], ops0 = rr_ops(h0, L);
	for (uint32_t r = 0; r < rows; ++r) {
		const RaHit h = r ? h1 : h0;
		const bool al = h.tid >= 0, rev = al && h.reverse;
		const uint32_t row = row0 + r, nc = r ? rr_ops(h1, L) : ops0, coff = a.op_at[i] + (r ? ops0 : 0u);
		const uint64_t soff = a.sq_at[i] + (uint64_t)r * blk;
		const int32_t tid = al ? h.tid : -1, pos = al ? h.pos : -1;
		const uint32_t flag = (al ? (rev ? 16u : 0u) : 4u) | (r ? 2048u : 0u), mapq = al ? h.mapq : 0u;
		// the operations: [q_beg S] M [tail S]
		const bool head = al && h.q_beg > 0;
		const uint32_t tail = al ? L - (uint32_t)h.q_end : 0u;
		const uint32_t op_s = (uint32_t)h.q_beg << 4 | (uint32_t)C_S, op_m = (uint32_t)(h.q_end - h.q_beg) << 4 | (uint32_t)C_M, op_t = tail << 4 | (uint32_t)C_S;
		const uint32_t op0 = !al ? 0u : head ? op_s : op_m, op1 = !al ? 0u : head ? op_m : tail ? op_t : 0u, op2 = head && tail ? op_t : 0u;
		if (lane == 0) {
			c.tid[row] = tid; c.pos[row] = pos; c.n_cigar[row] = (uint16_t)nc;
			c.cigar_ends[row] = (uint8_t)(al ? (head ? C_S : C_M) | (tail ? C_S : C_M) << 4 : 0xff);
			c.flag[row] = (uint16_t)flag; c.mapq[row] = (uint8_t)mapq; c.xc[row] = 0;
			c.l_qseq[row] = (int32_t)L; c.mtid[row] = -1; c.mpos[row] = -1; c.isize[row] = 0;
			c.cigar_off[row] = coff; c.seq_off[row] = soff; c.seq_bytes[row] = blk;
			row_name[row] = a.name_off[i];
		} else if (lane == 1) {
			uint4 *p = reinterpret_cast<uint4 *>(rec + row);
			p[0] = make_uint4((uint32_t)tid, (uint32_t)pos, flag | mapq << 16, nc);
			p[1] = make_uint4(L, 0xffffffffu, 0xffffffffu, 0u);
			p[2] = make_uint4(coff, op0, op1, op2);
			p[3] = make_uint4(0u, 0u, (uint32_t)soff, (uint32_t)(soff >> 32));
		} else if ((uint32_t)lane - 2u < nc) c.cigar[coff + (uint32_t)lane - 2u] = lane == 2 ? op0 : lane == 3 ? op1 : op2;
		// the block, a dword a lane
		uint32_t *o = reinterpret_cast<uint32_t *>(c.seqqual + soff);
		for (uint32_t d = (uint32_t)lane; d < blk / 4u; d += WAVE) {
			const uint32_t k = 4u * d;
			uint32_t w;
			if (k + 4u <= nb && 8u * d + 8u <= L) { // eight bases that are all there
				uint64_t x;
				__builtin_memcpy(&x, s + (rev ? L - 8u * d - 8u : 8u * d), 8);
				if (rev) x = __builtin_bswap64(x);
				w = 0u;
#pragma unroll
				for (int b = 0; b < 4; ++b)
					w |= (rr_code((uint32_t)(x >> (16 * b)) & 0xffu, rev) << 4 | rr_code((uint32_t)(x >> (16 * b + 8)) & 0xffu, rev)) << (8 * b);
			} else if (k >= nb && k - nb + 4u <= L) { // four qualities that are all there
				if (q) {
					const uint32_t j = k - nb;
					uint32_t x;
					__builtin_memcpy(&x, q + (rev ? L - j - 4u : j), 4);
					if (rev) x = __builtin_bswap32(x);
					w = ((x | 0x80808080u) - 0x21212121u) ^ (~x & 0x80808080u); // byte - 33 in every byte, no borrow between them
				} else w = 0xffffffffu;
			} else { // the seam between bases and qualities, the last bases of an L that is no multiple of 8, the end of the block
				w = 0u;
#pragma unroll
				for (uint32_t b = 0; b < 4u; ++b) w |= rr_byte(s, q, L, nb, rev, k + b) << (8u * b);
			}
			o[d] = w;
		}
	}
}

} // namespace ssv
