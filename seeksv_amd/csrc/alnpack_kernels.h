// alnpack_kernels.h - a decoded batch of clipped-sequence re-alignments as the columns the host join reads (junction_stage.cpp, RecSource): the fixed
// fields out of the record lines, the read names packed back to back, and the 64-bit hash of every name (text_hash, junction_stage.cpp:42-50), the join's
// first compare.  k_aln_name_len (per record) -> exclusive_scan -> k_aln_pack (four lanes per record).  The names come as DevNames (common.h).
// Names start at any byte of the decoder's text (or name) buffer and land at any byte of the blob: both kernels read whole ALIGNED 8-byte words only and
// funnel-shift; a word is read only when at least one of its bytes belongs to the name or is its NUL, so no load leaves the 8-byte granule - let alone the
// page - of a byte the name owns: no slack behind the buffers is relied on (ssv_samdec_decode leaves 128 bytes behind its text, ssv_bamdec_decode's names
// and ssv_aln_pack's own upload of host names at least 16; none of them is needed).
#pragma once

#include "common.h"
#include "clip_kernels.h"

namespace ssv {

constexpr uint32_t ALN_NAME_MAX = 254; // bytes of a read name without its NUL (BAM's l_read_name is one byte; the SAM decoder refuses longer ones)

// flag, mapq and cigar_off out of the record lines (tid, pos and n_cigar are hot columns of the batch already)
__global__ __launch_bounds__(BLOCK) void k_aln_cols(const ssv_record *__restrict__ rec, int64_t n, uint16_t *__restrict__ flag, uint8_t *__restrict__ mapq, uint32_t *__restrict__ cigar_off)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n) return;
	const uint4 a = reinterpret_cast<const uint4 *>(rec + i)[0];
	const uint32_t coff = reinterpret_cast<const uint32_t *>(rec + i)[8];
	flag[i] = (uint16_t)(a.z & 0xffffu); mapq[i] = (uint8_t)((a.z >> 16) & 0xffu); cigar_off[i] = coff;
}

// per record: bytes of its name with the NUL.  One lane walks the aligned words from the one the name starts in to the one its NUL is in (a name without a
// NUL within ALN_NAME_MAX + 1 bytes is cut there: the decoders hand out none).
__global__ __launch_bounds__(BLOCK) void k_aln_name_len(DevNames nm, int64_t n, uint32_t *__restrict__ nbytes)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n) return;
	const uint64_t s = (uint64_t)(uintptr_t)name_addr(nm, i);
	uint64_t a = s & ~7ull;
	const uint32_t lead = (uint32_t)(s & 7u);
	uint64_t w = *global_at<uint64_t>(a);
	if (lead) w |= (1ull << (8 * lead)) - 1ull; // the bytes in front of the name are someone else's: never a NUL
	uint32_t len = ALN_NAME_MAX;
	for (uint32_t at = 0u - lead;; ) { // `at`: offset of the word's first byte in the name (negative for the first word, modulo 2^32)
		const uint64_t z = (w - 0x0101010101010101ull) & ~w & 0x8080808080808080ull; // lowest set bit: the first zero byte
		if (z) { len = at + ((uint32_t)__builtin_ctzll(z) >> 3); break; }
		at += 8;
		if ((int32_t)at > (int32_t)ALN_NAME_MAX) break;
		a += 8;
		w = *global_at<uint64_t>(a);
	}
	nbytes[i] = (len < ALN_NAME_MAX ? len : ALN_NAME_MAX) + 1u;
}

// The 8 bytes at address p of a name that occupies [lo, end) with its NUL at `end`; bytes outside [lo, end) read as 0.  Aligned loads only, and only of
// words that overlap [lo, end].
__device__ __forceinline__ uint64_t aln_span_word(uint64_t p, uint64_t lo, uint64_t end)
{
	const uint64_t a = p & ~7ull;
	const uint32_t sh = (uint32_t)(p & 7u) * 8u;
	uint64_t w0 = 0, w1 = 0;
	if (a + 8 > lo && a <= end) w0 = *global_at<uint64_t>(a);
	if (sh && a + 16 > lo && a + 8 <= end) w1 = *global_at<uint64_t>(a + 8);
	const uint64_t v = sh ? (w0 >> sh) | (w1 << (64u - sh)) : w0;
	const uint64_t lead = p < lo ? lo - p : 0, keep = p < end ? end - p : 0; // the word's bytes [lead, keep) are the name's
	const uint64_t m_lo = lead >= 8 ? ~0ull : (1ull << (8 * lead)) - 1ull, m_hi = keep >= 8 ? ~0ull : (1ull << (8 * keep)) - 1ull;
	return v & m_hi & ~m_lo;
}

// Four lanes per record, sixteen records per wavefront (consecutive records: their names are neighbours in the blob, so a wavefront writes one stretch
// of it).  Round r: lane q of the quad builds the name's r * 4 + q-th word twice - as the blob's aligned word sees it (stored: whole words inside the
// name, single bytes where a word is shared with the neighbouring names) and as the hash sees it (from the name's first byte, the tail zero padded); the
// quad's four hash words are then exchanged (DPP) and every lane runs the same serial chain over them.
__global__ __launch_bounds__(BLOCK) void k_aln_pack(DevNames nm, int64_t n, const uint32_t *__restrict__ nbytes, const uint64_t *__restrict__ name_off, char *__restrict__ blob,
                                                   uint64_t *__restrict__ hash)
{
	const int64_t i = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 2;
	const uint32_t q = threadIdx.x & 3u;
	if (i >= n) return; // (a quad leaves together)
	const uint64_t s = (uint64_t)(uintptr_t)name_addr(nm, i);
	const uint32_t len = nbytes[i] - 1u;
	const uint64_t end = s + len, o = name_off[i];
	const uint32_t od = (uint32_t)(o & 7u);
	const uint64_t sd = s - od; // the source byte that lands on the blob's aligned word in front of (or at) the name
	char *const dst = blob + (o - od);
	const uint32_t n_dw = (od + len + 1u + 7u) >> 3, n_hw = (len + 7u) >> 3;
	const uint32_t rounds = ((n_dw > n_hw ? n_dw : n_hw) + 3u) >> 2;
	uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)len;
	for (uint32_t r = 0; r < rounds; ++r) {
		const uint32_t k = r * 4u + q;
		const uint64_t p = sd + 8ull * k;
		const uint64_t dv = aln_span_word(p, s, end);
		if (k < n_dw) {
			// the word's bytes [b0, b1) are this name's, the NUL included
			const uint32_t b0 = k == 0 ? od : 0u;
			const uint64_t left = end + 1 - p;
			const uint32_t b1 = left >= 8 ? 8u : (uint32_t)left;
			if (b0 == 0 && b1 == 8) *reinterpret_cast<uint64_t *>(dst + 8ull * k) = dv;
			else for (uint32_t b = b0; b < b1; ++b) dst[8ull * k + b] = (char)(dv >> (8 * b));
		}
		const uint64_t hv = aln_span_word(s + 8ull * k, s, end);
		const uint32_t lo = (uint32_t)hv, hi = (uint32_t)(hv >> 32);
		const uint64_t w[4] = {(uint64_t)quad_bcast<0>(lo) | ((uint64_t)quad_bcast<0>(hi) << 32), (uint64_t)quad_bcast<1>(lo) | ((uint64_t)quad_bcast<1>(hi) << 32),
		                       (uint64_t)quad_bcast<2>(lo) | ((uint64_t)quad_bcast<2>(hi) << 32), (uint64_t)quad_bcast<3>(lo) | ((uint64_t)quad_bcast<3>(hi) << 32)};
#pragma unroll
		for (uint32_t t = 0; t < 4; ++t)
			if (r * 4u + t < n_hw) { h = (h ^ w[t]) * 0xFF51AFD7ED558CCDull; h ^= h >> 29; }
	}
	if (q == 0) hash[i] = h * 0xC4CEB9FE1A85EC53ull;
}

} // namespace ssv
