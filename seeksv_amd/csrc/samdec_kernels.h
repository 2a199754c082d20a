// samdec_kernels.h - SAM text -> device batch (getsv -F reads `bwa bwasw` output, which is SAM text; process_bwasw.cpp:12-16 opens every name without
// ".bam" as text).  The text lies in HBM as the file has it; what libbam's sam_read1 does per line on one core happens here for a whole chunk:
//   k_sam_count / k_sam_marks  stream the text 16 bytes a lane: '\n' and '\t' by SWAR -> the ordered list of separator offsets, and every newline's place in it
//                              (the line table).  NUL bytes inside finished lines are refused here.
//   k_sam_sizes                per line: at least 11 fields, the name's length, the number of CIGAR operations, the SEQ length -> scanned into offsets
//   k_sam_fields               per line: integers, RNAME / RNEXT through a hash table of the header's names, CIGAR operations, XC:i:, the 64-byte line,
//                              the hot columns; a NUL over the line's first tab makes the name a C string where it lies
//   k_sam_seqqual              a wavefront per line: bases through a 256-entry LDS table into nibbles, QUAL - 33 in whole dwords
// A coordinate-sorted original (ssv_samdec_sorted: what getclip reads) takes the *_sorted forms of the two per-line kernels and, in k_sam_seqqual's place,
//   k_sam_seqqual_list         the same packing over the ordered list of the lines that ship bases and qualities (first or last CIGAR operation S)
//   k_sam_raw                  every UNMAP|MUNMAP line as a BAM record without optional fields (the unmapped-pair side channel)
// In that mode a QUAL byte below 33 is refused only where qualities are read: in lines that ship and in side-channel lines (libbam refuses none).
// A line that is not well-formed puts (line << 8 | reason) into one device word by atomic-min: the decode call fails with the smallest line.
#pragma once

#include "batch_columns.h"
#include "common.h"
#include "seeksv_hip.h"

namespace ssv {

constexpr int SAM_BYTES_PER_LANE = 16;
constexpr int SAM_TILE = BLOCK * SAM_BYTES_PER_LANE; // 4096 bytes of text per workgroup

enum SamErr : uint32_t {
	SAM_OK = 0, SAM_E_FIELDS, SAM_E_EMPTY, SAM_E_AT, SAM_E_NAME, SAM_E_NUMBER, SAM_E_CIGAR_CHAR, SAM_E_CIGAR_LEN, SAM_E_CIGAR_MANY, SAM_E_CIGAR_SEQ,
	SAM_E_SEQ_QUAL, SAM_E_QUAL, SAM_E_NUL, SAM_E_COUNT
};
constexpr unsigned long long SAM_NO_ERROR = ~0ull;

// the header's contig names: open addressing over FNV-1a, slot = tid + 1 (0: empty), the names' bytes to compare a hit against
struct SamRefTable {
	const uint32_t *slots;
	uint32_t mask;
	const uint32_t *off; // [n_targets + 1] into blob
	const uint8_t *blob;
};

// what only this decoder writes, beside the columns both decoders share (DecodedCols, batch_columns.h)
struct SamLineCols {
	uint64_t *name_off; // where the record's name starts in the text (ssv_samdec_names)
	ssv_record *rec;
};

// what the mode for coordinate-sorted originals adds (ssv_samdec_sorted)
struct SamSortedCols {
	uint32_t *ship;           // 1: the line ships bases + qualities (scanned into ship_idx)
	uint32_t *raw_bytes;      // size of the line's BAM record in the side channel, 0 for a line that is not UNMAP|MUNMAP (scanned into raw_off)
	const uint32_t *ship_idx; // the line's place in `list`
	uint32_t *list;           // the lines that ship, in file order
	int keep_all_seq;
};

// 0x80 in every byte of v that equals c
__device__ __forceinline__ uint32_t sam_eq_bytes(uint32_t v, uint32_t c)
{
	const uint32_t x = v ^ (c * 0x01010101u);
	return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
// ... as four bits
__device__ __forceinline__ uint32_t sam_bits4(uint32_t m)
{
	const uint32_t b = m >> 7;
	return (b | (b >> 7) | (b >> 14) | (b >> 21)) & 0xfu;
}

// the lane's 16 bytes of text [base, base + 16) as masks of newlines, tabs and NULs (bit k = byte base + k); bytes at and behind `len` count as nothing.
// virt_at >= 0: the byte there is the newline the host put behind a last line (ssv_samdec_decode, last): it counts unless a newline stands right in front of it
__device__ __forceinline__ void sam_lane_masks(const uint8_t *__restrict__ text, int64_t base, int64_t len, int64_t virt_at, uint32_t &nl, uint32_t &tab, uint32_t &nul)
{
	nl = tab = nul = 0;
	if (base >= len) return;
	const uint4 v = stream_load_u4(text + base);
	const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		nl |= sam_bits4(sam_eq_bytes(w[k], '\n')) << (4 * k);
		tab |= sam_bits4(sam_eq_bytes(w[k], '\t')) << (4 * k);
		nul |= sam_bits4(sam_eq_bytes(w[k], 0)) << (4 * k);
	}
	const uint32_t valid = len - base >= 16 ? 0xffffu : ((1u << (int)(len - base)) - 1u);
	nl &= valid; tab &= valid; nul &= valid;
	if (virt_at >= base && virt_at < base + 16) {
		const uint32_t bit = 1u << (int)(virt_at - base);
		tab &= ~bit; nul &= ~bit;
		if (virt_at == 0 || text[virt_at - 1] == '\n') nl &= ~bit;
	}
}

// per tile: separators (tabs + newlines) and newlines
__global__ __launch_bounds__(BLOCK) void k_sam_count(const uint8_t *__restrict__ text, int64_t len, int64_t virt_at, uint32_t *__restrict__ tile_sep, uint32_t *__restrict__ tile_nl)
{
	__shared__ uint32_t lds[2][WAVES_PER_BLOCK];
	const int64_t base = (int64_t)blockIdx.x * SAM_TILE + (int64_t)threadIdx.x * SAM_BYTES_PER_LANE;
	uint32_t nl, tab, nul;
	sam_lane_masks(text, base, len, virt_at, nl, tab, nul);
	const uint32_t a = wave_sum((uint32_t)__popc(nl | tab)), b = wave_sum((uint32_t)__popc(nl));
	if (lane_id() == 0) { lds[0][wave_id()] = a; lds[1][wave_id()] = b; }
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t s = 0, n = 0;
		for (int w = 0; w < WAVES_PER_BLOCK; ++w) { s += lds[0][w]; n += lds[1][w]; }
		tile_sep[blockIdx.x] = s; tile_nl[blockIdx.x] = n;
	}
}

// block-wide: the smallest error of the workgroup goes to *err with one atomic (none when there is no error)
__device__ __forceinline__ void sam_report(unsigned long long mine, unsigned long long *__restrict__ err)
{
	__shared__ unsigned long long smin;
	if (threadIdx.x == 0) smin = SAM_NO_ERROR;
	__syncthreads();
	if (mine != SAM_NO_ERROR) atomicMin(&smin, mine);
	__syncthreads();
	if (threadIdx.x == 0 && smin != SAM_NO_ERROR) atomicMin(err, smin);
}

// the separator list in text order, and per newline its index in that list.  sep_base / nl_base: the exclusive scans of k_sam_count's tile sums
__global__ __launch_bounds__(BLOCK) void k_sam_marks(const uint8_t *__restrict__ text, int64_t len, int64_t virt_at, const uint32_t *__restrict__ sep_base, const uint32_t *__restrict__ nl_base,
                                                    uint32_t n_lines, uint32_t *__restrict__ sep, uint32_t *__restrict__ nlidx, unsigned long long *__restrict__ err)
{
	__shared__ uint32_t lds[WAVES_PER_BLOCK + 1];
	const int64_t base = (int64_t)blockIdx.x * SAM_TILE + (int64_t)threadIdx.x * SAM_BYTES_PER_LANE;
	uint32_t nl, tab, nul;
	sam_lane_masks(text, base, len, virt_at, nl, tab, nul);
	// both counts in one block scan: separators in the low half, newlines in the high half (a tile holds at most 4096 of either)
	uint32_t tot;
	const uint32_t ex = block_exclusive_sum((uint32_t)__popc(nl | tab) | ((uint32_t)__popc(nl) << 16), lds, &tot);
	uint32_t s = sep_base[blockIdx.x] + (ex & 0xffffu), l = nl_base[blockIdx.x] + (ex >> 16);
	unsigned long long mine = SAM_NO_ERROR;
	if (nul) { // a NUL inside a finished line (the unfinished last one is looked at again with the next chunk)
		const uint32_t first = (uint32_t)__ffs((int)nul) - 1u;
		const uint32_t line = l + (uint32_t)__popc(nl & ((1u << first) - 1u));
		if (line < n_lines) mine = ((unsigned long long)line << 8) | SAM_E_NUL;
	}
	uint32_t m = nl | tab;
	while (m) {
		const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
		m &= m - 1u;
		sep[s] = (uint32_t)(base + k);
		if (nl >> k & 1u) nlidx[l++] = s;
		++s;
	}
	sam_report(mine, err);
}

// where line i lies: its bytes [start, end) without the newline and a '\r' in front of it, its separators sep[first .. first + ntabs) (tabs) and the newline behind them
struct SamLine {
	uint32_t start, end, first, ntabs;
	__device__ __forceinline__ uint32_t fs(const uint32_t *__restrict__ sep, uint32_t k) const { return k ? sep[first + k - 1] + 1u : start; }
	__device__ __forceinline__ uint32_t fe(const uint32_t *__restrict__ sep, uint32_t k) const { return k < ntabs ? sep[first + k] : end; }
};
__device__ __forceinline__ SamLine sam_line(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, int64_t i)
{
	SamLine L;
	const uint32_t last = nlidx[i];
	if (i) { const uint32_t p = nlidx[i - 1]; L.first = p + 1u; L.start = sep[p] + 1u; } else { L.first = 0; L.start = 0; }
	L.end = sep[last];
	L.ntabs = last - L.first;
	if (L.end > L.start && text[L.end - 1] == '\r') --L.end;
	return L;
}

// the checks of a line's shape; SAM_OK: the line has a name of 1..254 bytes and at least 11 fields
__device__ __forceinline__ uint32_t sam_shape(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const SamLine &L)
{
	if (L.end == L.start) return SAM_E_EMPTY;
	if (text[L.start] == '@') return SAM_E_AT;
	if (L.ntabs < 10) return SAM_E_FIELDS;
	const uint32_t nl = L.fe(sep, 0) - L.start;
	if (nl == 0 || nl > 254) return SAM_E_NAME;
	return SAM_OK;
}

// decimal in [0, limit]; false: not a number or out of range
__device__ __forceinline__ bool sam_uint(const uint8_t *__restrict__ text, uint32_t s, uint32_t e, uint64_t limit, uint64_t &out)
{
	if (e == s || e - s > 19u) return false;
	uint64_t v = 0;
	for (uint32_t p = s; p < e; ++p) {
		const uint32_t d = (uint32_t)text[p] - '0';
		if (d > 9u) return false;
		v = v * 10u + d;
		if (v > limit) return false;
	}
	out = v;
	return true;
}

// FLAG: decimal or 0x hex; false: refused (v: as far as it was read)
__device__ __forceinline__ bool sam_flag(const uint8_t *__restrict__ text, uint32_t s, uint32_t en, uint64_t &v)
{
	if (en - s > 2u && text[s] == '0' && (text[s + 1] == 'x' || text[s + 1] == 'X')) {
		bool ok = en - s <= 10u;
		for (uint32_t p = s + 2; p < en && ok; ++p) {
			const uint32_t ch = text[p], lc = ch | 0x20u;
			const uint32_t d = ch - '0' <= 9u ? ch - '0' : lc - 'a' <= 5u ? lc - 'a' + 10u : 16u;
			ok = d < 16u;
			v = v * 16u + d;
		}
		return ok && v <= 65535u;
	}
	return sam_uint(text, s, en, 65535u, v) && !(en - s > 1u && text[s] == '0'); // (a leading 0 is octal to libbam's strtol: refused)
}

// SORTED: bases + qualities ship by the BAM decoder's rule (record_fields_of, bamdec_kernels.h: first or last CIGAR operation S, or keep_all_seq), read off the
// CIGAR text's first and last operation letters; a line whose flag - with the 4 a '*' CIGAR sets - has UNMAP or MUNMAP gets the size of its BAM record
template <bool SORTED>
__device__ __forceinline__ void sam_sizes_body(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, int64_t n, const DecodedCols &c, const SamSortedCols &x,
                                               unsigned long long *__restrict__ err)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	unsigned long long mine = SAM_NO_ERROR;
	if (i < n) {
		const SamLine L = sam_line(text, sep, nlidx, i);
		uint32_t e = sam_shape(text, sep, L), nc = 0, lq = 0;
		bool soft = false, star = false;
		if (e == SAM_OK) {
			const uint32_t cs = L.fs(sep, 5), ce = L.fe(sep, 5);
			star = ce - cs == 1 && text[cs] == '*';
			if (!star)
				for (uint32_t p = cs; p < ce; ++p) {
					const uint32_t ch = text[p];
					const bool op = (ch - '0') > 9u;
					if (SORTED && op && (nc == 0 || p + 1 == ce)) soft = soft || ch == 'S';
					nc += op;
				}
			if (nc > 65535u) { e = SAM_E_CIGAR_MANY; nc = 0; }
			else {
				const uint32_t ss = L.fs(sep, 9), se = L.fe(sep, 9);
				lq = (se - ss == 1 && text[ss] == '*') ? 0u : se - ss;
			}
		}
		if (e != SAM_OK) mine = ((unsigned long long)i << 8) | e;
		c.n_cigar[i] = (uint16_t)nc;
		c.l_qseq[i] = (int32_t)lq;
		const uint32_t sb = (lq + 1u) / 2u + lq;
		if (!SORTED) c.seq_bytes[i] = sb;
		else {
			const uint32_t ships = (soft || x.keep_all_seq) ? sb : 0u;
			uint32_t rb = 0;
			uint64_t v = 0;
			if (e == SAM_OK && sam_flag(text, L.fs(sep, 1), L.fe(sep, 1), v) && (((uint32_t)v | (star ? (uint32_t)F_UNMAP : 0u)) & (uint32_t)(F_UNMAP | F_MUNMAP)))
				rb = 36u + (L.fe(sep, 0) - L.start) + 1u + 4u * nc + sb; // block_size, core, name and NUL, operations, bases, qualities
			c.seq_bytes[i] = ships; x.ship[i] = ships != 0u; x.raw_bytes[i] = rb;
		}
	}
	sam_report(mine, err);
}

__global__ __launch_bounds__(BLOCK) void k_sam_sizes(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, int64_t n, DecodedCols c,
                                                    unsigned long long *__restrict__ err)
{
	sam_sizes_body<false>(text, sep, nlidx, n, c, SamSortedCols{}, err);
}

__global__ __launch_bounds__(BLOCK) void k_sam_sizes_sorted(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, int64_t n, DecodedCols c,
                                                           SamSortedCols x, unsigned long long *__restrict__ err)
{
	sam_sizes_body<true>(text, sep, nlidx, n, c, x, err);
}

__device__ __forceinline__ int sam_lookup(const uint8_t *__restrict__ text, uint32_t s, uint32_t e, const SamRefTable &T)
{
	uint32_t h = 2166136261u;
	for (uint32_t p = s; p < e; ++p) h = (h ^ text[p]) * 16777619u;
	for (uint32_t probe = 0; probe <= T.mask; ++probe) {
		const uint32_t slot = T.slots[(h + probe) & T.mask];
		if (!slot) return -1;
		const uint32_t t = slot - 1u, o = T.off[t];
		if (T.off[t + 1] - o != e - s) continue;
		bool same = true;
		for (uint32_t k = 0; k < e - s && same; ++k) same = T.blob[o + k] == text[s + k];
		if (same) return (int)t;
	}
	return -1;
}

__device__ __forceinline__ int sam_cigar_code(uint32_t ch)
{
	switch (ch) {
	case 'M': return C_M; case 'I': return C_I; case 'D': return C_D; case 'N': return C_N; case 'S': return C_S;
	case 'H': return C_H; case 'P': return C_P; case '=': return C_EQ; case 'X': return C_X;
	default: return -1;
	}
}

// SORTED: xc, seq_off and the record line's offset as ssv_bamdec_decode(keep_all_seq = 0) gives them (xc only for a soft-clipped record, SSV_NO_SEQ for a
// record that ships nothing), and the line's number on the list of the lines that ship
template <bool SORTED>
__device__ __forceinline__ void sam_fields_body(uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, int64_t n, const SamRefTable &T, const DecodedCols &c,
                                                const SamLineCols &x, const SamSortedCols &srt, int32_t *__restrict__ max_span, unsigned long long *__restrict__ err)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	unsigned long long mine = SAM_NO_ERROR;
	int span_out = 0;
	if (i < n) {
		const SamLine L = sam_line(text, sep, nlidx, i);
		uint32_t e = SAM_OK;
		int32_t tid = -1, pos = -1, mtid = -1, mpos = -1, isize = 0;
		uint32_t flag = 0, mapq = 0, xc = 0, ends = 0xffu, h[5] = {0, 0, 0, 0, 0};
		const uint32_t nc = c.n_cigar[i], coff = c.cigar_off[i];
		const uint32_t lq = (uint32_t)c.l_qseq[i];
		uint64_t soff = c.seq_off[i];
		if (sam_shape(text, sep, L) == SAM_OK) { // (k_sam_sizes reported the others)
			uint64_t v = 0;
			if (!sam_flag(text, L.fs(sep, 1), L.fe(sep, 1), v)) e = SAM_E_NUMBER;
			flag = (uint32_t)v;
			{ // RNAME
				const uint32_t s = L.fs(sep, 2), en = L.fe(sep, 2);
				tid = (en - s == 1 && text[s] == '*') ? -1 : sam_lookup(text, s, en, T);
			}
			if (!e) { if (sam_uint(text, L.fs(sep, 3), L.fe(sep, 3), 0x7fffffffu, v)) pos = (int32_t)v - 1; else e = SAM_E_NUMBER; }
			if (!e) { if (sam_uint(text, L.fs(sep, 4), L.fe(sep, 4), 255u, v)) mapq = (uint32_t)v; else e = SAM_E_NUMBER; }
			uint64_t qlen = 0, span = 0;
			if (!e) { // CIGAR: nc operations were counted (every byte that is no digit); their slots are cigar[coff .. coff + nc)
				const uint32_t s = L.fs(sep, 5), en = L.fe(sep, 5);
				if (en - s == 1 && text[s] == '*') flag |= F_UNMAP; // (libbam: "mapped sequence without CIGAR" - it sets the flag and goes on)
				else {
					if (en == s) e = SAM_E_CIGAR_CHAR;
					uint64_t len = 0;
					uint32_t digits = 0, k = 0, lastc = 0;
					for (uint32_t p = s; p < en && !e; ++p) {
						const uint32_t ch = text[p], d = ch - '0';
						if (d <= 9u) { len = len * 10u + d; if (++digits > 9u) e = SAM_E_NUMBER; continue; }
						const int code = sam_cigar_code(ch);
						if (code < 0) { e = SAM_E_CIGAR_CHAR; break; }
						if (!digits) { e = SAM_E_CIGAR_LEN; break; }
						if (len >= (1u << 28)) { e = SAM_E_NUMBER; break; }
						const uint32_t op = (uint32_t)len << 4 | (uint32_t)code;
						if (k < nc) { c.cigar[coff + k] = op; if (k < 5) h[k] = op; }
						if (k == 0) ends = (uint32_t)code;
						lastc = (uint32_t)code;
						if (code == C_M || code == C_I || code == C_S || code == C_EQ || code == C_X) qlen += len;
						if (code == C_M || code == C_D || code == C_N || code == C_EQ || code == C_X) span += len;
						++k; len = 0; digits = 0;
					}
					if (!e && digits) e = SAM_E_CIGAR_CHAR; // a length without its operation
					if (!e) ends |= lastc << 4;
				}
			}
			if (!e) { // RNEXT
				const uint32_t s = L.fs(sep, 6), en = L.fe(sep, 6);
				if (en - s == 1 && text[s] == '=') mtid = tid;
				else mtid = (en - s == 1 && text[s] == '*') ? -1 : sam_lookup(text, s, en, T);
			}
			if (!e) { if (sam_uint(text, L.fs(sep, 7), L.fe(sep, 7), 0x7fffffffu, v)) mpos = (int32_t)v - 1; else e = SAM_E_NUMBER; }
			if (!e) { // TLEN
				uint32_t s = L.fs(sep, 8);
				const uint32_t en = L.fe(sep, 8);
				const bool neg = s < en && text[s] == '-';
				if (neg) ++s;
				if (sam_uint(text, s, en, neg ? 0x80000000ull : 0x7fffffffull, v)) isize = neg ? (int32_t)(0u - (uint32_t)v) : (int32_t)v; else e = SAM_E_NUMBER;
			}
			if (!e) {
				const uint32_t ss = L.fs(sep, 9), se = L.fe(sep, 9), qs = L.fs(sep, 10), qe = L.fe(sep, 10);
				const bool seq_given = !(se - ss == 1 && text[ss] == '*'), qual_given = !(qe - qs == 1 && text[qs] == '*');
				if (seq_given && nc && qlen != (uint64_t)lq) e = SAM_E_CIGAR_SEQ;
				else if (qual_given && qe - qs != lq) e = SAM_E_SEQ_QUAL;
			}
			if (!e) { // optional fields: XC:i: alone matters (clip_reads.cpp:126-129 asks whether its value is non-zero)
				for (uint32_t k = 11; k <= L.ntabs; ++k) {
					const uint32_t s = L.fs(sep, k), en = L.fe(sep, k);
					if (en - s > 5u && text[s] == 'X' && text[s + 1] == 'C' && text[s + 2] == ':' && text[s + 3] == 'i' && text[s + 4] == ':')
						for (uint32_t p = s + 5; p < en; ++p) xc |= (uint32_t)((uint32_t)text[p] - '1' <= 8u);
				}
			}
			if (!e) {
				span_out = span > 0x7fffffffull ? 0x7fffffff : (int)span;
				text[L.fe(sep, 0)] = 0; // the name as a C string where it lies (ssv_samdec_names)
			} else mine = ((unsigned long long)i << 8) | e;
		}
		if (SORTED) {
			if (!(nc && ((ends & 15u) == (uint32_t)C_S || (ends >> 4) == (uint32_t)C_S))) xc = 0;
			if (c.seq_bytes[i]) srt.list[srt.ship_idx[i]] = (uint32_t)i;
			else { soff = ~0ull; c.seq_off[i] = soff; }
		}
		c.tid[i] = tid; c.pos[i] = pos; c.mtid[i] = mtid; c.mpos[i] = mpos; c.isize[i] = isize;
		c.flag[i] = (uint16_t)flag; c.mapq[i] = (uint8_t)mapq; c.xc[i] = (uint8_t)xc; c.cigar_ends[i] = (uint8_t)ends;
		x.name_off[i] = L.start;
		uint4 *p = reinterpret_cast<uint4 *>(x.rec + i);
		p[0] = make_uint4((uint32_t)tid, (uint32_t)pos, flag | (mapq << 16) | (xc << 24), nc);
		p[1] = make_uint4(lq, (uint32_t)mtid, (uint32_t)mpos, (uint32_t)isize);
		p[2] = make_uint4(coff, h[0], h[1], h[2]);
		p[3] = make_uint4(h[3], h[4], (uint32_t)soff, (uint32_t)(soff >> 32));
	}
	span_out = wave_max(span_out);
	if (lane_id() == 0 && span_out > 0 && span_out > __hip_atomic_load(max_span, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(max_span, span_out); // (look first: one address, a wavefront each)
	sam_report(mine, err);
}

__global__ __launch_bounds__(BLOCK) void k_sam_fields(uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, int64_t n, SamRefTable T, DecodedCols c, SamLineCols x,
                                                     int32_t *__restrict__ max_span, unsigned long long *__restrict__ err)
{
	sam_fields_body<false>(text, sep, nlidx, n, T, c, x, SamSortedCols{}, max_span, err);
}

__global__ __launch_bounds__(BLOCK) void k_sam_fields_sorted(uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, int64_t n, SamRefTable T, DecodedCols c,
                                                            SamLineCols x, SamSortedCols srt, int32_t *__restrict__ max_span, unsigned long long *__restrict__ err)
{
	sam_fields_body<true>(text, sep, nlidx, n, T, c, x, srt, max_span, err);
}

// libbam's bam_nt16_table into 256 bytes of LDS, a thread per entry (BLOCK threads; the caller's barrier follows): '=' 0, "ACMGRSVTWYHKDBN" 1..15 in either case,
// "0123" 1 2 4 8, everything else 15 (bytes of 128 and above too: libbam indexes its table with a signed char there and reads whatever lies in front of it)
__device__ __forceinline__ void sam_nt16_fill(uint8_t *nt16)
{
	const uint32_t ch = threadIdx.x, up = ch & ~0x20u;
	uint32_t v = 15;
	if (ch == '=') v = 0;
	else if (ch >= '0' && ch <= '3') v = 1u << (ch - '0');
	else if ((ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z')) {
		switch (up) {
		case 'A': v = 1; break; case 'C': v = 2; break; case 'M': v = 3; break; case 'G': v = 4; break; case 'R': v = 5; break; case 'S': v = 6; break; case 'V': v = 7; break;
		case 'T': v = 8; break; case 'W': v = 9; break; case 'Y': v = 10; break; case 'H': v = 11; break; case 'K': v = 12; break; case 'D': v = 13; break; case 'B': v = 14; break;
		default: v = 15; break;
		}
	}
	nt16[ch] = (uint8_t)v;
}

// SEQ and QUAL of line L (l bases) by one wavefront: consecutive lanes read consecutive bytes of the text and write consecutive bytes of
// o[0 .. ceil(l / 2) + l) = [packed bases | qualities]; QUAL '*' gives 0xff.  true in the lanes that met a QUAL byte below 33.
__device__ __forceinline__ bool sam_pack_line(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const SamLine &L, uint32_t l, uint8_t *__restrict__ o, const uint8_t *nt16, int lane)
{
	if (L.ntabs < 10) return false;
	const uint32_t ss = L.fs(sep, 9), qs = L.fs(sep, 10), qe = L.fe(sep, 10);
	const bool qual_given = !(qe - qs == 1 && text[qs] == '*');
	if (L.fe(sep, 9) - ss != l || (qual_given && qe - qs != l)) return false; // (k_sam_fields refused the line)
	const uint32_t nb = (l + 1u) / 2u;
	for (uint32_t j = (uint32_t)lane; j < nb; j += WAVE) {
		const uint32_t hi = nt16[text[ss + 2u * j]], lo = 2u * j + 1u < l ? nt16[text[ss + 2u * j + 1u]] : 0u;
		o[j] = (uint8_t)(hi << 4 | lo);
	}
	// qualities: bytes up to the first aligned dword of the output, whole dwords, the bytes behind the last one
	uint8_t *q = o + nb;
	const uint32_t head = min(l, (uint32_t)((0u - (uint32_t)(uintptr_t)q) & 3u)), nd = (l - head) / 4u, tail0 = head + nd * 4u;
	bool bad = false;
	if (!qual_given) {
		if ((uint32_t)lane < head) q[lane] = 0xff;
		for (uint32_t j = (uint32_t)lane; j < nd; j += WAVE) reinterpret_cast<uint32_t *>(q + head)[j] = 0xffffffffu;
		if ((uint32_t)lane < l - tail0) q[tail0 + lane] = 0xff;
	} else {
		const uint8_t *src = text + qs;
		if ((uint32_t)lane < head) { const uint32_t b = src[lane]; bad |= b < 33u; q[lane] = (uint8_t)(b - 33u); }
		for (uint32_t j = (uint32_t)lane; j < nd; j += WAVE) {
			const uint8_t *s4 = src + head + 4u * j;
			const uint32_t w = (uint32_t)s4[0] | (uint32_t)s4[1] << 8 | (uint32_t)s4[2] << 16 | (uint32_t)s4[3] << 24;
			// a byte below 33: bit 7 of (byte | 0x80) - 33 is clear exactly then (bytes of 128 and above stay above)
			const uint32_t low = ~(((w & 0x7f7f7f7fu) | 0x80808080u) - 0x21212121u) & ~w & 0x80808080u;
			bad |= low != 0;
			// per-byte subtraction without borrows between the bytes: (w | 0x80..) - 0x21.. then the top bits put right
			const uint32_t d = ((w | 0x80808080u) - 0x21212121u) ^ ((~w) & 0x80808080u);
			reinterpret_cast<uint32_t *>(q + head)[j] = d;
		}
		if ((uint32_t)lane < l - tail0) { const uint32_t b = src[tail0 + lane]; bad |= b < 33u; q[tail0 + lane] = (uint8_t)(b - 33u); }
	}
	return bad;
}

// SEQ and QUAL, a wavefront per line (most of a SAM file's bytes).  out: [ceil(l / 2) packed bases | l qualities] at seq_off[i].  A QUAL byte below 33 is refused.
__global__ __launch_bounds__(BLOCK) void k_sam_seqqual(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, int64_t n, const int32_t *__restrict__ l_qseq,
                                                      const uint64_t *__restrict__ seq_off, uint8_t *__restrict__ out, unsigned long long *__restrict__ err)
{
	__shared__ uint8_t nt16[256];
	sam_nt16_fill(nt16);
	__syncthreads();
	const int lane = lane_id();
	const int64_t n_waves = (int64_t)gridDim.x * WAVES_PER_BLOCK;
	for (int64_t i = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave_id(); i < n; i += n_waves) {
		const uint32_t l = (uint32_t)l_qseq[i];
		if (l == 0) continue;
		const bool bad = sam_pack_line(text, sep, sam_line(text, sep, nlidx, i), l, out + seq_off[i], nt16, lane);
		if (__any(bad) && lane == 0) atomicMin(err, ((unsigned long long)i << 8) | SAM_E_QUAL);
	}
}

// ... over the list of the lines that ship (ssv_samdec_sorted: about one line in twenty of a coordinate-sorted original), a wavefront per listed line
__global__ __launch_bounds__(BLOCK) void k_sam_seqqual_list(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, const uint32_t *__restrict__ list,
                                                           uint32_t n_list, const int32_t *__restrict__ l_qseq, const uint64_t *__restrict__ seq_off, uint8_t *__restrict__ out,
                                                           unsigned long long *__restrict__ err)
{
	__shared__ uint8_t nt16[256];
	sam_nt16_fill(nt16);
	__syncthreads();
	const int lane = lane_id();
	const uint32_t n_waves = gridDim.x * WAVES_PER_BLOCK;
	for (uint32_t k = blockIdx.x * WAVES_PER_BLOCK + (uint32_t)wave_id(); k < n_list; k += n_waves) {
		const int64_t i = list[k];
		const uint32_t l = (uint32_t)l_qseq[i];
		if (l == 0) continue;
		const bool bad = sam_pack_line(text, sep, sam_line(text, sep, nlidx, i), l, out + seq_off[i], nt16, lane);
		if (__any(bad) && lane == 0) atomicMin(err, ((unsigned long long)i << 8) | SAM_E_QUAL);
	}
}

// The side channel: every line with raw_bytes (UNMAP|MUNMAP in its flag as decoded) as a BAM record at raw + raw_off - block_size, the 32 core bytes (bin 0), the
// name with its NUL, the CIGAR operations, packed bases, qualities; no optional fields.  A lane per line looks (such lines are few: a workgroup without one
// leaves at once); the wavefront then writes each record it found together.  Runs behind k_sam_fields: the core comes out of the decoded columns, name, SEQ and
// QUAL out of the text - whether or not the line ships.
__global__ __launch_bounds__(BLOCK) void k_sam_raw(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sep, const uint32_t *__restrict__ nlidx, int64_t n, DecodedCols c,
                                                  const uint32_t *__restrict__ raw_bytes, const uint64_t *__restrict__ raw_off, uint8_t *__restrict__ raw, unsigned long long *__restrict__ err)
{
	__shared__ uint8_t nt16[256];
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	const uint32_t nb = i < n ? raw_bytes[i] : 0u;
	if (!__syncthreads_or(nb != 0u)) return;
	sam_nt16_fill(nt16);
	__syncthreads();
	const int lane = lane_id();
	uint64_t m = __ballot(nb != 0u);
	while (m) {
		const int src = __ffsll((long long)m) - 1;
		m &= m - 1;
		const uint32_t knb = (uint32_t)__shfl((int)nb, src);
		const int64_t ki = i - lane + src;
		const SamLine L = sam_line(text, sep, nlidx, ki);
		const uint32_t nl = L.fe(sep, 0) - L.start, nc = c.n_cigar[ki], lq = (uint32_t)c.l_qseq[ki], coff = c.cigar_off[ki];
		if (knb != 36u + nl + 1u + 4u * nc + (lq + 1u) / 2u + lq) continue; // (the size k_sam_sizes_sorted gave the record: nothing is written outside it)
		uint8_t *o = raw + raw_off[ki];
		const uint32_t w[9] = {knb - 4u, (uint32_t)c.tid[ki], (uint32_t)c.pos[ki], (nl + 1u) | (uint32_t)c.mapq[ki] << 8, nc | (uint32_t)c.flag[ki] << 16, lq,
		                       (uint32_t)c.mtid[ki], (uint32_t)c.mpos[ki], (uint32_t)c.isize[ki]};
		if (lane < 36) {
			uint32_t v = 0;
#pragma unroll
			for (int k = 0; k < 9; ++k) v = (lane >> 2) == k ? w[k] : v;
			o[lane] = (uint8_t)(v >> (8 * (lane & 3)));
		}
		for (uint32_t j = (uint32_t)lane; j <= nl; j += WAVE) o[36u + j] = j < nl ? text[L.start + j] : (uint8_t)0;
		uint8_t *oc = o + 36u + nl + 1u;
		for (uint32_t j = (uint32_t)lane; j < 4u * nc; j += WAVE) oc[j] = (uint8_t)(c.cigar[coff + (j >> 2)] >> (8u * (j & 3u)));
		if (lq) {
			const bool bad = sam_pack_line(text, sep, L, lq, oc + 4u * nc, nt16, lane);
			if (__any(bad) && lane == 0) atomicMin(err, ((unsigned long long)ki << 8) | SAM_E_QUAL);
		}
	}
}

} // namespace ssv
