// table_wire.h - the narrow wire form of the compact cluster table's small columns, and the host code that turns it back into the columns
// ssv_clip_table_wait hands out.  No HIP in here: a host compiler takes this file alone (tests/native/table_wire_check.cpp).
//
// What crosses PCIe per cluster instead of pos i32 | left_len, right_len u16 | support u16 | n_cigar u8 and the CIGAR's operations:
//   one row of 6 bytes   dpos u16 | left_len u8 | right_len u8 | support u8 | n_cigar (6 bits) + CIGAR kind (2 bits)
//     dpos   pos minus the pos of the cluster before, or WIRE_ESC: the cluster's pos stands in the escape list.  The first cluster of a (contig, side) run, the
//            first cluster of every tile of 256 sorted slots and every cluster 65535 bases or more behind its predecessor escape.
//     kind   0: the cluster's n_cigar operations stand in the CIGAR stream;  1: they are exactly {left_len M, right_len S};  2: exactly {left_len S, right_len M}
//            (n_cigar is 2 then, and the stream holds nothing for the cluster)
//   escapes  cluster << 32 | pos, sorted by cluster before the rebuild
// A table with a value these fields cannot hold (a length of 256 or more, a support of 255 or more, more than 63 operations) crosses with the wide columns instead.
#pragma once

#include <stdint.h>
#include <string.h>
#include <vector>

namespace ssv {

struct WireRow {
	uint16_t dpos;
	uint8_t ll, lr, support, nck;
};
static_assert(sizeof(WireRow) == 6, "a wire row is 6 bytes");

constexpr uint32_t WIRE_ESC = 0xffffu;
constexpr int WIRE_NCIG_BITS = 6;
constexpr uint32_t WIRE_LEN_MAX = 255, WIRE_SUPPORT_MAX = 254, WIRE_NCIG_MAX = (1u << WIRE_NCIG_BITS) - 1;
constexpr uint32_t WIRE_OP_M = 0, WIRE_OP_S = 4; // BAM's codes: an operation is length << 4 | code

struct WireIn {
	const WireRow *rows; int64_t n;
	const uint64_t *esc; int64_t n_esc;   // sorted
	const void *cig; int cig_bytes;       // the kind-0 clusters' operations, 2 or 4 bytes each
	uint64_t wire_ops;
};

// the handed-out columns (ssv_cluster_table: pos, c_len, c_support, c_ncig, c_cigar) at their widths
struct WireOut {
	int32_t *pos;
	void *len; int len_bytes;             // 2 or 4
	void *support; int support_bytes;     // 2 or 4
	void *ncig; int ncig_bytes;           // 1 or 2
	void *cigar; uint64_t cigar_ops;      // cig_bytes each
};

// what pass 1 leaves of a range of clusters for the ranges behind it
struct WireRange {
	int64_t head_end = 0;      // clusters [k0, head_end) stand before the range's first escape: their pos waits for the carry
	uint32_t head_sum = 0;     // ... and the deltas among them add up to this
	bool has_esc = false;
	int32_t last_pos = 0;      // pos of the range's last cluster (relative to the carry while !has_esc)
	uint64_t ops = 0, wire_ops = 0;
	int bad = 0;
};

template <class T> static inline void wire_put(void *a, int64_t k, uint32_t v) { reinterpret_cast<T *>(a)[k] = (T)v; }

// pass 1 over clusters [k0, k1): the widened lengths, support and n_cigar, every pos behind the range's first escape, and the range's sums
inline void wire_pass1(const WireIn &in, const WireOut &out, int64_t k0, int64_t k1, WireRange &r)
{
	r = WireRange();
	r.head_end = k0;
	// first escape at or behind k0
	int64_t lo = 0, hi = in.n_esc;
	while (lo < hi) { const int64_t m = (lo + hi) / 2; if ((int64_t)(in.esc[m] >> 32) < k0) lo = m + 1; else hi = m; }
	int64_t e = lo;
	uint32_t pos = 0;
	for (int64_t k = k0; k < k1; ++k) {
		const WireRow w = in.rows[k];
		if (out.len_bytes == 2) { wire_put<uint16_t>(out.len, 2 * k, w.ll); wire_put<uint16_t>(out.len, 2 * k + 1, w.lr); }
		else { wire_put<uint32_t>(out.len, 2 * k, w.ll); wire_put<uint32_t>(out.len, 2 * k + 1, w.lr); }
		if (out.support_bytes == 2) wire_put<uint16_t>(out.support, k, w.support); else wire_put<uint32_t>(out.support, k, w.support);
		const uint32_t nc = w.nck & WIRE_NCIG_MAX, kind = w.nck >> WIRE_NCIG_BITS;
		if (out.ncig_bytes == 1) wire_put<uint8_t>(out.ncig, k, nc); else wire_put<uint16_t>(out.ncig, k, nc);
		if (kind > 2 || (kind && nc != 2)) r.bad = 1;
		r.ops += nc;
		if (!kind) r.wire_ops += nc;
		if (w.dpos == WIRE_ESC) {
			if (e >= in.n_esc || (int64_t)(in.esc[e] >> 32) != k) { r.bad = 1; continue; }
			pos = (uint32_t)in.esc[e++];
			r.has_esc = true;
			out.pos[k] = (int32_t)pos;
		} else {
			pos += w.dpos;
			if (r.has_esc) out.pos[k] = (int32_t)pos;
			else { r.head_end = k + 1; r.head_sum = pos; }
		}
	}
	r.last_pos = (int32_t)pos;
}

// pass 2: the heads' pos from the carry (the pos of cluster k0 - 1), and the CIGARs from where the ranges before left off
inline void wire_pass2(const WireIn &in, const WireOut &out, int64_t k0, int64_t k1, const WireRange &r, int32_t carry, uint64_t op0, uint64_t wop0, int &bad)
{
	uint32_t pos = (uint32_t)carry;
	for (int64_t k = k0; k < r.head_end; ++k) { pos += in.rows[k].dpos; out.pos[k] = (int32_t)pos; }
	uint64_t o = op0, wo = wop0;
	for (int64_t k = k0; k < k1; ++k) {
		const WireRow w = in.rows[k];
		const uint32_t nc = w.nck & WIRE_NCIG_MAX, kind = w.nck >> WIRE_NCIG_BITS;
		if (o + nc > out.cigar_ops || (!kind && wo + nc > in.wire_ops)) { bad = 1; return; }
		if (kind) {
			const uint32_t a = ((uint32_t)w.ll << 4) | (kind == 1 ? WIRE_OP_M : WIRE_OP_S), b = ((uint32_t)w.lr << 4) | (kind == 1 ? WIRE_OP_S : WIRE_OP_M);
			if (in.cig_bytes == 2) { wire_put<uint16_t>(out.cigar, (int64_t)o, a); wire_put<uint16_t>(out.cigar, (int64_t)o + 1, b); }
			else { wire_put<uint32_t>(out.cigar, (int64_t)o, a); wire_put<uint32_t>(out.cigar, (int64_t)o + 1, b); }
		} else if (nc) {
			memcpy(reinterpret_cast<uint8_t *>(out.cigar) + o * (uint64_t)in.cig_bytes, reinterpret_cast<const uint8_t *>(in.cig) + wo * (uint64_t)in.cig_bytes, (size_t)nc * (size_t)in.cig_bytes);
			wo += nc;
		}
		o += nc;
	}
}

// the whole rebuild over nt ranges of clusters; run(nt, fn) calls fn(0 .. nt - 1), side by side or one after the other.  0: done; 1: the wire form contradicts itself
template <class Run>
inline int wire_rebuild(const WireIn &in, const WireOut &out, int nt, Run &&run)
{
	const int64_t n = in.n;
	if (nt < 1) nt = 1;
	std::vector<WireRange> rg((size_t)nt);
	run(nt, [&](int w) { wire_pass1(in, out, n * w / nt, n * (w + 1) / nt, rg[(size_t)w]); });
	std::vector<int32_t> carry((size_t)nt, 0);
	std::vector<uint64_t> op0((size_t)nt + 1, 0), wop0((size_t)nt + 1, 0);
	int bad = 0;
	bool have = false; // a pos to carry on from
	int32_t last = 0;
	for (int w = 0; w < nt; ++w) {
		const WireRange &r = rg[(size_t)w];
		bad |= r.bad;
		if (r.head_end > n * w / nt && !have) bad = 1; // deltas in front of the table's first escape
		carry[(size_t)w] = last;
		if (n * (w + 1) / nt > n * w / nt) { last = r.has_esc ? r.last_pos : (int32_t)((uint32_t)last + (uint32_t)r.last_pos); have = have || r.has_esc; }
		op0[(size_t)w + 1] = op0[(size_t)w] + r.ops; wop0[(size_t)w + 1] = wop0[(size_t)w] + r.wire_ops;
	}
	if (bad || op0[(size_t)nt] != out.cigar_ops || wop0[(size_t)nt] != in.wire_ops) return 1;
	std::vector<int> bad2((size_t)nt, 0);
	run(nt, [&](int w) { wire_pass2(in, out, n * w / nt, n * (w + 1) / nt, rg[(size_t)w], carry[(size_t)w], op0[(size_t)w], wop0[(size_t)w], bad2[(size_t)w]); });
	for (int b : bad2) bad |= b;
	return bad;
}

} // namespace ssv
