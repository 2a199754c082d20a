// table_wire_check.cpp - the host rebuild of the cluster table's narrow wire form (seeksv_amd/csrc/table_wire.h) against an encoder written here, on its own:
// seeded random tables and the boundary cases, each rebuilt over 1, 3 and 16 thread ranges, over ranges that start on an escape and ranges that start just
// behind one, at every width of the handed-out columns.  Prints "<n> tables, <bad> bad"; exit status 1 when any differed.
//   g++ -std=c++17 -fsanitize=address,undefined -Iseeksv_amd/csrc tests/native/table_wire_check.cpp -o table_wire_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <random>
#include <vector>

#include "table_wire.h"

using namespace ssv;

namespace {

// a table as a caller sees it
struct Table {
	std::vector<int32_t> tid, pos;
	std::vector<uint8_t> side;
	std::vector<uint32_t> ll, lr, support;
	std::vector<std::vector<uint32_t>> cigar; // BAM operations: length << 4 | code
	std::vector<int64_t> tile_first;          // clusters that open a tile of sorted slots (they escape whatever their step)
};

struct Wire {
	std::vector<WireRow> rows;
	std::vector<uint64_t> esc;
	std::vector<uint8_t> cig;
	uint64_t wire_ops = 0, ops = 0;
};

// the encoder: rows, escapes and the CIGAR stream of `t`, by the rules of table_wire.h's head comment
Wire encode(const Table &t, int cig_bytes)
{
	Wire w;
	const size_t n = t.pos.size();
	for (size_t k = 0; k < n; ++k) {
		bool esc = k == 0 || t.tid[k] != t.tid[k - 1] || t.side[k] != t.side[k - 1] || std::binary_search(t.tile_first.begin(), t.tile_first.end(), (int64_t)k);
		const int64_t step = k ? (int64_t)t.pos[k] - (int64_t)t.pos[k - 1] : 0;
		if (!esc && (step < 0 || step >= 0xffff)) esc = true;
		WireRow r;
		r.dpos = esc ? 0xffff : (uint16_t)step;
		if (esc) w.esc.push_back(((uint64_t)k << 32) | (uint32_t)t.pos[k]);
		r.ll = (uint8_t)t.ll[k]; r.lr = (uint8_t)t.lr[k]; r.support = (uint8_t)t.support[k];
		const std::vector<uint32_t> &cg = t.cigar[k];
		uint32_t kind = 0;
		if (cg.size() == 2 && cg[0] == (t.ll[k] << 4 | 0u) && cg[1] == (t.lr[k] << 4 | 4u)) kind = 1;
		if (cg.size() == 2 && cg[0] == (t.ll[k] << 4 | 4u) && cg[1] == (t.lr[k] << 4 | 0u)) kind = 2;
		r.nck = (uint8_t)(cg.size() | (kind << 6));
		w.rows.push_back(r);
		w.ops += cg.size();
		if (!kind) {
			for (uint32_t op : cg) {
				if (cig_bytes == 2) { const uint16_t v = (uint16_t)op; w.cig.insert(w.cig.end(), reinterpret_cast<const uint8_t *>(&v), reinterpret_cast<const uint8_t *>(&v) + 2); }
				else w.cig.insert(w.cig.end(), reinterpret_cast<const uint8_t *>(&op), reinterpret_cast<const uint8_t *>(&op) + 4);
			}
			w.wire_ops += cg.size();
		}
	}
	return w;
}

int n_tables = 0, n_bad = 0;

// rebuild `t`'s wire form over the given cluster ranges (cuts: ascending, first 0, last n) and hold every column against the table
void check_cuts(const Table &t, const Wire &w, int cig_bytes, int len_bytes, int support_bytes, int ncig_bytes, const std::vector<int64_t> &cuts, const char *what)
{
	const int64_t n = (int64_t)t.pos.size();
	std::vector<int32_t> pos((size_t)n + 1, -7);
	std::vector<uint8_t> len((size_t)n * 2 * len_bytes + 1, 0xa5), sup((size_t)n * support_bytes + 1, 0xa5), nc((size_t)n * ncig_bytes + 1, 0xa5), cig((size_t)w.ops * cig_bytes + 1, 0xa5);
	const WireIn in{w.rows.data(), n, w.esc.data(), (int64_t)w.esc.size(), w.cig.data(), cig_bytes, w.wire_ops};
	const WireOut out{pos.data(), len.data(), len_bytes, sup.data(), support_bytes, nc.data(), ncig_bytes, cig.data(), w.ops};
	// wire_rebuild's own arithmetic with ranges of our choosing: the two passes and the carries between them
	const int nt = (int)cuts.size() - 1;
	std::vector<WireRange> rg((size_t)nt);
	for (int v = 0; v < nt; ++v) wire_pass1(in, out, cuts[(size_t)v], cuts[(size_t)v + 1], rg[(size_t)v]);
	int bad = 0, last = 0;
	uint64_t o = 0, wo = 0;
	for (int v = 0; v < nt; ++v) {
		const WireRange &r = rg[(size_t)v];
		bad |= r.bad;
		int b2 = 0;
		wire_pass2(in, out, cuts[(size_t)v], cuts[(size_t)v + 1], r, last, o, wo, b2);
		bad |= b2;
		if (cuts[(size_t)v + 1] > cuts[(size_t)v]) last = r.has_esc ? r.last_pos : (int32_t)((uint32_t)last + (uint32_t)r.last_pos);
		o += r.ops; wo += r.wire_ops;
	}
	auto get = [](const std::vector<uint8_t> &a, int64_t k, int width) { uint32_t v = 0; memcpy(&v, a.data() + k * width, (size_t)width); return v; };
	uint64_t co = 0;
	for (int64_t k = 0; k < n && !bad; ++k) {
		if (pos[(size_t)k] != t.pos[(size_t)k] || get(len, 2 * k, len_bytes) != t.ll[(size_t)k] || get(len, 2 * k + 1, len_bytes) != t.lr[(size_t)k] || get(sup, k, support_bytes) != t.support[(size_t)k] ||
		    get(nc, k, ncig_bytes) != t.cigar[(size_t)k].size()) bad = 1;
		for (uint32_t op : t.cigar[(size_t)k]) if (get(cig, (int64_t)co++, cig_bytes) != op) bad = 1;
	}
	if (o != w.ops || wo != w.wire_ops || pos[(size_t)n] != -7 || len.back() != 0xa5 || sup.back() != 0xa5 || nc.back() != 0xa5 || cig.back() != 0xa5) bad = 1;
	++n_tables;
	if (bad) { ++n_bad; printf("BAD: %s (%lld clusters, %d ranges, widths %d/%d/%d/%d)\n", what, (long long)n, nt, len_bytes, support_bytes, ncig_bytes, cig_bytes); }
}

void check(const Table &t, const char *what)
{
	const int64_t n = (int64_t)t.pos.size();
	for (int cig_bytes : {2, 4}) {
		const Wire w = encode(t, cig_bytes);
		for (int widths = 0; widths < 2; ++widths) {
			const int lb = widths ? 4 : 2, sb = widths ? 4 : 2, nb = widths ? 2 : 1;
			// wire_rebuild itself, 1 / 3 / 16 even ranges
			for (int nt : {1, 3, 16}) {
				std::vector<int32_t> pos((size_t)n);
				std::vector<uint8_t> len((size_t)n * 2 * lb), sup((size_t)n * sb), nc((size_t)n * nb), cig((size_t)w.ops * cig_bytes);
				const WireIn in{w.rows.data(), n, w.esc.data(), (int64_t)w.esc.size(), w.cig.data(), cig_bytes, w.wire_ops};
				const WireOut out{pos.data(), len.data(), lb, sup.data(), sb, nc.data(), nb, cig.data(), w.ops};
				const int rc = wire_rebuild(in, out, nt, [](int k, const std::function<void(int)> &f) { for (int v = k - 1; v >= 0; --v) f(v); }); // (ranges in any order)
				++n_tables;
				if (rc || !std::equal(pos.begin(), pos.end(), t.pos.begin())) { ++n_bad; printf("BAD: %s, wire_rebuild over %d ranges\n", what, nt); }
				std::vector<int64_t> cuts;
				for (int v = 0; v <= nt; ++v) cuts.push_back(n * v / nt);
				check_cuts(t, w, cig_bytes, lb, sb, nb, cuts, what);
			}
			// ranges that start on an escape, and ranges that start on the cluster behind one
			std::vector<int64_t> on{0}, behind{0};
			for (uint64_t e : w.esc) { const int64_t k = (int64_t)(e >> 32); if (k > on.back()) on.push_back(k); if (k + 1 < n && k + 1 > behind.back()) behind.push_back(k + 1); }
			on.push_back(n); behind.push_back(n);
			check_cuts(t, w, cig_bytes, lb, sb, nb, on, what);
			check_cuts(t, w, cig_bytes, lb, sb, nb, behind, what);
		}
	}
}

uint32_t op(uint32_t len, uint32_t code) { return len << 4 | code; }

Table random_table(uint32_t seed, int n, int tile)
{
	std::mt19937 g(seed);
	auto rnd = [&](uint32_t m) { return (uint32_t)(g() % m); };
	Table t;
	int32_t tid = 0, pos = 1 + (int32_t)rnd(1000);
	uint8_t side = '5';
	for (int k = 0; k < n; ++k) {
		if (k && rnd(200) == 0) { if (side == '5') side = '3'; else { side = '5'; tid += 1 + (int32_t)rnd(3); } pos = 1 + (int32_t)rnd(100000); }
		else if (k) pos += rnd(50) == 0 ? 65000 + (int32_t)rnd(1200) : rnd(10) == 0 ? 0 : (int32_t)rnd(2200);
		if (tile && k % tile == (int)rnd(3)) t.tile_first.push_back(k);
		t.tid.push_back(tid); t.pos.push_back(pos); t.side.push_back(side);
		const uint32_t ll = rnd(20) == 0 ? 255 - rnd(2) : 1 + rnd(150), lr = rnd(20) == 0 ? 255 : 1 + rnd(150);
		t.ll.push_back(ll); t.lr.push_back(lr); t.support.push_back(rnd(30) == 0 ? 254 - rnd(2) : 1 + rnd(3));
		std::vector<uint32_t> cg;
		switch (rnd(8)) {
		case 0: cg = {op(ll, 4), op(lr, 0)}; break;
		case 1: cg = {op(ll, 0), op(lr, 4)}; break;
		case 2: cg = {op(ll, 4), op(lr + 1, 0)}; break;                       // the record's lengths are not the consensus lengths
		case 3: cg = {op(ll, 4), op(lr, 0), op(7, 4)}; break;
		case 4: cg = {op(ll, 0), op(lr, 5)}; break;                           // H is not S
		case 5: for (uint32_t i = 0, m = rnd(64); i < m; ++i) cg.push_back(op(1 + rnd(4000), rnd(9))); break; // up to 63 operations, none at all too
		case 6: cg = {op(ll, 7), op(lr, 4)}; break;                           // = is not M
		default: cg = {op(ll, 4), op(3, 1), op(lr, 0), op(2, 2), op(5, 8)}; break;
		}
		t.cigar.push_back(cg);
	}
	std::sort(t.tile_first.begin(), t.tile_first.end());
	t.tile_first.erase(std::unique(t.tile_first.begin(), t.tile_first.end()), t.tile_first.end());
	return t;
}

} // namespace

int main()
{
	for (uint32_t seed = 1; seed <= 24; ++seed) check(random_table(seed, seed % 5 == 0 ? 1 + (int)seed : 300 + 97 * (int)seed, seed % 3 ? 200 : 0), "random");
	{ // steps of 65534 / 65535 / 65536 in one run, a step of 0, a run of one cluster, the largest pos
		Table t;
		const int32_t p[] = {10, 10 + 65534, 10 + 65534 + 65535, 10 + 65534 + 65535 + 65536, 10 + 65534 + 65535 + 65536, 0x7fffffff, 5, 5, 70000};
		const int32_t td[] = {0, 0, 0, 0, 0, 0, 1, 2, 2};
		for (int k = 0; k < 9; ++k) { t.tid.push_back(td[k]); t.pos.push_back(p[k]); t.side.push_back('5'); t.ll.push_back(255); t.lr.push_back(k); t.support.push_back(254); t.cigar.push_back({op(255, 0), op((uint32_t)k, 4)}); }
		check(t, "steps at the escape");
	}
	{ // an empty table, and one cluster
		Table t;
		check(t, "empty");
		t.tid = {3}; t.pos = {77}; t.side = {'3'}; t.ll = {1}; t.lr = {2}; t.support = {1}; t.cigar = {{}};
		check(t, "one cluster");
	}
	{ // a wire form that contradicts itself is refused, not followed: an escape that the list does not hold, a CIGAR stream too short
		const Table t = random_table(99, 500, 128);
		Wire w = encode(t, 2);
		std::vector<int32_t> pos(500);
		std::vector<uint8_t> len(2000), sup(1000), nc(500), cig(w.ops * 2);
		auto serial = [](int k, const std::function<void(int)> &f) { for (int v = 0; v < k; ++v) f(v); };
		WireIn in{w.rows.data(), 500, w.esc.data(), (int64_t)w.esc.size() - 1, w.cig.data(), 2, w.wire_ops};
		const WireOut out{pos.data(), len.data(), 2, sup.data(), 2, nc.data(), 1, cig.data(), w.ops};
		++n_tables;
		if (!wire_rebuild(in, out, 3, serial)) { ++n_bad; printf("BAD: a missing escape went through\n"); }
		in.n_esc = (int64_t)w.esc.size(); in.wire_ops = w.wire_ops - 1;
		++n_tables;
		if (!wire_rebuild(in, out, 3, serial)) { ++n_bad; printf("BAD: a short CIGAR stream went through\n"); }
	}
	printf("%d tables, %d bad\n", n_tables, n_bad);
	return n_bad ? 1 : 0;
}
