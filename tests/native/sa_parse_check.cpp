// sa_parse_check.cpp - the CPU build of `run -A -S`'s byte work (seeksv_amd/csrc/splitread_sa_parse.h: the two walkers, the entry parser, the geometry and
// the contig look-up) over hand-made optional-field areas.  Stand-alone: built with -fsanitize=address,undefined and run as it is (make asan; tests/
// test_splitread_sa_cli.py).  Every area is copied to the very end of an exactly sized heap buffer, so that a read at or beyond `end` is a heap overflow
// the sanitizer reports; every prefix of the long areas is walked too (each truncation of each field).  Exit status 0: every case gave what is written here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../seeksv_amd/csrc/splitread_sa_parse.h"

using namespace ssv;

static int failures = 0;

// the contig table as ssv_rt_begin_original_sa builds it, here with the hash cut to `bits` so that names share a hash
struct Table {
	std::vector<uint64_t> hash, off;
	std::vector<uint32_t> tid;
	std::vector<uint8_t> names;
	SaContigs view{};
	Table(const std::vector<std::string> &contigs, int bits)
	{
		const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
		std::vector<std::pair<uint64_t, uint32_t>> keyed;
		off.push_back(0);
		for (size_t t = 0; t < contigs.size(); ++t) {
			names.insert(names.end(), contigs[t].begin(), contigs[t].end());
			off.push_back(names.size());
			keyed.emplace_back(sa_name_hash(reinterpret_cast<const uint8_t *>(contigs[t].data()), (uint32_t)contigs[t].size()) & mask, (uint32_t)t);
		}
		std::sort(keyed.begin(), keyed.end());
		for (auto &k : keyed) { hash.push_back(k.first); tid.push_back(k.second); }
		names.push_back(0);
		view = SaContigs{hash.data(), tid.data(), off.data(), names.data(), (int64_t)contigs.size(), mask};
	}
};

// the area at the very end of a heap buffer of exactly its size
struct Exact {
	uint8_t *p; size_t n;
	explicit Exact(const std::string &s) : p(static_cast<uint8_t *>(malloc(s.size()))), n(s.size()) { if (n) memcpy(p, s.data(), n); }
	~Exact() { free(p); }
	const uint8_t *end() const { return p + n; }
};

struct Want { int status; int tid; int pos0; char strand; int mapq; unsigned n_keep; long long R; char side; int left, right, pos; };

static void check(const char *what, int enc, const std::string &area, const Table &T, const Want &w)
{
	Exact x(area);
	SaEntry e;
	const int st = sa_entry_of(x.p, x.end(), enc, &e);
	bool ok = st == w.status;
	if (ok && st == SA_OK && w.tid != -2) {
		SaGeometry g{};
		const bool geo = sa_geometry(e, &g);
		ok = sa_contig_find(T.view, e.rname, e.rname_len) == w.tid && e.pos0 == w.pos0 && e.strand == (uint8_t)w.strand && e.mapq == w.mapq && e.n_keep == w.n_keep && e.R == w.R;
		if (w.side) ok = ok && geo && g.side == (uint8_t)w.side && g.left == w.left && g.right == w.right && g.pos == w.pos;
		else ok = ok && !geo;
		// the operations as the gather decodes them: n_ops of them, ending exactly at the CIGAR text's end
		const uint8_t *q = e.cigar;
		uint32_t n = 0;
		while (q < e.cigar + e.cigar_len) { (void)sa_cigar_next(&q); ++n; }
		ok = ok && n == e.n_ops && q == e.cigar + e.cigar_len;
	}
	if (!ok) { ++failures; fprintf(stderr, "FAIL %s: status %d, wanted %d\n", what, st, w.status); }
}

static const Want NONE{-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, REFUSED{SA_REFUSED, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, MULTI{SA_MULTI, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
// chrB,5000,+,60S40M,60,0; : 5' clipped, left 60, right 40, pos 5000
static Want ok_at(int tid) { return Want{SA_OK, tid, 4999, '+', 60, 1, 100, '5', 60, 40, 5000}; }

static std::string z(const std::string &v) { return std::string("SAZ") + v + std::string(1, '\0'); }
static std::string b_array(char sub, uint32_t count, size_t bytes)
{
	std::string s = std::string("XBB") + sub;
	for (int k = 0; k < 4; ++k) s.push_back((char)(count >> (8 * k) & 255));
	return s + std::string(bytes, '\1');
}

int main()
{
	const std::vector<std::string> contigs{"chrB", "chrA", "chrA_alt", "chr;C:*"};
	const Table T(contigs, 64), T1(contigs, 1); // (one bit of hash: the four names in two runs)
	const std::string V = "chrB,5000,+,60S40M,60,0;", SA = z(V), NUL(1, '\0');

	// ---- the value's grammar (through the SAM walker: the value is the whole area behind SA:Z:) ----
	struct G { const char *name, *value; Want want; };
	const G grammar[] = {
		{"plain", "chrB,5000,+,60S40M,60,0;", ok_at(0)},
		{"no final ;", "chrB,5000,+,60S40M,60,0", ok_at(0)},
		{"two entries", "chrB,5000,+,60S40M,60,0;chrA,100,+,60S40M,60,0;", MULTI},
		{"a byte behind ;", "chrB,5000,+,60S40M,60,0;;", MULTI},
		{"empty", "", REFUSED},
		{"only a name", "chrB", REFUSED},
		{"name and comma", "chrB,", REFUSED},
		{"missing field", "chrB,5000,+,60S40M,60;", REFUSED},
		{"empty NM", "chrB,5000,+,60S40M,60,;", REFUSED},
		{"ends in mapQ", "chrB,5000,+,60S40M,60", REFUSED},
		{"ends in CIGAR", "chrB,5000,+,60S40M", REFUSED},
		{"ends in a length", "chrB,5000,+,60S40", REFUSED},
		{"ends at strand", "chrB,5000,+", REFUSED},
		{"ends in pos", "chrB,5000", REFUSED},
		{"pos 0", "chrB,0,+,60S40M,60,0;", REFUSED},
		{"pos 2^31", "chrB,2147483648,+,60S40M,60,0;", REFUSED},
		{"pos 2^31-1", "chrB,2147483647,+,60S40M,60,0;", Want{SA_OK, 0, 2147483646, '+', 60, 1, 100, '5', 60, 40, 2147483647}},
		{"pos of 30 digits", "chrB,500000000000000000000000000000,+,60S40M,60,0;", REFUSED},
		{"signed pos", "chrB,+5000,+,60S40M,60,0;", REFUSED},
		{"strand *", "chrB,5000,*,60S40M,60,0;", REFUSED},
		{"bad letter", "chrB,5000,+,60S40Q,60,0;", REFUSED},
		{"no length", "chrB,5000,+,60SM,60,0;", REFUSED},
		{"CIGAR *", "chrB,5000,+,*,60,0;", REFUSED},
		{"empty CIGAR", "chrB,5000,+,,60,0;", REFUSED},
		{"length 2^28", "chrB,5000,+,268435456S40M,60,0;", REFUSED},
		{"length 2^28-1", "chrB,5000,+,268435455S40M,60,0;", Want{SA_OK, 0, 4999, '+', 60, 1, 268435495, '5', 268435455, 40, 5000}},
		{"both ends clipped", "chrB,5000,+,30S40M30S,60,0;", Want{SA_OK, 0, 4999, '+', 60, 1, 100, 0, 0, 0, 0}},
		{"no end clipped", "chrB,5000,+,100M,60,0;", Want{SA_OK, 0, 4999, '+', 60, 1, 100, 0, 0, 0, 0}},
		{"one clip alone", "chrB,5000,+,100S,60,0;", Want{SA_OK, 0, 4999, '+', 60, 0, 100, 0, 0, 0, 0}},
		{"mapQ 256", "chrB,5000,+,60S40M,256,0;", REFUSED},
		{"mapQ 255", "chrB,5000,-,60S40M,255,0;", Want{SA_OK, 0, 4999, '-', 255, 1, 100, '5', 60, 40, 5000}},
		{"unknown contig", "chrZ,5000,+,60S40M,60,0;", Want{SA_OK, -1, 4999, '+', 60, 1, 100, '5', 60, 40, 5000}},
		{"empty contig", ",5000,+,60S40M,60,0;", Want{SA_OK, -1, 4999, '+', 60, 1, 100, '5', 60, 40, 5000}},
		{"prefix, short", "chrA,5000,+,60S40M,60,0;", ok_at(1)},
		{"prefix, long", "chrA_alt,5000,+,60S40M,60,0;", ok_at(2)},
		{"prefix, cut", "chrA_al,5000,+,60S40M,60,0;", Want{SA_OK, -1, 4999, '+', 60, 1, 100, '5', 60, 40, 5000}},
		{"; in the name", "chr;C:*,5000,+,60S40M,60,0;", ok_at(3)},
		{"3' clipped, D N = X I P", "chrB,1000,+,10M5D10=2X3I100N5P35M30S10H,7,3;", Want{SA_OK, 0, 999, '+', 7, 8, 100, '3', 60, 40, 999 + 10 + 5 + 10 + 100 + 35}},
		{"H and S run in front", "chrB,5000,+,50H10S40M,60,12;", ok_at(0)},
	};
	for (const G &g : grammar) {
		check(g.name, SA_ENC_SAM, std::string("SA:Z:") + g.value, T, g.want);
		check(g.name, SA_ENC_SAM, std::string("SA:Z:") + g.value, T1, g.want);                      // names that share a hash resolve alike
		check(g.name, SA_ENC_BAM, z(g.value), T, g.want);                                           // ... and the same value as a BAM field
	}
	// 65535 operations are taken, 65536 are not
	{
		std::string ops = "1S";
		for (int k = 0; k < 65534; ++k) ops += "1M";
		check("65535 operations", SA_ENC_SAM, "SA:Z:chrB,1,+," + ops + ",60,0;", T, Want{SA_OK, 0, 0, '+', 60, 65534, 65535, '5', 1, 65534, 1});
		check("65536 operations", SA_ENC_SAM, "SA:Z:chrB,1,+," + ops + "1M,60,0;", T, REFUSED);
	}

	// ---- the BAM walk ----
	struct B { const char *name; std::string area; Want want; };
	const std::string f32(4, '\2'), f64(8, '\3');
	const B bam[] = {
		{"first", SA + "NMC\1", ok_at(0)},
		{"last", std::string("NMC\1") + "ASS" + std::string(2, '\7') + SA, ok_at(0)},
		{"behind A", "XAAq" + SA, ok_at(0)}, {"behind c", "Xcc\1" + SA, ok_at(0)}, {"behind C", "XCC\1" + SA, ok_at(0)},
		{"behind s", "Xss\1\1" + SA, ok_at(0)}, {"behind S", "XSS\1\1" + SA, ok_at(0)}, {"behind i", "Xii" + f32 + SA, ok_at(0)},
		{"behind I", "XII" + f32 + SA, ok_at(0)}, {"behind f", "Xff" + f32 + SA, ok_at(0)}, {"behind d", "Xdd" + f64 + SA, ok_at(0)},
		{"behind Z", "XZZtext" + NUL + SA, ok_at(0)}, {"behind empty Z", "XZZ" + NUL + SA, ok_at(0)}, {"behind H", "XHH1AE3" + NUL + SA, ok_at(0)},
		{"behind B c", b_array('c', 3, 3) + SA, ok_at(0)}, {"behind B C", b_array('C', 3, 3) + SA, ok_at(0)}, {"behind B s", b_array('s', 3, 6) + SA, ok_at(0)},
		{"behind B S", b_array('S', 3, 6) + SA, ok_at(0)}, {"behind B i", b_array('i', 3, 12) + SA, ok_at(0)}, {"behind B I", b_array('I', 3, 12) + SA, ok_at(0)},
		{"behind B f", b_array('f', 2, 8) + SA, ok_at(0)}, {"behind an empty B", b_array('c', 0, 0) + SA, ok_at(0)},
		{"SA of type A first", "SAAx" + SA, ok_at(0)}, {"SA of type i first", "SAi" + f32 + SA, ok_at(0)}, {"SA of type H first", "SAH1AE3" + NUL + SA, ok_at(0)},
		{"the bytes SAZ inside a Z", "XZZSAZchrA,1,+,60S40M,60,0;" + NUL + "NMC\1", NONE},
		{"... and a real SA behind", "XZZSAZchrA,1,+,60S40M,60,0;" + NUL + SA, ok_at(0)},
		{"unknown type in front", "XQQ\1" + SA, NONE},
		{"no SA", "NMC\1", NONE}, {"empty area", "", NONE}, {"one byte", "S", NONE}, {"two bytes", "SA", NONE}, {"tag and type alone", "SAZ", NONE},
		{"truncated fixed value", "Xii\1\1", NONE},
		{"truncated Z", "NMC\1SAZ" + V, NONE},
		{"truncated Z in front", "XZZtext", NONE},
		{"truncated H", "XHH1AE3", NONE},
		{"B header cut", "XBBi\1\1", NONE},
		{"over-long B", b_array('i', 0x3fffffffu, 8) + SA, NONE},
		{"B count 2^32-1", b_array('i', 0xffffffffu, 8) + SA, NONE},
		{"B one element short", b_array('s', 3, 5), NONE},
		{"empty SA value", z(""), REFUSED},
	};
	for (const B &b : bam) check(b.name, SA_ENC_BAM, b.area, T, b.want);

	// ---- the SAM walk ----
	const std::string t = "\t", TV = "SA:Z:" + V;
	const B sam[] = {
		{"field 12", TV + t + "NM:i:1", ok_at(0)},
		{"last field", "NM:i:1" + t + "AS:i:77" + t + TV, ok_at(0)},
		{"ends at a newline", "NM:i:1" + t + TV + "\n", ok_at(0)},
		{"ends at \\r\\n", "NM:i:1" + t + TV + "\r\n", ok_at(0)},
		{"the next line is not read", "NM:i:1\nq\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*\t" + TV, NONE},
		{"\\r without a newline stays in the value", TV + "\r", MULTI},
		{"inside XA", "XA:Z:chrA,+1,60S40M,0;SA:Z:chrA,1,+,60S40M,60,0;" + t + "NM:i:0", NONE},
		{"inside XA, a real SA behind", "XA:Z:" + TV + t + TV, ok_at(0)},
		{"SA:i", "SA:i:5" + t + "NM:i:0", NONE},
		{"SA:i, then SA:Z", "SA:i:5" + t + TV, ok_at(0)},
		{"lower case", "sa:Z:" + V, NONE},
		{"SA:Z without its colon", "SA:Z" + t + "NM:i:0", NONE},
		{"empty value", "SA:Z:", REFUSED}, {"empty value, \\r\\n", "SA:Z:\r\n", REFUSED}, {"empty value, tab", "SA:Z:" + t + "NM:i:0", REFUSED},
		{"empty area", "", NONE}, {"empty fields", t + t + t, NONE}, {"four bytes", "SA:Z", NONE},
	};
	for (const B &s : sam) check(s.name, SA_ENC_SAM, s.area, T, s.want);

	// ---- every truncation of a long area of each encoding: whatever it gives, it reads nothing at or beyond its end ----
	const std::string long_bam = std::string("XAAq") + "Xss\1\1" + "Xii" + f32 + "Xdd" + f64 + "XZZtext" + NUL + "XHH1AE3" + NUL + b_array('s', 3, 6) + b_array('i', 2, 8) + SA + "NMC\1";
	const std::string long_sam = "NM:i:1" + t + "XA:Z:" + TV + t + "SA:i:5" + t + TV + t + "AS:i:77\r\n";
	for (size_t n = 0; n <= long_bam.size(); ++n) check("a prefix of the long BAM area", SA_ENC_BAM, long_bam.substr(0, n), T, Want{n >= long_bam.size() - 4 ? SA_OK : -1, -2, 0, 0, 0, 0, 0, 0, 0, 0, 0});
	for (size_t n = 0; n <= long_sam.size(); ++n) {
		Exact x(long_sam.substr(0, n));
		SaEntry e;
		(void)sa_entry_of(x.p, x.end(), SA_ENC_SAM, &e);
	}
	for (size_t n = 0; n <= V.size(); ++n) { // ... and of the value itself, in both encodings
		Exact x("SA:Z:" + V.substr(0, n)), y(z(V.substr(0, n)));
		SaEntry e;
		const int a = sa_entry_of(x.p, x.end(), SA_ENC_SAM, &e), b = sa_entry_of(y.p, y.end(), SA_ENC_BAM, &e);
		const int want = n >= V.size() - 1 ? SA_OK : SA_REFUSED; // (the whole entry, or all of it but the final ';')
		if (a != want || b != want) { ++failures; fprintf(stderr, "FAIL value cut to %zu bytes: %d %d, wanted %d\n", n, a, b, want); }
	}
	if (failures) { fprintf(stderr, "%d case(s) failed\n", failures); return 1; }
	printf("sa_parse_check: every case passed\n");
	return 0;
}
