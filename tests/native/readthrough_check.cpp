// readthrough_check.cpp - the host end of `getsv -F` (seeksv_amd/host/readthrough_stage.cpp) without a GPU: the CIGAR edits and the
// insert-or-count rule on a hand-made ssv_rt_result.  Prints what it finds; tests/test_readthrough_stage.py holds the expectations.
#include <cstdio>
#include <string>
#include <vector>

#include "../../seeksv_amd/host/readthrough_stage.h"

using namespace seeksv;

static std::string text(const CigarVec &v)
{
	std::string s;
	for (auto &x : v) s += std::to_string(x.first) + x.second;
	return s;
}

int main()
{
	// MinusCigarRight / AddCigarLeft (clip_reads.cpp:507-558)
	const char *minus[][2] = {{"40M3I7M2D", "0"}, {"40M3I7M2D", "5"}, {"70M", "30"}, {"30M", "30"}, {"10M5D20M10X", "12"}, {"5=50M", "50"}};
	for (auto &m : minus) {
		CigarVec v = parse_cigar(m[0]);
		const bool ok = minus_cigar_right(v, atoi(m[1]));
		printf("minus %s %s -> %s %d\n", m[0], m[1], text(v).c_str(), (int)ok);
	}
	const char *add[][2] = {{"70M", "10"}, {"5I65M", "10"}, {"3=40M", "2"}};
	for (auto &a : add) {
		CigarVec v = parse_cigar(a[0]);
		add_cigar_left(v, atoi(a[1]));
		printf("add %s %s -> %s\n", a[0], a[1], text(v).c_str());
	}
	// three pairs on one key (the second with equal lengths, the third with other lengths), one pair on the key of a -B row, one on a key of its own
	const std::vector<std::string> names = {"chrA", "chrB"};
	std::string seqs;
	std::vector<uint32_t> cigars;
	std::vector<ssv_rt_pair> pairs;
	auto add_pair = [&](int ut, int up, char us, int dt, int dp, char ds, int mh, const std::string &a, const std::string &b, std::vector<uint32_t> ca,
	                    std::vector<uint32_t> cb, int ue, int de) {
		ssv_rt_pair p{};
		p.up_tid = ut; p.up_pos = up; p.up_strand = us; p.down_tid = dt; p.down_pos = dp; p.down_strand = ds; p.microhomology = mh;
		p.up_len = (int)a.size(); p.down_len = (int)b.size(); p.up_cig_n = (int)ca.size(); p.down_cig_n = (int)cb.size(); p.up_cig_edit = ue; p.down_cig_edit = de;
		p.seq_off = seqs.size(); p.cig_off = cigars.size();
		seqs += a + b;
		cigars.insert(cigars.end(), ca.begin(), ca.end()); cigars.insert(cigars.end(), cb.begin(), cb.end());
		pairs.push_back(p);
	};
	const uint32_t M70 = 70u << 4, M60 = 60u << 4, I5 = (5u << 4) | 1;
	add_pair(1, 6050, '+', 0, 20001, '+', 0, "AAAA", "CCCCCC", {M70}, {M60}, 0, 0);
	add_pair(1, 6050, '+', 0, 20001, '+', 0, "GGGG", "TTTTTT", {M70}, {M60}, 0, 0);
	add_pair(1, 6050, '+', 0, 20001, '+', 3, "GGG", "TTTTTT", {M70}, {M60}, 1, 0);
	add_pair(0, 1040, '+', 0, 5001, '+', 30, "ACGTACGT", "TTT", {M70}, {I5, M60}, 1, 2);
	add_pair(0, 100, '-', 1, 200, '+', 4, "ACG", "TGCA", {M70}, {I5, M60}, 0, 2);
	ssv_rt_result r{};
	r.n_pairs = (int64_t)pairs.size(); r.pairs = pairs.data(); r.seqs = seqs.data(); r.cigars = cigars.data();
	JunctionMap m;
	OtherInfo b; // a -B row on chrA 1040 + -> chrA 5001 +
	b.up.seq = "ACGT"; b.down.seq = "ACGT"; b.up.support = 3; b.down.support = 2;
	m.insert(std::make_pair(Junction{"chrA", 1040, '+', "chrA", 5001, '+'}, b));
	apply_readthrough(r, names, m);
	for (auto &kv : m) {
		const Junction &j = kv.first; const OtherInfo &o = kv.second;
		printf("%s %d %c %s %d %c | %d %d | %s %s %d %d %d %d | %s %s %d %d %d %d | %d\n", j.up_chr.c_str(), j.up_pos, j.up_strand, j.down_chr.c_str(), j.down_pos, j.down_strand,
		       o.microhomology, o.abnormal, o.up.seq.c_str(), text(o.up.cigar_vec).c_str(), o.up.left_clipped, o.up.right_clipped, o.up.support, o.up.uniq,
		       o.down.seq.c_str(), text(o.down.cigar_vec).c_str(), o.down.left_clipped, o.down.right_clipped, o.down.support, o.down.uniq, (int)m.count(j));
	}
	return 0;
}
