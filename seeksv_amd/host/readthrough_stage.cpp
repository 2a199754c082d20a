// readthrough_stage.cpp - see readthrough_stage.h
#include "readthrough_stage.h"

namespace seeksv {

bool minus_cigar_right(CigarVec &cigar_vec, int length)
{
	int len = 0;
	for (const auto &x : cigar_vec) if (x.second == 'M' || x.second == 'I') len += x.first;
	if (len <= length) return false;
	int l = len - length;
	for (auto it = cigar_vec.begin(); it != cigar_vec.end(); ++it) {
		if (it->second != 'M' && it->second != 'I') continue;
		if (it->first >= l) { // this operation ends the kept part: everything behind it goes
			it->first = l;
			cigar_vec.erase(it + 1, cigar_vec.end());
			break;
		}
		l -= it->first;
	}
	return true;
}

void add_cigar_left(CigarVec &cigar_vec, int length)
{
	if (!cigar_vec.empty() && cigar_vec[0].second == 'M') cigar_vec[0].first += length;
	else cigar_vec.insert(cigar_vec.begin(), std::make_pair(length, 'M')); // (an empty vector is undefined behaviour in the reference)
}

static CigarVec cigar_of(const uint32_t *ops, int n)
{
	CigarVec v;
	v.reserve((size_t)n);
	for (int k = 0; k < n; ++k) v.push_back(std::make_pair((int)(ops[k] >> 4), "MIDNSHP=X???????"[ops[k] & 15]));
	return v;
}

void readthrough_seq_infos(const ssv_rt_result &r, const ssv_rt_pair &p, SeqInfo &up, SeqInfo &down)
{
	up = SeqInfo(); down = SeqInfo();
	up.seq.assign(r.seqs + p.seq_off, (size_t)p.up_len);
	down.seq.assign(r.seqs + p.seq_off + (uint64_t)p.up_len, (size_t)p.down_len);
	up.cigar_vec = cigar_of(r.cigars + p.cig_off, p.up_cig_n);
	down.cigar_vec = cigar_of(r.cigars + p.cig_off + (uint64_t)p.up_cig_n, p.down_cig_n);
	if (p.up_cig_edit == 1) minus_cigar_right(up.cigar_vec, p.microhomology);
	if (p.down_cig_edit == 2) add_cigar_left(down.cigar_vec, p.microhomology);
	up.left_clipped = p.up_left_clipped; up.right_clipped = p.up_right_clipped; up.support = 0; up.uniq = 2;
	down.left_clipped = p.down_left_clipped; down.right_clipped = p.down_right_clipped; down.support = 1; down.uniq = 2;
}

void apply_readthrough(const ssv_rt_result &r, const std::vector<std::string> &target_names, JunctionMap &junction2other)
{
	for (int64_t k = 0; k < r.n_pairs; ++k) {
		const ssv_rt_pair &p = r.pairs[k];
		const Junction j{target_names[(size_t)p.up_tid], p.up_pos, (char)p.up_strand, target_names[(size_t)p.down_tid], p.down_pos, (char)p.down_strand};
		auto it = junction2other.find(j); // (the first entry of the key's range: it may be a -B row)
		if (it == junction2other.end()) {
			OtherInfo o;
			readthrough_seq_infos(r, p, o.up, o.down);
			o.microhomology = p.microhomology; o.abnormal = 0;
			junction2other.insert(std::make_pair(j, o));
		} else if ((int64_t)it->second.up.seq.size() != p.up_len || (int64_t)it->second.down.seq.size() != p.down_len) {
			it->second.down.support++;
		}
	}
}

} // namespace seeksv
