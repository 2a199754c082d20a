// readthrough_stage.h - host end of `getsv -F` (FindJunction, process_bwasw.cpp:5-227): the pairs the GPU pass found (ssv_rt_finish) become
// junctions of the map, in the order of the records that completed them.  Small, string-heavy and order-dependent: stays on the host, like the
// junction stage.
#pragma once

#include <string>
#include <vector>

#include "junction_stage.h"
#include "seeksv_hip.h"

namespace seeksv {

bool minus_cigar_right(CigarVec &cigar_vec, int length); // MinusCigarRight, clip_reads.cpp:507-543
void add_cigar_left(CigarVec &cigar_vec, int length);    // AddCigarLeft, clip_reads.cpp:546-558

// The two SeqInfo values of one pair (process_bwasw.cpp:94-197: seq, CIGAR with its edit, clipped lengths, support 0 / 1, uniq 2 / 2).
void readthrough_seq_infos(const ssv_rt_result &r, const ssv_rt_pair &p, SeqInfo &up, SeqInfo &down);
// Every pair in order (:198-216): find(junction) - no entry: insert OtherInfo(up, down, microhomology, 0); an entry whose up or down seq length
// differs from the pair's: its down support + 1.  target_names[tid] = the -F file's contig names.
void apply_readthrough(const ssv_rt_result &r, const std::vector<std::string> &target_names, JunctionMap &junction2other);

} // namespace seeksv
