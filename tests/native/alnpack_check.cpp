// alnpack_check.cpp - clip_text_hash (seeksv_amd/host/junction_stage.cpp) of every line of standard input, one decimal number per line: the host function that
// the GPU's name hash (ssv_aln_pack) and the tests' Python model of it (tests/clip_sam.py) must agree with.  For tests/test_alnpack_model.py.
#include <cstdio>
#include <iostream>
#include <string>

#include "../../seeksv_amd/host/junction_stage.h"

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) printf("%llu\n", (unsigned long long)seeksv::clip_text_hash(line.data(), line.size()));
	return 0;
}
