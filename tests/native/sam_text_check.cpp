// sam_text_check.cpp - SamTextReader (seeksv_amd/host/sam_text.cpp) on its own, for tests/test_sam_text_stdin.py:
//   sam_text_check <file | -> <chunk bytes>   the header's contigs, the first record's line number, gzip or not, then the records' text as the chunks carry it
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../../seeksv_amd/host/sam_text.h"

int main(int argc, char **argv)
{
	if (argc < 3) { std::cerr << "usage: sam_text_check <file | -> <chunk bytes>" << std::endl; return 2; }
	seeksv::SamTextReader rd;
	std::string err;
	if (!rd.open(argv[1], err)) { std::cerr << err << std::endl; return 1; }
	printf("targets %zu first_line %llu gzip %d\n", rd.target_names().size(), (unsigned long long)rd.first_record_line(), rd.is_gzip() ? 1 : 0);
	for (size_t t = 0; t < rd.target_names().size(); ++t) printf("%s %d\n", rd.target_names()[t].c_str(), rd.target_lens()[t]);
	rd.start((size_t)atoll(argv[2]));
	seeksv::SamTextReader::Chunk ck;
	size_t chunks = 0;
	bool last = false;
	while (rd.next(ck, err)) { fwrite(ck.data, 1, ck.bytes, stdout); ++chunks; last = ck.last; }
	if (!err.empty()) { std::cerr << err << std::endl; return 1; }
	fflush(stdout);
	fprintf(stderr, "chunks %zu last %d\n", chunks, last ? 1 : 0);
	return 0;
}
