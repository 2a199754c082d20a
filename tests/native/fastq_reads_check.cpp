// CPU check of seeksv_amd/host/fastq_reads.h (the FASTQ cutting of `seeksv run -P`): records whose text lies in an allocation of exactly its size, so
// that a read past either end is an error under AddressSanitizer.  Built and run by `make asan`.  Exit code 0 = every case gave what it should.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>

#include "fastq_reads.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// the text in memory of exactly its size (no terminator behind it)
static int cut_all(const std::string &text, seeksv::FastqReads &out, std::string &err)
{
	std::unique_ptr<char[]> exact(new char[text.size() ? text.size() : 1]);
	memcpy(exact.get(), text.data(), text.size());
	size_t at = 0;
	int rc, n = 0;
	while ((rc = seeksv::fastq_next(exact.get(), text.size(), at, out, err)) > 0) ++n;
	return rc < 0 ? rc : n;
}

int main()
{
	seeksv::FastqReads r;
	std::string err;
	// two records, a comment behind the name, "*" for the qualities, a last line without its newline
	EXPECT(cut_all("@jn3/2 1:N:0\nACGTN\n+\nIIII#\n@q\tx\nAC\n+\n*", r, err) == 2);
	EXPECT(r.n() == 2 && r.seqs == "ACGTNAC" && r.quals == "IIII#!!" && r.names == std::string("jn3/2\0q\0", 8));
	EXPECT(r.seq_off.size() == 3 && r.seq_off[1] == 5 && r.seq_off[2] == 7 && r.name_off[1] == 6 && r.name_off[2] == 8);
	// carriage returns are dropped; an empty read is a read; records are appended behind the ones that are there
	EXPECT(cut_all("@e\r\n\r\n+\r\n\r\n", r, err) == 1);
	EXPECT(r.n() == 3 && r.seq_off[3] == 7 && r.names.size() == 10 && r.quals.size() == r.seqs.size());
	r.clear();
	EXPECT(r.n() == 0 && r.seq_off.size() == 1 && r.name_off.size() == 1 && cut_all("", r, err) == 0 && cut_all("\n", r, err) == -1);
	// a one-base quality line that is as long as the read is the read's quality
	r.clear();
	EXPECT(cut_all("@a\nA\n+\n*\n", r, err) == 1 && r.quals == "*");
	// truncated, malformed, names of 0, 254 and 255 bytes: a refused record leaves what was there
	r.clear();
	EXPECT(cut_all("@a\nACGT\n+\n", r, err) == -1 && err == "Truncated FASTQ record" && r.n() == 0);
	EXPECT(cut_all("a\nACGT\n+\nIIII\n", r, err) == -1 && err == "Malformed FASTQ record");
	EXPECT(cut_all("@a\nACGT\n-\nIIII\n", r, err) == -1 && cut_all("@a\nACGT\n\nIIII\n", r, err) == -1);
	EXPECT(cut_all("@\nACGT\n+\nIIII\n", r, err) == -1 && cut_all("@ x\nACGT\n+\nIIII\n", r, err) == -1 && r.n() == 0 && r.names.empty());
	EXPECT(cut_all("@" + std::string(254, 'n') + "\nACGT\n+\nIIII\n", r, err) == 1 && r.name_off[1] == 255);
	EXPECT(cut_all("@" + std::string(255, 'n') + " c\nACGT\n+\nIIII\n", r, err) == -1 && r.n() == 1 && r.seqs == "ACGT");
	// pieces put together from two texts: ranges that begin and end anywhere, offsets rebased
	seeksv::FastqReads a, b, m;
	const std::string ta = "@a1\nAC\n+\nII\n@a2\n\n+\n\n@a3\nGGG\n+\n*\n", tb = "@b1 c\nT\n+\n#\n", tc = "@a\nAC\n+\nII\n@b\nAC\n";
	EXPECT(seeksv::fastq_all(ta.data(), ta.size(), a, err) == 3 && seeksv::fastq_all(tb.data(), tb.size(), b, err) == 1);
	seeksv::fastq_append_range(m, a, 1, 3); seeksv::fastq_append_range(m, b, 0, 1); seeksv::fastq_append_range(m, a, 0, 1); seeksv::fastq_append_range(m, a, 2, 2);
	EXPECT(m.n() == 4 && m.seqs == "GGGTAC" && m.quals == "!!!#II" && m.names == std::string("a2\0a3\0b1\0a1\0", 12));
	EXPECT(m.seq_off[1] == 0 && m.seq_off[2] == 3 && m.seq_off[3] == 4 && m.seq_off[4] == 6 && m.name_off[2] == 6 && m.name_off[4] == 12);
	EXPECT(seeksv::fastq_all(tc.data(), tc.size(), r, err) == -1 && err == "Truncated FASTQ record");
	if (failures) return 1;
	printf("fastq_reads_check: ok\n");
	return 0;
}
