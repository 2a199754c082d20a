// fastq_reads.h - whole reads out of FASTQ text, laid out as ssv_realign_split_batch takes them (`seeksv run -P`: the text of prefix.unmapped_[12].fq as
// getclip's side channel wrote it).  No HIP, no file access: `make asan` runs tests/native/fastq_reads_check.cpp over it.
//
// A record is four lines; a line ends at '\n' (a '\r' in front of it is dropped), the last line may lack it.  The read's name is line 1 behind '@' up to the
// first blank or tab ("/1" and "/2" stay), as `seeksv realign -P` takes it.  The qualities are line 4 when it is as long as the bases; every other line 4 -
// getclip writes "*" for a read without qualities - gives '!' (phred 0) for every base, as `seeksv realign` writes such a record.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace seeksv {

struct FastqReads {
	std::string seqs, quals, names;          // bases and qualities back to back at the same offsets; the names with their NULs
	std::vector<uint64_t> seq_off, name_off; // [n + 1]
	FastqReads() : seq_off(1, 0), name_off(1, 0) {}
	int64_t n() const { return (int64_t)seq_off.size() - 1; }
	void clear() { seqs.clear(); quals.clear(); names.clear(); seq_off.assign(1, 0); name_off.assign(1, 0); }
};

// One line of text[at, size): -> false at the end of the text (an empty last line without '\n' is no line)
inline bool fastq_line(const char *text, size_t size, size_t &at, const char *&p, size_t &len)
{
	if (at >= size) return false;
	p = text + at;
	const char *e = static_cast<const char *>(memchr(p, '\n', size - at));
	len = e ? (size_t)(e - p) : size - at;
	at += len + (e ? 1 : 0);
	if (e && len && p[len - 1] == '\r') --len;
	return e != nullptr || len != 0;
}

// The next record of text[at, size) appended to `out`.  -> 1 a record, 0 the end of the text, -1 a truncated or malformed record or a name that is empty or
// longer than 254 bytes (`err` says which; `out` is as it was)
inline int fastq_next(const char *text, size_t size, size_t &at, FastqReads &out, std::string &err)
{
	const char *l1, *l2, *l3, *l4;
	size_t n1, n2, n3, n4;
	if (!fastq_line(text, size, at, l1, n1)) return 0;
	if (!fastq_line(text, size, at, l2, n2) || !fastq_line(text, size, at, l3, n3) || !fastq_line(text, size, at, l4, n4)) { err = "Truncated FASTQ record"; return -1; }
	if (n1 == 0 || l1[0] != '@' || n3 == 0 || l3[0] != '+') { err = "Malformed FASTQ record"; return -1; }
	size_t k = 1;
	while (k < n1 && l1[k] != ' ' && l1[k] != '\t') ++k;
	if (k - 1 == 0 || k - 1 > 254) { err = "A read name is empty or longer than 254 bytes"; return -1; }
	out.names.append(l1 + 1, k - 1); out.names.push_back('\0');
	out.name_off.push_back(out.names.size());
	out.seqs.append(l2, n2);
	if (n4 == n2) out.quals.append(l4, n4); else out.quals.append(n2, '!');
	out.seq_off.push_back(out.seqs.size());
	return 1;
}

// Every record of text[0, size) appended to `out` -> the number of records, or -1 (`err` says why; the records before the refused one are in `out`)
inline int64_t fastq_all(const char *text, size_t size, FastqReads &out, std::string &err)
{
	size_t at = 0;
	int64_t n = 0;
	for (int rc; (rc = fastq_next(text, size, at, out, err)) != 0; ++n)
		if (rc < 0) return -1;
	return n;
}

// The reads [i0, i1) of `src` appended to `dst` (a piece of reads is put together from texts that were cut side by side)
inline void fastq_append_range(FastqReads &dst, const FastqReads &src, int64_t i0, int64_t i1)
{
	if (i1 <= i0) return;
	const uint64_t s0 = src.seq_off[(size_t)i0], s1 = src.seq_off[(size_t)i1], n0 = src.name_off[(size_t)i0], n1 = src.name_off[(size_t)i1];
	const uint64_t sb = dst.seqs.size(), nb = dst.names.size();
	dst.seqs.append(src.seqs, (size_t)s0, (size_t)(s1 - s0)); dst.quals.append(src.quals, (size_t)s0, (size_t)(s1 - s0)); dst.names.append(src.names, (size_t)n0, (size_t)(n1 - n0));
	for (int64_t i = i0 + 1; i <= i1; ++i) { dst.seq_off.push_back(src.seq_off[(size_t)i] - s0 + sb); dst.name_off.push_back(src.name_off[(size_t)i] - n0 + nb); }
}

} // namespace seeksv
