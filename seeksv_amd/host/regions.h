// regions.h - the BED reader of `seeksv run -L` / `-X`: a file of regions against a header's contigs -> the normalised list that ssv_regions_set takes
// (the rule: include/seeksv_hip.h).  Host code only, no GPU: tests/native/regions_check.cpp runs it under the sanitizers.
//   columns   chrom, start, end, separated by tabs; further columns are ignored.  0-based half-open.
//   skipped   empty lines, and lines that start with '#', "track" or "browser"
//   ignored   a line whose contig the header does not have (counted: blacklists name decoys that a reference may lack)
//   refused   fewer than three fields, a field that is not a number, start < 0, end <= start: "FILE: line N: reason"
// A name that ends in .gz is read through zlib, every other file as plain text.
#pragma once

#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>

namespace seeksv {

struct Region { int32_t tid, s, t; };

struct RegionList {
	std::vector<Region> regions; // normalised: per contig sorted by s, no two overlapping or abutting, t clipped to the contig's length
	int64_t lines = 0;           // lines that named a region
	int64_t unknown = 0;         // of them: lines whose contig the header does not have
	int32_t contigs = 0;         // contigs with at least one region
};

// sorted by (contig, s); regions of one contig that overlap or abut merged; t clipped to the contig's length; a region the clipping leaves empty dropped
inline void normalise_regions(std::vector<Region> &r, const std::vector<int32_t> &lens)
{
	for (Region &x : r) x.t = std::min(x.t, lens[(size_t)x.tid]);
	r.erase(std::remove_if(r.begin(), r.end(), [](const Region &x) { return x.s >= x.t; }), r.end());
	std::sort(r.begin(), r.end(), [](const Region &a, const Region &b) { return a.tid != b.tid ? a.tid < b.tid : a.s < b.s; });
	size_t n = 0;
	for (const Region &x : r) {
		if (n > 0 && r[n - 1].tid == x.tid && x.s <= r[n - 1].t) r[n - 1].t = std::max(r[n - 1].t, x.t);
		else r[n++] = x;
	}
	r.resize(n);
}

// a whole field as a number: an optional '-' and digits, nothing else; values beyond 2^62 saturate there (no contig is that long)
inline bool bed_number(const char *p, const char *end, int64_t *out)
{
	const bool neg = p < end && *p == '-';
	if (neg) ++p;
	if (p == end) return false;
	int64_t v = 0;
	for (; p < end; ++p) {
		if (*p < '0' || *p > '9') return false;
		if (v < ((int64_t)1 << 62) / 10) v = v * 10 + (*p - '0'); else v = (int64_t)1 << 62;
	}
	*out = neg ? -v : v;
	return true;
}

// one line (without its end) -> 0: nothing to take, 1: a region (tid < 0: its contig is unknown), -1: refused, *why says so
inline int bed_line(const char *p, size_t len, const std::unordered_map<std::string, int32_t> &tid_of, const std::vector<int32_t> &lens, Region *out, const char **why)
{
	while (len > 0 && (p[len - 1] == '\r' || p[len - 1] == '\n')) --len;
	if (len == 0 || p[0] == '#') return 0;
	auto starts = [&](const char *w, size_t n) { return len >= n && std::equal(w, w + n, p); };
	if (starts("track", 5) || starts("browser", 7)) return 0;
	const char *end = p + len, *f[4];
	int nf = 0;
	f[nf++] = p;
	for (const char *q = p; q < end && nf < 4; ++q) if (*q == '\t') f[nf++] = q + 1;
	if (nf < 3) { *why = "fewer than three tab-separated fields"; return -1; }
	const char *e2 = nf == 4 ? f[3] - 1 : end;
	int64_t s = 0, t = 0;
	if (!bed_number(f[1], f[2] - 1, &s)) { *why = "start is not a number"; return -1; }
	if (!bed_number(f[2], e2, &t)) { *why = "end is not a number"; return -1; }
	if (s < 0) { *why = "start < 0"; return -1; }
	if (t <= s) { *why = "end <= start"; return -1; }
	const auto it = tid_of.find(std::string(f[0], (size_t)(f[1] - 1 - f[0])));
	if (it == tid_of.end()) { out->tid = -1; return 1; }
	const int64_t L = lens[(size_t)it->second];
	out->tid = it->second;
	out->s = (int32_t)std::min<int64_t>(s, L); // (a region that starts behind its contig's end is left empty by the clipping)
	out->t = (int32_t)std::min<int64_t>(t, L);
	return 1;
}

// Reads `path` against the header's contigs (the first of equal names).  false: *err is the one line to print ("FILE: line N: reason", or that the file
// cannot be read) and `out` is not to be used.
inline bool read_bed(const std::string &path, const std::vector<std::string> &names, const std::vector<int32_t> &lens, RegionList &out, std::string *err)
{
	std::unordered_map<std::string, int32_t> tid_of;
	for (size_t t = 0; t < names.size(); ++t) tid_of.emplace(names[t], (int32_t)t);
	const bool gz = path.size() >= 3 && path.compare(path.size() - 3, 3, ".gz") == 0;
	std::string text;
	{
		char buf[1 << 16];
		if (gz) {
			gzFile f = gzopen(path.c_str(), "rb");
			if (!f) { *err = path + ": cannot open the file"; return false; }
			int n;
			while ((n = gzread(f, buf, sizeof(buf))) > 0) text.append(buf, (size_t)n);
			const bool bad = n < 0;
			gzclose(f);
			if (bad) { *err = path + ": cannot read the file (not gzip, or damaged)"; return false; }
		} else {
			FILE *f = fopen(path.c_str(), "rb");
			if (!f) { *err = path + ": cannot open the file"; return false; }
			size_t n;
			while ((n = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, n);
			const bool bad = ferror(f) != 0;
			fclose(f);
			if (bad) { *err = path + ": cannot read the file"; return false; }
		}
	}
	out = RegionList();
	int64_t line_no = 0;
	for (size_t at = 0; at < text.size();) {
		size_t nl = text.find('\n', at);
		if (nl == std::string::npos) nl = text.size();
		++line_no;
		Region r{0, 0, 0};
		const char *why = nullptr;
		const int rc = bed_line(text.data() + at, nl - at, tid_of, lens, &r, &why);
		if (rc < 0) { *err = path + ": line " + std::to_string(line_no) + ": " + why; return false; }
		if (rc > 0) {
			++out.lines;
			if (r.tid < 0) ++out.unknown; else out.regions.push_back(r);
		}
		at = nl + 1;
	}
	normalise_regions(out.regions, lens);
	for (size_t k = 0; k < out.regions.size(); ++k) if (k == 0 || out.regions[k - 1].tid != out.regions[k].tid) ++out.contigs;
	return true;
}

} // namespace seeksv
