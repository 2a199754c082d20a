// CPU check of seeksv_amd/host/regions.h (the BED reader of `seeksv run -L` / `-X`): lines in memory of exactly their size, so that a read past either
// end is an error under AddressSanitizer; the normalised list; whole files, plain and gzip.  Built and run by `make asan`.  Exit code 0 = every case gave
// what it should.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <memory>
#include <string>

#include "regions.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const std::vector<std::string> kNames = {"c0", "c1", "c0"}; // (a name twice: the first one counts)
static const std::vector<int32_t> kLens = {100, 64, 7};

// one line in memory of exactly its size -> bed_line's answer
static int line(const std::string &text, seeksv::Region *r, std::string *why)
{
	std::unordered_map<std::string, int32_t> tid_of;
	for (size_t t = 0; t < kNames.size(); ++t) tid_of.emplace(kNames[t], (int32_t)t);
	std::unique_ptr<char[]> exact(new char[text.size() ? text.size() : 1]);
	memcpy(exact.get(), text.data(), text.size());
	const char *w = nullptr;
	const int rc = seeksv::bed_line(exact.get(), text.size(), tid_of, kLens, r, &w);
	*why = w ? w : "";
	return rc;
}

static std::string write_file(const std::string &dir, const char *name, const std::string &text, bool gz)
{
	const std::string path = dir + "/" + name;
	if (gz) { gzFile f = gzopen(path.c_str(), "wb"); gzwrite(f, text.data(), (unsigned)text.size()); gzclose(f); }
	else { FILE *f = fopen(path.c_str(), "wb"); fwrite(text.data(), 1, text.size(), f); fclose(f); }
	return path;
}

static bool same(const std::vector<seeksv::Region> &a, std::initializer_list<seeksv::Region> b)
{
	if (a.size() != b.size()) return false;
	size_t k = 0;
	for (const seeksv::Region &x : b) { if (a[k].tid != x.tid || a[k].s != x.s || a[k].t != x.t) return false; ++k; }
	return true;
}

int main()
{
	seeksv::Region r{0, 0, 0};
	std::string why;
	// three fields, further fields, a carriage return; what is skipped; an unknown contig
	EXPECT(line("c1\t10\t20", &r, &why) == 1 && r.tid == 1 && r.s == 10 && r.t == 20);
	EXPECT(line("c1\t10\t20\tname\t0\t+\r\n", &r, &why) == 1 && r.tid == 1 && r.s == 10 && r.t == 20);
	EXPECT(line("c0\t0\t1\t", &r, &why) == 1 && r.tid == 0 && r.s == 0 && r.t == 1);
	EXPECT(line("", &r, &why) == 0 && line("\r", &r, &why) == 0 && line("#c1\t1\t2", &r, &why) == 0 && line("track name=x", &r, &why) == 0 && line("browser hide all", &r, &why) == 0);
	EXPECT(line("chrUn\t5\t9", &r, &why) == 1 && r.tid == -1);
	EXPECT(line("tracks\t5\t9", &r, &why) == 0); // (starts with "track": skipped, as the rule says)
	// clipped to the contig where it is read: past the end, and behind it altogether
	EXPECT(line("c1\t60\t70", &r, &why) == 1 && r.s == 60 && r.t == 64);
	EXPECT(line("c1\t64\t70", &r, &why) == 1 && r.s == 64 && r.t == 64);
	EXPECT(line("c1\t5000000000\t9000000000000000000000", &r, &why) == 1 && r.s == 64 && r.t == 64);
	// refused, with the reason
	EXPECT(line("c1\t10", &r, &why) == -1 && why == "fewer than three tab-separated fields");
	EXPECT(line("c1 10 20", &r, &why) == -1 && why == "fewer than three tab-separated fields");
	EXPECT(line("c1\tx\t20", &r, &why) == -1 && why == "start is not a number" && line("c1\t\t20", &r, &why) == -1 && line("c1\t1e3\t2000", &r, &why) == -1 && line("c1\t-\t20", &r, &why) == -1);
	EXPECT(line("c1\t10\t2o", &r, &why) == -1 && why == "end is not a number" && line("c1\t10\t", &r, &why) == -1 && why == "end is not a number" && line("c1\t10\t \t", &r, &why) == -1);
	EXPECT(line("c1\t-1\t20", &r, &why) == -1 && why == "start < 0");
	EXPECT(line("c1\t10\t10", &r, &why) == -1 && why == "end <= start" && line("c1\t10\t9", &r, &why) == -1 && line("chrUn\t10\t-3", &r, &why) == -1 && why == "end <= start");

	// normalised: sorted, overlapping and abutting regions merged, clipped, empty ones dropped
	std::vector<seeksv::Region> v = {{1, 40, 41}, {1, 20, 25}, {1, 60, 70}, {1, 10, 20}, {0, 5, 9}, {1, 12, 14}, {1, 64, 90}, {0, 8, 30}, {0, 31, 32}};
	seeksv::normalise_regions(v, kLens);
	EXPECT(same(v, {{0, 5, 30}, {0, 31, 32}, {1, 10, 25}, {1, 40, 41}, {1, 60, 64}}));
	v.clear();
	seeksv::normalise_regions(v, kLens);
	EXPECT(v.empty());

	// whole files
	char tmpl[] = "/tmp/regions_check.XXXXXX";
	const char *dir = mkdtemp(tmpl);
	if (!dir) { perror("mkdtemp"); return 1; }
	const std::string text = "# targets\ntrack name=t\n\nc1\t20\t25\tx\nc1\t10\t20\r\nchrUn\t1\t2\nc0\t90\t200\nc1\t60\t70"; // (the last line without its newline)
	seeksv::RegionList L;
	std::string err;
	for (int gz = 0; gz < 2; ++gz) {
		const std::string path = write_file(dir, gz ? "a.bed.gz" : "a.bed", text, gz != 0);
		EXPECT(seeksv::read_bed(path, kNames, kLens, L, &err));
		EXPECT(same(L.regions, {{0, 90, 100}, {1, 10, 25}, {1, 60, 64}}) && L.lines == 5 && L.unknown == 1 && L.contigs == 2);
		unlink(path.c_str());
	}
	std::string path = write_file(dir, "bad.bed", "c1\t1\t2\n\n#x\nc1\t5\n", false);
	EXPECT(!seeksv::read_bed(path, kNames, kLens, L, &err) && err == path + ": line 4: fewer than three tab-separated fields");
	unlink(path.c_str());
	path = write_file(dir, "empty.bed", "", false);
	EXPECT(seeksv::read_bed(path, kNames, kLens, L, &err) && L.regions.empty() && L.lines == 0 && L.contigs == 0);
	unlink(path.c_str());
	path = write_file(dir, "plain.bed.gz", "c1\t1\t2\n", false); // (a .gz name over plain text: zlib hands plain text through)
	EXPECT(seeksv::read_bed(path, kNames, kLens, L, &err) && L.regions.size() == 1);
	unlink(path.c_str());
	EXPECT(!seeksv::read_bed(std::string(dir) + "/none.bed", kNames, kLens, L, &err) && err.find("cannot open the file") != std::string::npos);
	rmdir(dir);
	if (failures) return 1;
	printf("regions_check: ok\n");
	return 0;
}
