"""CPU: the BED reader of `seeksv run -L` / `-X` (seeksv_amd/host/regions.h) - lines, refusals with their reasons, the normalised list, whole files plain and
gzip - through tests/native/regions_check.cpp; and its normalised list against tests/region_model.py's normalise() on the lists of tests/region_inputs.py."""
import os
import subprocess

import region_inputs as ri
import region_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name, source=None):
    exe = str(tmp_path / name)
    flags = os.environ.get("SSV_TEST_CXXFLAGS", "-O2").split()
    src = source or os.path.join(ROOT, "tests", "native", name + ".cpp")
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "seeksv_amd", "host"), src, "-lz", "-o", exe])
    return exe


def test_regions_check(tmp_path):
    r = subprocess.run([build(tmp_path, "regions_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "regions_check: ok" in r.stdout, r.stdout + r.stderr


PRINTER = r'''
#include <stdio.h>
#include "regions.h"
// argv: BED file, then name length pairs of the header -> the normalised list, one region a line, then the counts
int main(int argc, char **argv)
{
	std::vector<std::string> names;
	std::vector<int32_t> lens;
	for (int k = 2; k + 1 < argc; k += 2) { names.push_back(argv[k]); lens.push_back(atoi(argv[k + 1])); }
	seeksv::RegionList L;
	std::string err;
	if (!seeksv::read_bed(argv[1], names, lens, L, &err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
	for (const seeksv::Region &r : L.regions) printf("%d\t%d\t%d\n", r.tid, r.s, r.t);
	printf("lines %lld unknown %lld contigs %d\n", (long long)L.lines, (long long)L.unknown, L.contigs);
	return 0;
}
'''


def test_the_reader_normalises_as_the_model_does(tmp_path):
    src = str(tmp_path / "printer.cpp")
    with open(src, "w") as f:
        f.write(PRINTER)
    exe = build(tmp_path, "printer", src)
    cases = [(s["regions"], s["lens"], s["targets"]) for s in ri.SETS] + [(ri.cli_bed(), [60000, 60000], ["tA", "tB"])]
    for k, (regions, lens, names) in enumerate(cases):
        bed = str(tmp_path / f"{k}.bed")
        with open(bed, "w") as f:
            f.write(ri.bed_text(regions, names))
        header = [x for n, l in zip(names, lens) for x in (n, str(l))]
        r = subprocess.run([exe, bed] + header, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        want = rm.normalise(regions, lens)
        assert [tuple(int(x) for x in l.split("\t")) for l in out[:-1]] == want, k
        assert out[-1] == f"lines {len(regions)} unknown 0 contigs {len({x[0] for x in want})}"
