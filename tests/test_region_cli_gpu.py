"""-m gpu, through the binary: `seeksv run -L bed` / `-X bed` write what `seeksv run` writes on a file that holds the records the rule keeps
(tests/region_model.py) - every file byte for byte and stdout, except prefix.unmapped_[12].fq.gz, which are not restricted -, in one chunk and in chunks of
1 MB; with -u on a shuffled file the kept records in the sorted order (tests/coordsort_model.py); with -D and -M the expected file carries the flags that the
rule sets on the WHOLE sample (tests/pairdup_model.py, tests/markdup_model.py) - the mates of junction A's marked reads lie outside every region;
`somatic -K -L`; a BED with an unknown contig, comment lines and further columns, plain and gzip; the refusals; malformed lines with their numbers.
Sample: tests/pairdup_cli_inputs.py and tests/coordsort_inputs.py (cli_sample); the BED: tests/region_inputs.py (cli_bed), held to its properties on the CPU
in tests/test_region_inputs.py."""
import glob
import gzip
import os
import re
import subprocess

import pytest

import bamio
import coordsort_inputs as ci
import coordsort_model as cm
import markdup_cli_inputs as CI
import pairdup_cli_inputs as PI
import region_inputs as ri
import region_model as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
SV_OPTS = ["-v", "-b 3"]
NAMES, LENS = list(PI.NAMES), list(PI.LENS)
CHUNKED = {"SSV_CHUNK_INFLATED_MB": "1", "SSV_SORT_BATCH_RECORDS": "5000", "SSV_SAM_CHUNK_KB": "1024"}
BED = ri.cli_bed(LENS)


def kept(recs, exclude=False):
    return [recs[i] for i in rm.keep(recs, BED, exclude)]


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("region_cli")
    contigs, recs = PI.sample()
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for name, c in zip(NAMES, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 70] for i in range(0, len(c), 70)) + "\n")
    files, counts = {}, {}

    def bam(tag, records):
        files[tag] = str(d / f"{tag}.bam")
        counts[tag] = len(records)
        bamio.write_bam(files[tag], NAMES, LENS, records)

    bam("plain", recs)
    bam("want_L", kept(recs))
    bam("want_X", kept(recs, True))
    shuffled = ci.shuffled(recs)
    bam("shuffled", shuffled)
    sel = kept(shuffled)                                          # restricted in input order, then sorted by the sort's rule
    bam("want_uL", [sel[i] for i in cm.order(sel, len(NAMES))])
    bam("want_DL", kept(PI.flagged(recs)))                        # the flags of the whole sample, then the restriction
    plain_m = ci.cli_sample()[1]                                  # (-M's sample: the copies lie at one place)
    bam("plain_M", plain_m)
    bam("want_ML", kept(CI.flagged(plain_m)))
    bed = str(d / "regions.bed")
    with open(bed, "w") as f:
        f.write(ri.bed_text(BED, NAMES))
    return d, fa, files, counts, bed


def run(args, env=None):
    r = subprocess.run([SEEKSV] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (args, r.stderr[-800:])
    return r


def same_outputs(a, b):
    """every file of the two prefixes but prefix.unmapped_[12].fq.gz, which are not restricted"""
    for ext in (".clip.gz", ".clip.fq.gz"):
        assert gzip.open(a + ext, "rb").read() == gzip.open(b + ext, "rb").read(), ext
    for ext in (".sv.txt", ".unmapped.clip.fq"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert bamio.read_bam_records(a + ".clip.bam") == bamio.read_bam_records(b + ".clip.bam")
    assert sorted(os.path.basename(x)[len(os.path.basename(a)):] for x in glob.glob(a + ".*")) == sorted(os.path.basename(x)[len(os.path.basename(b)):] for x in glob.glob(b + ".*"))


def closing_line(r, opt, n_kept, n_in):
    lines = [l for l in r.stderr.splitlines() if l.startswith(f"[seeksv] {opt}:") and " kept " in l]
    norm = rm.normalise(BED, LENS)
    assert lines == [f"[seeksv] {opt}: kept {n_kept} of {n_in} records ({len(norm)} regions on {len({x[0] for x in norm})} contigs)"], r.stderr[-800:]


@pytest.fixture(scope="module")
def expected(sample):
    """`seeksv run` on a file of the sample, once per way of reading it: (prefix, stdout)"""
    d, fa, files, _, _ = sample
    made = {}

    def get(tag, chunked=False):
        if (tag, chunked) not in made:
            pre = str(d / f"expect_{tag}_{'c' if chunked else 'w'}")
            r = run(["run"] + SV_OPTS + [files[tag], fa, pre], CHUNKED if chunked else None)
            assert "[seeksv] -L:" not in r.stderr and "[seeksv] -X:" not in r.stderr
            made[(tag, chunked)] = (pre, r.stdout)
        return made[(tag, chunked)]
    return get


@pytest.mark.parametrize("chunked", [False, True], ids=["one-chunk", "chunks-of-1MB"])
@pytest.mark.parametrize("opt", ["-L", "-X"])
def test_run_L_and_X_equal_run_on_the_filtered_file(sample, expected, opt, chunked):
    d, fa, files, counts, bed = sample
    pre = str(d / f"got{opt}_{'c' if chunked else 'w'}")
    r = run(["run", opt, bed] + SV_OPTS + [files["plain"], fa, pre], dict(CHUNKED if chunked else {}, SSV_TIMING="2"))
    want, want_stdout = expected("want_" + opt[1], chunked)
    same_outputs(pre, want)
    assert r.stdout == want_stdout
    closing_line(r, opt, counts["want_" + opt[1]], counts["plain"])
    chunks = sum(1 for l in r.stderr.splitlines() if l.startswith("[timing] (chunk of ") and " 0 blocks" not in l)
    assert chunks >= 7 if chunked else chunks == 1
    m = re.search(r"\(-[LX] kernel time: region_select ([0-9.e+-]+) ms in (\d+) launches, region_gather ([0-9.e+-]+) ms in (\d+) launches\)", r.stderr)
    assert m and int(m.group(2)) > 0 and int(m.group(4)) > 0
    # the restriction changes what the passes see (the comparison is not one of empty tables: the clipped reads of one junction lie inside the regions, those
    # of the other outside)
    plain, _ = expected("plain", chunked)
    rows = gzip.open(pre + ".clip.gz", "rb").read()
    assert rows and rows != gzip.open(plain + ".clip.gz", "rb").read() and rows != gzip.open(expected("want_" + ("X" if opt == "-L" else "L"), chunked)[0] + ".clip.gz", "rb").read()
    # the side channel is not restricted: the unmapped pairs are those of the unrestricted run, byte for byte
    for ext in (".unmapped_1.fq.gz", ".unmapped_2.fq.gz"):
        got = gzip.open(pre + ext, "rb").read()
        assert got == gzip.open(plain + ext, "rb").read() and got.count(b"\n") == 4 * ci.N_HALF_MAPPED, ext
        assert got != gzip.open(want + ext, "rb").read()          # (the filtered file holds fewer of them)


def test_run_u_L_on_a_shuffled_file(sample, expected):
    d, fa, files, counts, bed = sample
    pre = str(d / "got_uL")
    r = run(["run", "-u", "-L", bed] + SV_OPTS + [files["shuffled"], fa, pre], CHUNKED)
    want, want_stdout = expected("want_uL", True)
    same_outputs(pre, want)
    assert r.stdout == want_stdout
    closing_line(r, "-L", counts["want_uL"], counts["shuffled"])
    m = re.search(r"\[seeksv\] -u: sorted (\d+) records from (\d+) into (\d+) batches", r.stderr)
    assert m and int(m.group(1)) == counts["want_uL"]           # the sort sees the kept records only


@pytest.mark.parametrize("chunked", [False, True], ids=["one-chunk", "chunks-of-1MB"])
def test_run_D_L_carries_the_flags_of_the_whole_input(sample, expected, chunked):
    d, fa, files, counts, bed = sample
    pre = str(d / f"got_DL_{'c' if chunked else 'w'}")
    r = run(["run", "-D", "-L", bed] + SV_OPTS + [files["plain"], fa, pre], CHUNKED if chunked else None)
    want, want_stdout = expected("want_DL", chunked)
    same_outputs(pre, want)
    assert r.stdout == want_stdout
    closing_line(r, "-L", counts["want_DL"], counts["plain"])
    assert len([l for l in r.stderr.splitlines() if l.startswith("[seeksv] -D: marked ")]) == 1
    # restricting first and marking then would not find the copies: their mates lie outside the regions
    unmarked, _ = expected("want_L", chunked)
    assert gzip.open(unmarked + ".clip.gz", "rb").read() != gzip.open(pre + ".clip.gz", "rb").read()


def test_run_M_L_carries_the_flags_of_the_whole_input(sample, expected):
    d, fa, files, counts, bed = sample
    pre = str(d / "got_ML")
    r = run(["run", "-M", "-L", bed] + SV_OPTS + [files["plain_M"], fa, pre], CHUNKED)
    want, want_stdout = expected("want_ML", True)
    same_outputs(pre, want)
    assert r.stdout == want_stdout
    closing_line(r, "-L", counts["want_ML"], counts["plain_M"])
    assert "[seeksv] -M: marked " in r.stderr


def test_somatic_K_L_equals_somatic_K_on_the_filtered_normal(sample, expected, tmp_path):
    d, fa, files, counts, bed = sample
    tumor = expected("plain")[0] + ".sv.txt"
    outs = {}
    for tag, args in (("l", ["-L", bed, files["plain"]]), ("f", [files["want_L"]]), ("x", ["-X", bed, files["plain"]]), ("fx", [files["want_X"]]), ("u", [files["plain"]])):
        out = str(tmp_path / f"{tag}.somatic.sv")
        r = run(["somatic", "-K"] + args + [tumor, out])
        outs[tag] = (open(out).read(), r)
        assert sorted(os.listdir(tmp_path)) == sorted(f"{t}.somatic.sv" for t in outs)       # writes no other file
    assert outs["l"][0] == outs["f"][0] and outs["x"][0] == outs["fx"][0]
    closing_line(outs["l"][1], "-L", counts["want_L"], counts["plain"])
    closing_line(outs["x"][1], "-X", counts["want_X"], counts["plain"])
    assert "[seeksv] -L:" not in outs["f"][1].stderr and "[seeksv] -L:" not in outs["u"][1].stderr
    # a malformed BED is refused here too, with its line, and no file is written
    bad = str(tmp_path / "bad.bed")
    with open(bad, "w") as f:
        f.write("tA\t10\t20\ntA\t30\n")
    before = sorted(os.listdir(tmp_path))
    r = subprocess.run([SEEKSV, "somatic", "-K", "-L", bad, files["plain"], tumor, str(tmp_path / "bad.somatic.sv")], capture_output=True, text=True)
    assert r.returncode == 1 and bed_lines(r, bad) == [f"{bad}: line 2: fewer than three tab-separated fields"] and sorted(os.listdir(tmp_path)) == before


def test_a_bed_with_an_unknown_contig_comments_and_further_columns(sample, expected, tmp_path):
    d, fa, files, counts, bed = sample
    lines = ["# a comment", "track name=targets", "browser position tA:1-100", ""]
    for k, (t, s, e) in enumerate(BED):
        lines.append(f"{NAMES[t]}\t{s}\t{e}" + (f"\ttarget{k}\t0\t+" if k % 2 else ""))
        if k == 3:
            lines += ["chrUn_decoy\t0\t5000\tdecoy", "", "#chrUn_decoy\t1\t2"]
    lines.append("HLA-A\t100\t200")
    text = "\n".join(lines) + "\n"
    plain_bed, gz_bed = str(tmp_path / "targets.bed"), str(tmp_path / "targets.bed.gz")
    with open(plain_bed, "w") as f:
        f.write(text.replace("\n", "\r\n", 3))                   # (a few lines with a carriage return)
    with gzip.open(gz_bed, "wt") as f:
        f.write(text)
    want, want_stdout = expected("want_L")
    for k, path in enumerate((plain_bed, gz_bed)):
        pre = str(tmp_path / f"got{k}")
        r = run(["run", "-L", path] + SV_OPTS + [files["plain"], fa, pre])
        same_outputs(pre, want)
        assert r.stdout == want_stdout
        closing_line(r, "-L", counts["want_L"], counts["plain"])
        unknown = [l for l in r.stderr.splitlines() if "name a contig that the input's header does not have" in l]
        assert len(unknown) == 1 and unknown[0].startswith(f"[seeksv] -L: 2 of {len(BED) + 2} lines of {path} ")


def one_line(r):
    return [l for l in r.stderr.splitlines() if not l.startswith("[stamp]")]


def bed_lines(r, path):
    """what stderr says about the file"""
    return [l for l in r.stderr.splitlines() if l.startswith(path + ": ")]


def test_refusals(sample, tmp_path):
    d, fa, files, _, bed = sample
    bam = files["plain"]
    cases = [(["run", "-L", bed, "-X", bed, bam, fa], "seeksv run: -L", "-X"), (["run", "-L", bed, "-N", "2", bam, fa], "seeksv run: -L", "-N"),
             (["run", "-X", bed, "-N", "2", bam, fa], "seeksv run: -X", "-N"), (["run", "-c", f"-L {bed}", bam, fa], "seeksv run: -L and -X", "-c"),
             (["run", "-c", f"-X {bed}", bam, fa], "seeksv run: -L and -X", "-c"), (["run", "-v", f"-b 3 -X {bed}", bam, fa], "seeksv run: -L and -X", "-v"),
             (["somatic", "-L", bed, bam, "x.clip.gz", "t.sv"], "seeksv somatic: -L and -X", "-K"), (["somatic", "-X", bed, bam, "x.clip.gz", "t.sv"], "seeksv somatic: -L and -X", "-K"),
             (["somatic", "-K", "-L", bed, "-X", bed, bam, "t.sv"], "seeksv somatic: -L", "-X")]
    for k, (args, start, word) in enumerate(cases):
        pre = str(tmp_path / f"refused{k}")
        r = subprocess.run([SEEKSV] + args + [pre], capture_output=True, text=True)
        lines = one_line(r)
        assert r.returncode == 1 and len(lines) == 1 and lines[0].startswith(start) and word in lines[0], (args, r.stderr)
        assert not glob.glob(pre + "*")
    # a file that is not there
    pre = str(tmp_path / "nofile")
    r = subprocess.run([SEEKSV, "run", "-L", str(tmp_path / "none.bed"), bam, fa, pre], capture_output=True, text=True)
    assert r.returncode == 1 and any("none.bed: cannot open the file" in l for l in one_line(r)) and not glob.glob(pre + "*")
    # getclip and realign have no such options; getsv's -L is its flank length, as before, also inside -v
    for cmd in ("getclip", "realign"):
        r = subprocess.run([SEEKSV, cmd, "-X", bed, bam], capture_output=True, text=True)
        assert r.returncode == 1 and f"seeksv {cmd}" in r.stderr
    r = subprocess.run([SEEKSV, "getsv", "-X", bed, bam], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage: seeksv getsv" in r.stderr
    # the first usage line of both commands stays as it was, and both usage texts name the options, the rule and the exception
    for cmd, first in (("run", "Usage: seeksv run [options] <input.sorted.bam> <reference fasta(.gz)> <output prefix>"), ("somatic", "Usage: seeksv somatic [options] <input normal original bam>")):
        r = subprocess.run([SEEKSV, cmd], capture_output=True, text=True)
        assert r.stderr.splitlines()[0].startswith(first) and "         -L <file>" in r.stderr and "         -X <file>" in r.stderr
    r = subprocess.run([SEEKSV, "run"], capture_output=True, text=True)
    assert "prefix.unmapped_[12].fq.gz, which are not restricted" in r.stderr and "no external tool was matched" in r.stderr


MALFORMED = [("tA\t10\n", 1, "fewer than three"), ("tA\t10\t20\ntA 30 40\n", 2, "fewer than three"), ("# c\n\ntA\tten\t20\n", 3, "start is not a number"),
             ("tA\t10\t20\ntA\t30\t4o\n", 2, "end is not a number"), ("tA\t-1\t20\n", 1, "start < 0"), ("tA\t10\t20\ntB\t5\t5\n", 2, "end <= start"),
             ("tA\t10\t20\nchrUn\t9\t3\n", 2, "end <= start"), ("tA\t10\t\n", 1, "end is not a number"), ("tA\t1.5\t20\n", 1, "start is not a number")]


@pytest.mark.parametrize("text,line,reason", MALFORMED, ids=[f"{m[2].replace(' ', '_')}-{k}" for k, m in enumerate(MALFORMED)])
def test_malformed_lines_are_refused_with_their_number(sample, tmp_path, text, line, reason):
    d, fa, files, _, _ = sample
    bed = str(tmp_path / "bad.bed")
    with open(bed, "w") as f:
        f.write(text)
    r = subprocess.run([SEEKSV, "run", "-X", bed, files["plain"], fa, str(tmp_path / "out")], capture_output=True, text=True)
    lines = bed_lines(r, bed)
    assert r.returncode == 1 and len(lines) == 1 and lines[0].startswith(f"{bed}: line {line}: ") and reason in lines[0] and r.stderr.rstrip().endswith(lines[0]), r.stderr
    assert sorted(os.listdir(tmp_path)) == ["bad.bed"] and r.stdout == ""
