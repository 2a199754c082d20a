"""-m gpu, through the binary: `seeksv run -D` on a file whose duplicates are not marked writes what `seeksv run` writes on the same records with the pair
rule's flags set (tests/pairdup_model.py) - every file byte for byte and stdout -, in one chunk and in chunks of 1 MB; `run -u -D` on the records in any order
what `run` writes on them marked in that order and then sorted by tests/coordsort_model.py (prefix.unmapped_[12].fq.gz: the same pairs), as BAM and as SAM
text in read-name order through standard input, plain and gzip; `somatic -K -D`; the closing line on stderr; the refusals; `run`, `run -M` and `run -u` on the
same files as before.  Sample: tests/pairdup_cli_inputs.py, held to its properties on the CPU in tests/test_pairdup_cli_inputs.py."""
import collections
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
import markdup_inputs as mi
import pairdup_cli_inputs as PI
import pairdup_model as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
SV_OPTS = ["-v", "-b 3"]
NAMES, LENS = list(PI.NAMES), list(PI.LENS)
CHUNKED = {"SSV_CHUNK_INFLATED_MB": "1", "SSV_SORT_BATCH_RECORDS": "5000", "SSV_SAM_CHUNK_KB": "1024"}


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairdup_cli")
    contigs, recs = PI.sample()
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for name, c in zip(NAMES, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 70] for i in range(0, len(c), 70)) + "\n")
    files = {}

    def bam(tag, records):
        files[tag] = str(d / f"{tag}.bam")
        bamio.write_bam(files[tag], NAMES, LENS, records)

    bam("plain", recs)
    bam("flagged", PI.flagged(recs))
    bam("flagged_by_M", PI.flagged_by_M(recs))
    for tag, make in (("shuffled", ci.shuffled), ("name", ci.by_name)):
        order = make(recs)
        bam(tag, order)
        marked = PI.flagged(order)                                 # marked in the order given, then sorted by the sort's rule
        bam(tag + "_marked_sorted", [marked[i] for i in cm.order(marked, len(NAMES))])
        bam(tag + "_sorted", [order[i] for i in cm.order(order, len(NAMES))])
    text = ci.sam_header(NAMES, LENS).encode() + mi.sam_text(ci.by_name(recs), NAMES)
    files["sam"], files["sam_gz"] = str(d / "name.sam"), str(d / "name.sam.gz")
    with open(files["sam"], "wb") as f:
        f.write(text)
    with gzip.open(files["sam_gz"], "wb", compresslevel=1) as f:
        f.write(text)
    st = {}
    pm.mark(list(recs), stats=st)
    return d, fa, files, st


def run(args, env=None, stdin=None):
    r = subprocess.run([SEEKSV] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})), stdin=stdin)
    assert r.returncode == 0, (args, r.stderr[-800:])
    return r


def fastq_pairs(prefix):
    def records(path):
        lines = gzip.open(path, "rt").read().splitlines()
        assert len(lines) % 4 == 0
        return [tuple(lines[k:k + 4]) for k in range(0, len(lines), 4)]
    one, two = records(prefix + ".unmapped_1.fq.gz"), records(prefix + ".unmapped_2.fq.gz")
    assert len(one) == len(two)
    return collections.Counter(zip(one, two))


def same_outputs(a, b, unmapped_in_order=True):
    for ext in (".clip.gz", ".clip.fq.gz") + ((".unmapped_1.fq.gz", ".unmapped_2.fq.gz") if unmapped_in_order else ()):
        assert gzip.open(a + ext, "rb").read() == gzip.open(b + ext, "rb").read(), ext
    for ext in (".sv.txt", ".unmapped.clip.fq"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert bamio.read_bam_records(a + ".clip.bam") == bamio.read_bam_records(b + ".clip.bam")
    assert sorted(os.path.basename(x)[len(os.path.basename(a)):] for x in glob.glob(a + ".*")) == sorted(os.path.basename(x)[len(os.path.basename(b)):] for x in glob.glob(b + ".*"))
    pa, pb = fastq_pairs(a), fastq_pairs(b)
    assert pa == pb and sum(pa.values()) == ci.N_HALF_MAPPED


def closing_line(r, st):
    lines = [l for l in r.stderr.splitlines() if l.startswith("[seeksv] -D:")]
    assert lines == [f"[seeksv] -D: marked {st['pairs_marked']} duplicate pairs ({st['groups_many']} groups of two or more) of {st['pairs']} pairs; {st['unpaired']} of "
                     f"{st['taking_part']} records that take part have no mate by name, {st['records']} records"], r.stderr[-800:]


@pytest.fixture(scope="module")
def expected(sample):
    """`seeksv run` on a file of the sample, once per way of reading it: (prefix, stdout)"""
    d, fa, files, _ = sample
    made = {}

    def get(tag, chunked=False):
        if (tag, chunked) not in made:
            pre = str(d / f"want_{tag}_{'c' if chunked else 'w'}")
            r = run(["run"] + SV_OPTS + [files[tag], fa, pre], CHUNKED if chunked else None)
            assert "[seeksv] -D:" not in r.stderr and "[seeksv] -M:" not in r.stderr and "[seeksv] -u:" not in r.stderr
            made[(tag, chunked)] = (pre, r.stdout)
        return made[(tag, chunked)]
    return get


@pytest.mark.parametrize("chunked", [False, True], ids=["one-chunk", "chunks-of-1MB"])
def test_run_D_equals_run_on_the_flagged_bam(sample, expected, chunked):
    d, fa, files, st = sample
    pre = str(d / f"got_D_{'c' if chunked else 'w'}")
    env = dict(CHUNKED if chunked else {}, SSV_TIMING="2")
    r = run(["run", "-D"] + SV_OPTS + [files["plain"], fa, pre], env)
    want, want_stdout = expected("flagged", chunked)
    same_outputs(pre, want)
    assert r.stdout == want_stdout
    closing_line(r, st)
    chunks = sum(1 for l in r.stderr.splitlines() if l.startswith("[timing] (chunk of ") and " 0 blocks" not in l)
    assert chunks >= 7 if chunked else chunks == 1
    m = re.search(r"\(-D kernel time: pairdup_ends ([0-9.e+-]+) ms in (\d+) launches, pairdup_join ([0-9.e+-]+) ms in (\d+) launches, pairdup_mark ([0-9.e+-]+) ms in (\d+) launches; "
                  r"resident at the peak beside the records: (\d+) bytes of rows, (\d+) bytes of keys and indices\)", r.stderr)
    assert m and all(int(m.group(k)) > 0 for k in (2, 4, 6)) and int(m.group(7)) == 24 * st["records"]
    # marking changes what the passes see: without it the copies count, and -M's rule does not find them
    plain, _ = expected("plain", chunked)
    assert gzip.open(plain + ".clip.gz", "rb").read() != gzip.open(pre + ".clip.gz", "rb").read()
    table, without = open(pre + ".sv.txt").read(), open(plain + ".sv.txt").read()
    assert CI.names_both_ends(without, CI.JUNCTION_B)
    assert not CI.names_both_ends(table, CI.JUNCTION_A) and CI.names_both_ends(table, CI.JUNCTION_B)
    if not chunked:                                                # -D on a file that is marked already changes nothing
        again = str(d / "got_D_again")
        run(["run", "-D"] + SV_OPTS + [files["flagged"], fa, again])
        same_outputs(again, want)


@pytest.mark.parametrize("tag,chunked", [("shuffled", False), ("name", True)])
def test_run_u_D_on_a_bam_in_any_order(sample, expected, tag, chunked):
    d, fa, files, st = sample
    pre = str(d / f"got_uD_{tag}")
    r = run(["run", "-u", "-D"] + SV_OPTS + [files[tag], fa, pre], CHUNKED if chunked else None)
    want, want_stdout = expected(tag + "_marked_sorted", chunked)
    same_outputs(pre, want, unmapped_in_order=False)
    assert r.stdout == want_stdout
    closing_line(r, st)
    assert len([l for l in r.stderr.splitlines() if l.startswith("[seeksv] -u: sorted ")]) == 1


@pytest.mark.parametrize("form", ["sam", "sam_gz"])
def test_run_u_D_on_sam_text_through_standard_input(sample, expected, form):
    d, fa, files, st = sample
    chunked = form == "sam_gz"
    pre = str(d / f"got_uD_{form}")
    with open(files[form], "rb") as f:
        r = run(["run", "-u", "-D"] + SV_OPTS + ["-", fa, pre], CHUNKED if chunked else None, stdin=f)
    want, want_stdout = expected("name_marked_sorted", chunked)
    same_outputs(pre, want, unmapped_in_order=False)
    assert r.stdout == want_stdout
    closing_line(r, st)


def test_run_D_on_sorted_sam_text(sample, expected, tmp_path):
    d, fa, files, st = sample
    sam = str(tmp_path / "sorted.sam")
    with open(sam, "wb") as f:
        f.write(ci.sam_header(NAMES, LENS).encode() + mi.sam_text(PI.sample()[1], NAMES))
    pre = str(tmp_path / "got")
    r = run(["run", "-D"] + SV_OPTS + [sam, fa, pre], CHUNKED)
    want, want_stdout = expected("flagged", True)
    same_outputs(pre, want)
    assert r.stdout == want_stdout
    closing_line(r, st)


def test_somatic_K_D_equals_somatic_K_on_the_flagged_normal(sample, expected, tmp_path):
    d, fa, files, st = sample
    tumor = expected("plain")[0] + ".sv.txt"
    outs = {}
    for tag, args in (("d", ["-D", files["plain"]]), ("f", [files["flagged"]]), ("u", [files["plain"]])):
        out = str(tmp_path / f"{tag}.somatic.sv")
        r = run(["somatic", "-K"] + args + [tumor, out])
        outs[tag] = (open(out).read(), r)
        assert sorted(os.listdir(tmp_path)) == sorted(f"{t}.somatic.sv" for t in outs)       # writes no other file
    assert outs["d"][0] == outs["f"][0]
    closing_line(outs["d"][1], st)
    assert "[seeksv] -D:" not in outs["f"][1].stderr and "[seeksv] -D:" not in outs["u"][1].stderr


def test_refusals(sample, tmp_path):
    d, fa, files, _ = sample
    bam = files["plain"]
    cases = [(["run", "-D", "-M", bam, fa], "seeksv run: -D", "-M"), (["run", "-D", "-N", "2", bam, fa], "seeksv run: -D", "-N"), (["run", "-D", "-P", bam, fa], "seeksv run: -D", "-P"),
             (["somatic", "-D", bam, "x.clip.gz", "t.sv"], "seeksv somatic: -D", "-K"),
             (["run", "-u", "-M", bam, fa], "seeksv run: -u does not carry the read names through the sort, which -M's digests need; -M is not supported with it", "-M"),
             (["run", "-M", files["sam"], fa], "seeksv run: -M reads a BAM; SAM text is not supported with it", "SAM")]
    for k, (args, start, word) in enumerate(cases):
        pre = str(tmp_path / f"refused{k}")
        r = subprocess.run([SEEKSV] + args + [pre], capture_output=True, text=True)
        lines = [l for l in r.stderr.splitlines() if not l.startswith("[stamp]")]
        assert r.returncode == 1 and len(lines) == 1 and lines[0].startswith(start) and word in lines[0], (args, r.stderr)
        assert not glob.glob(pre + "*")
    # getclip and getsv have no such option
    for cmd in ("getclip", "getsv"):
        r = subprocess.run([SEEKSV, cmd, "-D", bam], capture_output=True, text=True)
        assert r.returncode == 1 and f"Usage: seeksv {cmd}" in r.stderr
    # the first usage line of both commands stays as it was, and both usage texts name the option and its limits
    for cmd, first in (("run", "Usage: seeksv run [options] <input.sorted.bam> <reference fasta(.gz)> <output prefix>"), ("somatic", "Usage: seeksv somatic [options] <input normal original bam>")):
        r = subprocess.run([SEEKSV, cmd], capture_output=True, text=True)
        assert r.stderr.splitlines()[0].startswith(first) and "         -D  " in r.stderr and "         -M  " in r.stderr
    r = subprocess.run([SEEKSV, "run"], capture_output=True, text=True)
    assert "Libraries are not told apart" in r.stderr and "Not with -M, -P or -N above 1" in r.stderr


def test_run_M_and_run_u_on_the_same_files_are_what_they_were(sample, expected):
    """-M's rule finds none of the differently-clipped copies: `run -M` writes what `run` writes for the file with -M's flags (none new); `run -u` what `run`
    writes for the sorted records; neither prints -D's line"""
    d, fa, files, _ = sample
    pre = str(d / "got_M")
    r = run(["run", "-M"] + SV_OPTS + [files["plain"], fa, pre])
    want, want_stdout = expected("flagged_by_M")
    same_outputs(pre, want)
    assert r.stdout == want_stdout and "[seeksv] -D:" not in r.stderr and "[seeksv] -M: marked 0 + 0 duplicate records" in r.stderr
    same_outputs(pre, expected("plain")[0])
    pre = str(d / "got_u")
    r = run(["run", "-u"] + SV_OPTS + [files["shuffled"], fa, pre])
    want, want_stdout = expected("shuffled_sorted")
    same_outputs(pre, want, unmapped_in_order=False)
    assert r.stdout == want_stdout and "[seeksv] -D:" not in r.stderr
