"""-m gpu, through the binary: `seeksv run -u` on a file in any order writes what `seeksv run` writes on the same records stably sorted by the rule
(tests/coordsort_model.py: the expected file of an order is the model's sort OF THAT ORDER) - every file byte for byte and stdout, except
prefix.unmapped_[12].fq.gz, which hold the same pairs in input order.  Orders: a seeded random permutation and read-name order, as BAM; read-name order also as
SAM text, plain and gzip.  One chunk, and chunks of 1 MB with output batches of 5000 records (seven and more batches in, eight and more out, counted; a cut
inside the 11,000-record pile).  The shortcut for sorted input, the refusals.  Sample: tests/coordsort_inputs.py (cli_sample), held to its properties on the
CPU in tests/test_coordsort_inputs.py."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
SV_OPTS = ["-v", "-b 3"]
NAMES, LENS = list(CI.NAMES), list(CI.LENS)
ORDERS = {"shuffled": ci.shuffled, "name": ci.by_name}
CHUNKED = {"SSV_CHUNK_INFLATED_MB": "1", "SSV_SORT_BATCH_RECORDS": "5000", "SSV_SAM_CHUNK_KB": "1024"}


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("coordsort_cli")
    contigs, recs = ci.cli_sample()
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for name, c in zip(NAMES, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 70] for i in range(0, len(c), 70)) + "\n")
    files = {}
    for tag, make in ORDERS.items():
        order = make(recs)
        want = [order[i] for i in cm.order(order, len(NAMES))]
        files[tag] = (str(d / f"{tag}.bam"), str(d / f"{tag}.expected.bam"))
        bamio.write_bam(files[tag][0], NAMES, LENS, order)
        bamio.write_bam(files[tag][1], NAMES, LENS, want)
        files[tag + "_records"] = want
    text = ci.sam_header(NAMES, LENS).encode() + mi.sam_text(ORDERS["name"](recs), NAMES)
    files["plain"], files["gzip"] = str(d / "name.sam"), str(d / "name.sam.gz")
    with open(files["plain"], "wb") as f:
        f.write(text)
    with gzip.open(files["gzip"], "wb", compresslevel=1) as f:
        f.write(text)
    return d, fa, files


def run(args, env=None, ok=True):
    r = subprocess.run([SEEKSV] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, (args, r.stderr[-800:])
    return r


def fastq_pairs(prefix):
    """prefix.unmapped_1.fq.gz and _2 as a multiset of (read 1's record, read 2's record)"""
    def records(path):
        lines = gzip.open(path, "rt").read().splitlines()
        assert len(lines) % 4 == 0
        return [tuple(lines[k:k + 4]) for k in range(0, len(lines), 4)]
    one, two = records(prefix + ".unmapped_1.fq.gz"), records(prefix + ".unmapped_2.fq.gz")
    assert len(one) == len(two)
    return collections.Counter(zip(one, two))


def same_outputs(a, b, unmapped_in_order):
    """test_markdup_cli_gpu.same_outputs, but for the two unmapped files when the inputs' orders differ: the same pairs, as multisets"""
    for ext in (".clip.gz", ".clip.fq.gz") + ((".unmapped_1.fq.gz", ".unmapped_2.fq.gz") if unmapped_in_order else ()):
        assert gzip.open(a + ext, "rb").read() == gzip.open(b + ext, "rb").read(), ext
    for ext in (".sv.txt", ".unmapped.clip.fq"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert bamio.read_bam_records(a + ".clip.bam") == bamio.read_bam_records(b + ".clip.bam")
    assert sorted(os.path.basename(x)[len(os.path.basename(a)):] for x in glob.glob(a + ".*")) == sorted(os.path.basename(x)[len(os.path.basename(b)):] for x in glob.glob(b + ".*"))
    pa, pb = fastq_pairs(a), fastq_pairs(b)
    assert pa == pb and sum(pa.values()) == ci.N_HALF_MAPPED        # every pair with one unmapped end, once: the comparison is not one of empty files


def closing_line(r):
    lines = [l for l in r.stderr.splitlines() if l.startswith("[seeksv] -u:")]
    assert len(lines) == 1, r.stderr[-800:]
    return lines[0]


def sorted_counts(r):
    m = re.fullmatch(r"\[seeksv\] -u: sorted (\d+) records from (\d+) into (\d+) batches", closing_line(r))
    assert m, closing_line(r)
    return tuple(int(x) for x in m.groups())


@pytest.fixture(scope="module")
def expected(sample):
    """`seeksv run` on the expected file of each order, once per way of reading it: (prefix, stdout)"""
    d, fa, files = sample
    made = {}

    def get(tag, chunked):
        if (tag, chunked) not in made:
            pre = str(d / f"want_{tag}_{'c' if chunked else 'w'}")
            r = run(["run"] + SV_OPTS + [files[tag][1], fa, pre], CHUNKED if chunked else None)
            assert "[seeksv] -u:" not in r.stderr
            made[(tag, chunked)] = (pre, r.stdout)
        return made[(tag, chunked)]
    return get


@pytest.mark.parametrize("chunked", [False, True], ids=["one-chunk", "chunks-of-1MB"])
@pytest.mark.parametrize("tag", list(ORDERS))
def test_run_u_equals_run_on_the_sorted_file(sample, expected, tag, chunked):
    d, fa, files = sample
    pre = str(d / f"got_{tag}_{'c' if chunked else 'w'}")
    r = run(["run", "-u"] + SV_OPTS + [files[tag][0], fa, pre], CHUNKED if chunked else None)
    want, want_stdout = expected(tag, chunked)
    same_outputs(pre, want, unmapped_in_order=False)
    assert r.stdout == want_stdout
    table = open(pre + ".sv.txt").read()                                          # (the comparison is not one of empty tables: both planted junctions are there)
    assert CI.names_both_ends(table, CI.JUNCTION_A) and CI.names_both_ends(table, CI.JUNCTION_B)
    n, n_in, n_out = sorted_counts(r)
    recs = files[tag + "_records"]
    assert n == len(recs)
    if chunked:
        assert n_in >= 7 and n_out == (n + 4999) // 5000 >= 8
        pile = [i for i, x in enumerate(recs) if x["qname"].startswith("pile")]
        assert pile == list(range(pile[0], pile[0] + CI.PILE)) and any(pile[0] < c < pile[-1] for c in range(5000, n, 5000))      # a cut inside the pile
    else:
        assert n_in == 1 and n_out == 1


@pytest.mark.parametrize("form", ["plain", "gzip"])
def test_run_u_on_sam_text_in_read_name_order(sample, expected, form):
    d, fa, files = sample
    chunked = form == "gzip"
    pre = str(d / f"got_text_{form}")
    r = run(["run", "-u"] + SV_OPTS + [files[form], fa, pre], CHUNKED if chunked else None)
    want, want_stdout = expected("name", chunked)
    same_outputs(pre, want, unmapped_in_order=False)
    assert r.stdout == want_stdout
    n, n_in, n_out = sorted_counts(r)
    assert n == len(files["name_records"]) and (n_in >= 7 and n_out >= 8 if chunked else n_in == n_out == 1)


def test_sorted_input_takes_the_shortcut(sample, expected):
    d, fa, files = sample
    pre = str(d / "got_sorted")
    r = run(["run", "-u"] + SV_OPTS + [files["name"][1], fa, pre], dict(CHUNKED, SSV_TIMING="1"))
    want, want_stdout = expected("name", True)
    same_outputs(pre, want, unmapped_in_order=True)
    assert r.stdout == want_stdout
    line = closing_line(r)
    assert line.endswith("already in coordinate order") and f" {len(files['name_records'])} records " in line
    m = re.search(r"\(-u kernel time: sort_keys ([0-9.e+-]+) ms in (\d+) launches, sort_radix ([0-9.e+-]+) ms in (\d+) launches, sort_gather ([0-9.e+-]+) ms in (\d+) launches; "
                  r"resident at the peak: (\d+) \+ (\d+) bytes of records, (\d+) bytes of keys and indices\)", r.stderr)
    assert m and int(m.group(2)) > 0 and int(m.group(4)) == 0 and int(m.group(6)) == 0          # the check and the change lists; no sort, no gather
    assert int(m.group(7)) > 80 * 40000 and int(m.group(8)) == 0 and int(m.group(9)) == 0          # nothing copied


def test_more_contig_changes_than_a_sorted_file_can_have(sample, tmp_path):
    """SAM text whose contig changes 66,000 times in one chunk: `run` refuses it as not coordinate sorted, as it always did; `run -u` takes it.  (The sample
    above has 40,072 records: no order of it reaches the decoder's 65,536 changes, and `run` without -u goes through it pass by pass as the reference would.)"""
    d, fa, files = sample
    n = 66000
    recs = [dict(qname=f"r{k}", flag=0, tid=k % 2, pos=100 + k % 50000, mapq=60, cigar="10M", mtid=-1, mpos=-1, isize=0, seq="ACGTACGTAC", qual=bytes([30] * 10)) for k in range(n)]
    sam = str(tmp_path / "alternating.sam")
    with open(sam, "wb") as f:
        f.write(ci.sam_header(NAMES, LENS).encode() + mi.sam_text(recs, NAMES))
    pre = str(tmp_path / "refused")
    r = run(["run"] + SV_OPTS + [sam, fa, pre], ok=False)
    assert r.returncode == 1 and "not coordinate sorted" in r.stderr
    pre = str(tmp_path / "taken")
    r = run(["run", "-u"] + SV_OPTS + [sam, fa, pre])
    assert sorted_counts(r) == (n, 1, 1) and os.path.exists(pre + ".sv.txt")


def test_refusals(sample, tmp_path):
    d, fa, files = sample
    bam = files["shuffled"][0]
    cases = [(["run", "-u", "-N", "2", bam, fa], "-N"), (["run", "-u", "-P", bam, fa], "-P"), (["run", "-u", "-M", bam, fa], "-M"),
             (["run", "-c", "-u", bam, fa], "-c"), (["run", "-u", "-v", "-b 3 -u", bam, fa], "-v")]
    for k, (args, word) in enumerate(cases):
        pre = str(tmp_path / f"refused{k}")
        r = subprocess.run([SEEKSV] + args + [pre], capture_output=True, text=True)
        lines = [l for l in r.stderr.splitlines() if not l.startswith("[stamp]")]
        assert r.returncode == 1 and len(lines) == 1 and lines[0].startswith("seeksv run: -u") and word in lines[0], (args, r.stderr)
        assert not glob.glob(pre + "*")
    # getclip, getsv and somatic have no such option
    for cmd in ("getclip", "getsv", "somatic"):
        r = subprocess.run([SEEKSV, cmd, "-u", bam], capture_output=True, text=True)
        assert r.returncode == 1 and f"Usage: seeksv {cmd}" in r.stderr
    # the first usage line stays as it was, and the usage text names the option and what it does not promise
    r = subprocess.run([SEEKSV, "run"], capture_output=True, text=True)
    assert r.stderr.splitlines()[0].startswith("Usage: seeksv run [options] <input.sorted.bam> <reference fasta(.gz)> <output prefix>")
    assert "         -u  " in r.stderr and "unmapped_[12].fq.gz, which hold the same pairs in input order" in r.stderr
