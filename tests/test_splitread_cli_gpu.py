"""-m gpu, through the binary: `seeksv run -A`.  On the agreement set (where the split-read rule and FindJunction say the same) written as a coordinate-sorted
BAM among filler records, `run -A in.bam` writes byte for byte the table and stdout of `run -v "-F in.bam" in.bam`.  On the hard-clipped paired-end sample
(tests/splitread_inputs.cli_sample) the columns of the table that the pass decides are the model's (tests/splitread_model.py, readthrough_model.apply +
row_columns) - as a BAM, as SAM text, with -u on a shuffled copy and with -D -, the closing line carries the model's counts, and everything getclip and the
aligner step write is what `run` writes without -A.  `run` without -A prints nothing of the stage; the refusals leave no file."""
import glob
import gzip
import os
import re
import subprocess

import pytest

import bamio
import readthrough_model as RM
import sam_text as ST
import splitread_inputs as SI
import splitread_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
LOOSE = "-f 0 -b 0 -T 100000 -m 0"      # getsv prints every junction
FLANK = 50                                # getsv -l, MergeJunction's search length


def run(args, env=None):
    r = subprocess.run([SEEKSV] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (args, r.stderr[-1200:])
    return r


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("splitread_cli")
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        f.write(SI.reference_fasta())
    records = {"agree": SI.coordinate_sorted(SI.agreement(0)["records"] + SI.filler(200)), "hard": SI.coordinate_sorted(SI.cli_sample())}
    records["shuffled"] = SI.shuffled(records["hard"])
    files = {}
    for tag, recs in records.items():
        files[tag] = str(d / f"{tag}.bam")
        bamio.write_bam(files[tag], SI.CONTIGS, SI.LENS, recs)
    files["sam"] = str(d / "hard.sam")
    ST.write(files["sam"], records["hard"], SI.CONTIGS, SI.LENS)
    return d, fa, files, records


@pytest.fixture(scope="module")
def plain(sample):
    """`seeksv run` without -A on the hard-clipped sample, recorded once: (prefix, the process)"""
    d, fa, files, _ = sample
    pre = str(d / "plain")
    return pre, run(["run", "-v", LOOSE, files["hard"], fa, pre], {"SSV_TIMING": "1"})


def printed_rows(prefix, stdout):
    """every junction of a run, from the table and from stdout's filtered rows: key -> the columns the -F pass decides"""
    rows = {}
    for line in open(prefix + ".sv.txt").read().splitlines():
        if line.startswith("@"):
            continue
        f = line.split("\t")
        assert len(f) == 23, line
        rows[(f[0], int(f[1]), f[2], f[4], int(f[5]), f[6])] = dict(left_support=int(f[3]), right_support=int(f[7]), microhomology=int(f[8]), left_cigar=f[19], right_cigar=f[20],
                                                                   left_seq=f[21], right_seq=f[22])
    for line in stdout.splitlines():
        f = line.split("\t")
        assert len(f) == 20, line
        f = f[1:]
        rows[(f[0], int(f[1]), f[2], f[4], int(f[5]), f[6])] = dict(left_support=int(f[3]), right_support=int(f[7]), microhomology=int(f[8]), left_cigar=f[15], right_cigar=f[16],
                                                                   left_seq=f[17], right_seq=f[18])
    return rows


def model_of(records, min_mapq=1):
    b, names = SI.batch_of(records)
    pairs, counts = SM.find_pairs([b], [names], min_mapq, SI.CONTIGS)
    return RM.apply(pairs), counts


def closing_line(stderr, c):
    lines = [l for l in stderr.splitlines() if l.startswith("[seeksv] -A:")]
    assert lines == [f"[seeksv] -A: {c['pairs']} pairs ({c['pairs_borrowed']} with a borrowed seq) of {c['candidates']} one-side-clipped records ({c['hard_clipped']} hard-clipped); "
                     f"dropped at the pairing: {c['dropped_no_carrier']} without a record that carries the read, {c['dropped_length']} for unequal read lengths"], stderr[-1200:]


def hold_to_model(prefix, r, records, without):
    """the junctions that -A adds to what the run prints without it are the model's, column for column; every model junction is printed"""
    jmap, counts = model_of(records)
    rows = printed_rows(prefix, r.stdout)
    added = {k: v for k, v in rows.items() if k not in without}
    assert len(jmap) == counts["pairs"] > 30 and set(added) == set(jmap)          # (cli_sample: every junction alone within FLANK, none merged away)
    for key, got in added.items():
        assert dict(got, key=key) == RM.row_columns(key, jmap[key]), key
    closing_line(r.stderr, counts)
    return rows


def same_getclip_and_aligner_files(a, b, unmapped_in_order=True):
    for ext in (".clip.gz", ".clip.fq.gz") + ((".unmapped_1.fq.gz", ".unmapped_2.fq.gz") if unmapped_in_order else ()):
        assert gzip.open(a + ext, "rb").read() == gzip.open(b + ext, "rb").read(), ext
    assert open(a + ".unmapped.clip.fq", "rb").read() == open(b + ".unmapped.clip.fq", "rb").read()
    assert bamio.read_bam_records(a + ".clip.bam") == bamio.read_bam_records(b + ".clip.bam")
    assert sorted(x[len(a):] for x in glob.glob(a + ".*")) == sorted(x[len(b):] for x in glob.glob(b + ".*"))


def test_run_A_equals_run_F_on_the_agreement_set(sample):
    d, fa, files, records = sample
    a, f = str(d / "agree_A"), str(d / "agree_F")
    ra = run(["run", "-A", "-v", LOOSE, files["agree"], fa, a])
    rf = run(["run", "-v", f"-F {files['agree']} {LOOSE}", files["agree"], fa, f])
    assert open(a + ".sv.txt", "rb").read() == open(f + ".sv.txt", "rb").read()
    assert ra.stdout == rf.stdout
    same_getclip_and_aligner_files(a, f)
    jmap, counts = model_of(records["agree"])
    assert counts["pairs"] >= 20 and len(printed_rows(a, ra.stdout)) >= 10
    closing_line(ra.stderr, counts)
    assert "'FindJunction' finished" in rf.stderr and "[seeksv] -A:" not in rf.stderr
    # -w of -v is the floor of both
    a0, f0 = str(d / "agree_A_w31"), str(d / "agree_F_w31")
    ra = run(["run", "-A", "-v", LOOSE + " -w 31", files["agree"], fa, a0])
    rf = run(["run", "-v", f"-F {files['agree']} -w 31 {LOOSE}", files["agree"], fa, f0])
    assert open(a0 + ".sv.txt", "rb").read() == open(f0 + ".sv.txt", "rb").read() and ra.stdout == rf.stdout
    closing_line(ra.stderr, model_of(records["agree"], 31)[1])
    assert open(a0 + ".sv.txt", "rb").read() != open(a + ".sv.txt", "rb").read()


def test_run_A_on_the_hard_clipped_sample_gives_the_model_s_columns(sample, plain):
    d, fa, files, records = sample
    without = printed_rows(plain[0], plain[1].stdout)
    pre = str(d / "hard_A")
    r = run(["run", "-A", "-v", LOOSE, files["hard"], fa, pre], {"SSV_TIMING": "1", "SSV_CHUNK_INFLATED_MB": "1"})
    hold_to_model(pre, r, records["hard"], without)
    same_getclip_and_aligner_files(pre, plain[0])
    m = re.search(r"\(-A kernel time: splitread_scan ([0-9.e+-]+) ms in (\d+) launches, splitread_finish ([0-9.e+-]+) ms in (\d+) launches; the scans held the pump for ([0-9.e+-]+) s; "
                  r"candidate store (\d+) bytes\)", r.stderr)
    assert m and int(m.group(2)) >= 1 and int(m.group(4)) == 1 and int(m.group(6)) > 0, r.stderr[-1500:]
    assert "splitread (run -A: the original's own supplementary alignments)" in r.stderr
    # what `-F` makes of the same file is something else: H is refused there and mates meet
    f = str(d / "hard_F")
    rf = run(["run", "-v", f"-F {files['hard']} {LOOSE}", files["hard"], fa, f])
    assert open(f + ".sv.txt").read() != open(pre + ".sv.txt").read()


def test_run_A_on_sam_text(sample, plain):
    d, fa, files, records = sample
    pre = str(d / "hard_A_sam")
    r = run(["run", "-A", "-v", LOOSE, files["sam"], fa, pre], {"SSV_SAM_CHUNK_KB": "4"})
    hold_to_model(pre, r, records["hard"], printed_rows(plain[0], plain[1].stdout))


def test_run_A_with_u_on_a_shuffled_copy(sample, plain):
    """the pass runs in input order: the model over the shuffled records"""
    d, fa, files, records = sample
    pre = str(d / "hard_A_u")
    r = run(["run", "-A", "-u", "-v", LOOSE, files["shuffled"], fa, pre])
    hold_to_model(pre, r, records["shuffled"], printed_rows(plain[0], plain[1].stdout))
    assert len([l for l in r.stderr.splitlines() if l.startswith("[seeksv] -u: sorted ")]) == 1


def test_run_A_with_D_and_with_a_restriction(sample, plain, tmp_path):
    """the pass reads the input's flags and every record: -D's marks and -L's restriction come behind it"""
    d, fa, files, records = sample
    pre = str(d / "hard_A_D")
    r = run(["run", "-A", "-D", "-v", LOOSE, files["hard"], fa, pre])
    hold_to_model(pre, r, records["hard"], printed_rows(plain[0], plain[1].stdout))
    assert len([l for l in r.stderr.splitlines() if l.startswith("[seeksv] -D: marked ")]) == 1
    bed = str(tmp_path / "keep.bed")
    with open(bed, "w") as f:
        f.write("chrB\t15000\t16000\n")                                      # none of the split reads lies here
    pre = str(d / "hard_A_L")
    r = run(["run", "-A", "-L", bed, "-v", LOOSE, files["hard"], fa, pre])
    _, counts = model_of(records["hard"])
    closing_line(r.stderr, counts)


def test_run_without_A_is_unchanged(sample, plain):
    d, fa, files, _ = sample
    pre, r = plain
    for words in ("[seeksv] -A:", "-A kernel time", "splitread"):
        assert words not in r.stderr, words
    again = str(d / "plain_again")
    r2 = run(["run", "-v", LOOSE, files["hard"], fa, again], {"SSV_TIMING": "1"})
    assert open(again + ".sv.txt", "rb").read() == open(pre + ".sv.txt", "rb").read() and r2.stdout == r.stdout
    same_getclip_and_aligner_files(again, pre)
    lines = lambda text: sorted(l for l in text.splitlines() if not l.startswith("[stamp]") and not l.startswith("[timing]"))  # noqa: E731
    timed = lambda text: sorted(re.sub(r"[0-9.e+-]+", "N", l) for l in text.splitlines() if l.startswith("[timing]"))          # noqa: E731
    assert lines(r2.stderr) == lines(r.stderr) and timed(r2.stderr) == timed(r.stderr)


def test_refusals_leave_no_file(sample, tmp_path):
    d, fa, files, _ = sample
    cases = [(["-A", "-P"], "-P"), (["-A", "-v", f"-F {files['agree']}"], "-F"), (["-A", "-N", "2"], "-N"), (["-c", "-A"], "inside"), (["-v", "-A"], "inside"), (["-a", "-A"], "inside")]
    for k, (opts, word) in enumerate(cases):
        pre = str(tmp_path / f"refused{k}")
        r = subprocess.run([SEEKSV, "run"] + opts + [files["hard"], fa, pre], capture_output=True, text=True)
        lines = [l for l in r.stderr.splitlines() if not l.startswith("[stamp]")]
        assert r.returncode == 1 and len(lines) == 1 and lines[0].startswith("seeksv run: -A") and word in lines[0], (opts, r.stderr)
        assert not glob.glob(pre + "*")
