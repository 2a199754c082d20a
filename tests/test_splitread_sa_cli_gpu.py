"""-m gpu, through the binary: `seeksv run -A -S`.  The sample is tests/splitread_sa_inputs.cli_sample: paired-end fragments whose supplementary records are
hard-clipped and whose primary records name them in their SA tags.  On the complete sample `run -A -S` writes byte for byte what `run -A` writes; with the
supplementary records removed the columns of the table that the pass decides are the model's (tests/splitread_sa_model.py, readthrough_model.apply +
row_columns) and the junctions are the complete sample's - as a BAM, as SAM text on a pipe with -u and -D, with -L; the two closing lines carry the model's
counts; `run -A` without -S prints nothing of the mode and launches none of its groups; the refusals leave no file."""
import glob
import os
import re
import subprocess

import pytest

import bamio
import readthrough_model as RM
import sam_text as ST
import splitread_inputs as SI
import splitread_sa_inputs as SAI
import splitread_sa_model as SAM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
LOOSE = "-f 0 -b 0 -T 100000 -m 0"      # getsv prints every junction


def run(args, env=None, stdin=None):
    r = subprocess.run([SEEKSV] + args, capture_output=True, env=dict(os.environ, **(env or {})), input=stdin)
    r.stdout, r.stderr = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0, (args, r.stderr[-1500:])
    return r


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("splitread_sa_cli")
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        f.write(SI.reference_fasta())
    complete, removed = SAI.cli_sample()
    records = {"complete": SI.coordinate_sorted(complete), "removed": SI.coordinate_sorted(removed)}
    records["shuffled"] = SI.shuffled(records["removed"])
    files = {}
    for tag, recs in records.items():
        files[tag] = str(d / f"{tag}.bam")
        bamio.write_bam(files[tag], SI.CONTIGS, SI.LENS, recs)
    return d, fa, files, records


@pytest.fixture(scope="module")
def plain(sample):
    """`seeksv run` without -A on the sample without its supplementary records: the junctions that no split-read pass made"""
    d, fa, files, _ = sample
    pre = str(d / "plain")
    return pre, run(["run", "-v", LOOSE, files["removed"], fa, pre])


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


def model_of(records, enc):
    b, names = SAI.batch_of(records)
    pairs, counts, sa = SAM.find_pairs([b], [names], [(enc, SAI.areas(records, enc))], 1, SI.CONTIGS)
    return RM.apply(pairs), counts, sa


def closing_lines(stderr, c, sa):
    lines = [l for l in stderr.splitlines() if l.startswith("[seeksv] -A:") or l.startswith("[seeksv] -S:")]
    want = [f"[seeksv] -A: {c['pairs']} pairs ({c['pairs_borrowed']} with a borrowed seq) of {c['candidates']} one-side-clipped records ({c['hard_clipped']} hard-clipped); "
            f"dropped at the pairing: {c['dropped_no_carrier']} without a record that carries the read, {c['dropped_length']} for unequal read lengths"]
    if sa is not None:
        want.append("[seeksv] -S: " + ", ".join(f"{k} {sa[k]}" for k in SAM.SA_COUNTS))
    assert lines == want, stderr[-1500:]


def hold_to_model(prefix, r, records, enc, without):
    """the junctions that the pass adds to what the run prints without it are the model's, column for column; every model junction is printed"""
    jmap, counts, sa = model_of(records, enc)
    rows = printed_rows(prefix, r.stdout)
    added = {k: v for k, v in rows.items() if k not in without}
    assert len(jmap) == counts["pairs"] == sa["pairs_from_sa"] > 30 and set(added) == set(jmap)
    for key, got in added.items():
        assert dict(got, key=key) == RM.row_columns(key, jmap[key]), key
    closing_lines(r.stderr, counts, sa)
    return rows


def test_supplementary_records_removed_gives_the_model_s_columns(sample, plain):
    d, fa, files, records = sample
    without = printed_rows(plain[0], plain[1].stdout)
    pre = str(d / "removed_AS")
    r = run(["run", "-A", "-S", "-v", LOOSE, files["removed"], fa, pre], {"SSV_TIMING": "1", "SSV_CHUNK_INFLATED_MB": "1"})
    hold_to_model(pre, r, records["removed"], SAI.BAM, without)
    m = re.search(r"\(-A -S kernel time: splitread_sa_aux ([0-9.e+-]+) ms in (\d+) launches, splitread_sa_scan ([0-9.e+-]+) ms in (\d+) launches, splitread_sa_finish ([0-9.e+-]+) ms in "
                  r"(\d+) launches; the scans held the pump for ([0-9.e+-]+) s; candidate store (\d+) bytes\)", r.stderr)
    assert m and int(m.group(2)) == int(m.group(4)) >= 1 and int(m.group(6)) == 1 and int(m.group(8)) > 0, r.stderr[-1500:]


def test_without_S_the_run_says_nothing_of_the_mode(sample, plain):
    """`run -A` on the same file: none of the junctions, no new line, no launch of the new groups"""
    d, fa, files, _ = sample
    a = str(d / "removed_A")
    ra = run(["run", "-A", "-v", LOOSE, files["removed"], fa, a], {"SSV_TIMING": "1"})
    assert printed_rows(a, ra.stdout) == printed_rows(plain[0], plain[1].stdout)
    assert "[seeksv] -S:" not in ra.stderr and "splitread_sa" not in ra.stderr and "-A kernel time: splitread_scan" in ra.stderr


def test_complete_sample_is_what_run_A_writes(sample, plain):
    """every primary has its supplementary: the same table and stdout byte for byte, every virtual candidate redundant - and these are the junctions that the
    sample without its supplementary records gives under -S (the model's, as the first test holds the binary to them)"""
    d, fa, files, records = sample
    c, cs = str(d / "complete_A"), str(d / "complete_AS")
    rc = run(["run", "-A", "-v", LOOSE, files["complete"], fa, c])
    rcs = run(["run", "-A", "-S", "-v", LOOSE, files["complete"], fa, cs])
    assert open(c + ".sv.txt", "rb").read() == open(cs + ".sv.txt", "rb").read() and rc.stdout == rcs.stdout
    jmap, counts, sa = model_of(records["complete"], SAI.BAM)
    closing_lines(rcs.stderr, counts, sa)
    closing_lines(rc.stderr, counts, None)
    assert sa["virtuals"] == sa["sa_redundant"] > 30 and sa["pairs_from_sa"] == 0
    removed_jmap = model_of(records["removed"], SAI.BAM)[0]
    rows = printed_rows(c, rc.stdout)
    assert set(removed_jmap) == set(jmap) <= set(rows)
    for key in removed_jmap:
        assert RM.row_columns(key, removed_jmap[key]) == RM.row_columns(key, jmap[key]) == dict(rows[key], key=key), key


def test_sam_text_on_a_pipe_with_u_and_D(sample, plain):
    """an aligner's output as it comes: SAM text on stdin, in any order; the pass runs in input order - the model over the shuffled records"""
    d, fa, files, records = sample
    data = ST.text(records["shuffled"], SI.CONTIGS, SI.LENS).encode("latin-1")
    pre = str(d / "removed_AS_pipe")
    r = run(["run", "-u", "-D", "-A", "-S", "-v", LOOSE, "-", fa, pre], {"SSV_SAM_CHUNK_KB": "4"}, stdin=data)
    hold_to_model(pre, r, records["shuffled"], SAI.SAM, printed_rows(plain[0], plain[1].stdout))
    assert len([l for l in r.stderr.splitlines() if l.startswith("[seeksv] -u: sorted ")]) == 1
    assert len([l for l in r.stderr.splitlines() if l.startswith("[seeksv] -D: marked ")]) == 1


def test_with_a_restriction(sample, tmp_path):
    """-L comes behind the pass: the counts are those of the whole input"""
    d, fa, files, records = sample
    bed = str(tmp_path / "keep.bed")
    with open(bed, "w") as f:
        f.write("chrB\t15000\t16000\n")
    r = run(["run", "-A", "-S", "-L", bed, "-v", LOOSE, files["removed"], fa, str(d / "removed_AS_L")])
    _, counts, sa = model_of(records["removed"], SAI.BAM)
    closing_lines(r.stderr, counts, sa)


def test_refusals_leave_no_file(sample, tmp_path):
    d, fa, files, _ = sample
    cases = [(["-S"], "without -A"), (["-A", "-S", "-c", "-S"], "inside"), (["-A", "-S", "-v", "-S"], "inside"), (["-A", "-S", "-a", "-S 8"], "inside")]
    for k, (opts, word) in enumerate(cases):
        pre = str(tmp_path / f"refused{k}")
        r = subprocess.run([SEEKSV, "run"] + opts + [files["removed"], fa, pre], capture_output=True, text=True)
        lines = [l for l in r.stderr.splitlines() if not l.startswith("[stamp]")]
        assert r.returncode == 1 and len(lines) == 1 and lines[0].startswith("seeksv run: -S") and word in lines[0], (opts, r.stderr)
        assert not glob.glob(pre + "*")
