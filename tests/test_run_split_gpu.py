"""-m gpu: `seeksv run -P` - the unmapped pairs split-aligned inside `run`, their records built on the device and handed to the -F pass there (DESIGN.md
10g) - against the goldens the real reference's getsv printed (tests/golden/realign_split) and against the chain of the separate commands: getclip,
realign, `realign -P` on the two concatenated unmapped-pair files, `getsv -F`.  Inputs: tests/realign_split_inputs.e2e_sample() and
tests/run_split_inputs.e2e_variant(), held to their properties on the CPU in tests/test_run_split_inputs.py."""
import glob
import gzip
import os
import subprocess

import pytest

import bamio
import golden_util as G
import realign_split_inputs as SI
import run_split_inputs as RI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")


def write_sample(d, sample):
    contigs, recs = sample
    bam, fa = str(d / "s.bam"), str(d / "ref.fa")
    bamio.write_bam(bam, list(SI.E2E_NAMES), list(SI.E2E_LENS), recs)
    with open(fa, "w") as f:
        for name, c in zip(SI.E2E_NAMES, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 70] for i in range(0, len(c), 70)) + "\n")
    return bam, fa


def run(args, env=None):
    r = subprocess.run([SEEKSV] + args, capture_output=True, text=True, env=env)
    assert r.returncode == 0, (args, r.stderr[-800:])
    return r


def summaries(r):
    return [l for l in r.stderr.splitlines() if l.startswith("[seeksv realign]")]


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp("run_split_e2e")
    return d, write_sample(d, SI.e2e_sample())


def test_run_P_prints_the_reference_table_from_one_command(e2e):
    """no read is soft-clipped at the planted junction: `run` prints the table without it, `run -P` the one the real reference's getsv printed with -F; the
    leg's closing line counts the ten split reads; no prefix.F.bam appears"""
    d, (bam, fa) = e2e
    pre = str(d / "p")
    r = run(["run", "-P", bam, fa, pre])
    assert open(pre + ".sv.txt").read() == G.read_text("realign_split", "e2e.F.sv")
    assert r.stdout == G.read_text("realign_split", "e2e.F.stdout")
    assert SI.e2e_names_both_ends(open(pre + ".sv.txt").read()) or SI.e2e_names_both_ends(r.stdout)
    last = summaries(r)
    assert len(last) == 2 and last[1].startswith("[seeksv realign] 20 clipped sequences, 20 aligned") and last[1].endswith(f", {SI.E2E_READS} split reads (mate pieces written)")
    assert "split" not in last[0] and r.stderr.count("'FindJunction' finished") == 1
    assert not glob.glob(pre + "*.F.bam") and not glob.glob(str(d / "*.F.bam*"))
    assert sorted(os.path.basename(x) for x in glob.glob(pre + ".*")) == ["p.clip.bam", "p.clip.fq.gz", "p.clip.gz", "p.sv.txt", "p.unmapped.clip.fq", "p.unmapped_1.fq.gz", "p.unmapped_2.fq.gz"]


def test_run_without_P_and_with_a_floor_above_every_mapq(e2e):
    d, (bam, fa) = e2e
    pre = str(d / "q")
    r = run(["run", bam, fa, pre])
    assert open(pre + ".sv.txt").read() == G.read_text("realign_split", "e2e.sv") and r.stdout == G.read_text("realign_split", "e2e.stdout")
    assert len(summaries(r)) == 1 and "FindJunction" not in r.stderr
    pre = str(d / "w")
    r = run(["run", "-P", "-v", "-w 61", bam, fa, pre])
    assert open(pre + ".sv.txt").read() == G.read_text("realign_split", "e2e.sv") and r.stdout == G.read_text("realign_split", "e2e.stdout")
    assert summaries(r)[1].endswith(f", {SI.E2E_READS} split reads (mate pieces written)")


def test_refusals_come_before_any_file(e2e):
    d, (bam, fa) = e2e
    for k, (extra, word) in enumerate(((["-v", "-F other.bam"], "-F"), (["-v", "-b 2 -Fother.bam"], "-F"), (["-c", "-N 2"], "-N"), (["-c", "-q 5 -N2"], "-N"))):
        pre = str(d / f"refused{k}")
        r = subprocess.run([SEEKSV, "run", "-P"] + extra + [bam, fa, pre], capture_output=True, text=True)
        assert r.returncode == 1 and not glob.glob(pre + "*"), (extra, r.stderr)
        lines = [l for l in r.stderr.splitlines() if not l.startswith("[stamp]")]
        assert len(lines) == 1 and word in lines[0] and "-P" in lines[0], r.stderr
    # -P stays no option of the aligner step
    r = subprocess.run([SEEKSV, "run", "-a", "-P", bam, fa, str(d / "refused_a")], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Usage: seeksv realign") and not glob.glob(str(d / "refused_a*"))


def chain(d, tag, bam, fa, aln):
    """the separate commands -> (prefix, getsv's run)"""
    a = str(d / f"chain_{tag}")
    run(["getclip", "-o", a, bam])
    run(["realign"] + aln + [fa, a + ".clip.fq.gz", a + ".clip.bam"])
    with open(a + ".u12.fq.gz", "wb") as f:
        f.write(open(a + ".unmapped_1.fq.gz", "rb").read() + open(a + ".unmapped_2.fq.gz", "rb").read())
    r = run(["realign", "-P"] + aln + [fa, a + ".u12.fq.gz", a + ".F.bam"])
    return a, run(["getsv", "-F", a + ".F.bam", a + ".clip.bam", bam, a + ".clip.gz", a + ".sv.txt", a + ".unmapped.clip.fq"]), summaries(r)[0]


@pytest.mark.parametrize("aln", [[], ["-c", str(SI.CAP)]], ids=["hash", "sorted"])
def test_run_P_equals_the_chain_of_commands(tmp_path, aln):
    """junction reads in both unmapped-pair files: every file and stdout of `run -P` equals the chain's, on either index, in one piece and in pieces of three
    reads (a read's two records never straddle one)"""
    bam, fa = write_sample(tmp_path, RI.e2e_variant())
    a, r3, closing = chain(tmp_path, "v", bam, fa, aln)
    assert SI.e2e_names_both_ends(open(a + ".sv.txt").read()) or SI.e2e_names_both_ends(r3.stdout)
    u1, u2 = gzip.open(a + ".unmapped_1.fq.gz", "rt").read(), gzip.open(a + ".unmapped_2.fq.gz", "rt").read()
    assert "@jn1/1\n" in u1 and "@jn2/2\n" in u2 and u1.count("\n") == u2.count("\n") == 4 * SI.E2E_READS
    opts = ["-a", " ".join(aln)] if aln else []
    for tag, env in (("one", None), ("pieces", dict(os.environ, SSV_REALIGN_SPLIT_PIECE="3"))):
        b = str(tmp_path / f"run_{tag}")
        r = run(["run", "-P"] + opts + [bam, fa, b], env=env)
        for ext in (".clip.gz", ".clip.fq.gz", ".unmapped_1.fq.gz", ".unmapped_2.fq.gz"):
            assert gzip.open(a + ext, "rb").read() == gzip.open(b + ext, "rb").read(), (tag, ext)
        for ext in (".sv.txt", ".unmapped.clip.fq"):
            assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), (tag, ext)
        assert bamio.read_bam_records(a + ".clip.bam") == bamio.read_bam_records(b + ".clip.bam"), tag
        assert r.stdout == r3.stdout, tag
        assert summaries(r)[1] == closing, tag
        assert not os.path.exists(b + ".F.bam")
