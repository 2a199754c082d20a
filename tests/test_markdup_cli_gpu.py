"""-m gpu, through the binary: `seeksv run -M` and `seeksv somatic -K -M` on a BAM whose duplicates are not marked write what the same commands without -M
write on the same BAM with the model's flags set (tests/markdup_model.py) - every file, byte for byte - also when the BAM comes in chunks of 1 MB (seven and more, counted) - and what
the real reference wrote for that flagged BAM (tests/golden/markdup); the planted junction that only the copies carry leaves the table; the closing line on
stderr; the refusals.  Sample: tests/markdup_cli_inputs.py, held to its properties on the CPU in tests/test_markdup_cli_inputs.py."""
import glob
import gzip
import os
import subprocess

import pytest

import bamio
import golden_util as G
import markdup_cli_inputs as CI
import markdup_model as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
SV_OPTS = ["-v", "-b 3"]


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("markdup_cli")
    contigs, recs = CI.sample()
    plain, marked, fa = str(d / "plain.bam"), str(d / "marked.bam"), str(d / "ref.fa")
    bamio.write_bam(plain, list(CI.NAMES), list(CI.LENS), recs)
    bamio.write_bam(marked, list(CI.NAMES), list(CI.LENS), CI.flagged(recs))
    with open(fa, "w") as f:
        for name, c in zip(CI.NAMES, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 70] for i in range(0, len(c), 70)) + "\n")
    return d, plain, marked, fa


def run(args, env=None):
    r = subprocess.run([SEEKSV] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (args, r.stderr[-800:])
    return r


def same_outputs(a, b):
    for ext in (".clip.gz", ".clip.fq.gz", ".unmapped_1.fq.gz", ".unmapped_2.fq.gz"):
        assert gzip.open(a + ext, "rb").read() == gzip.open(b + ext, "rb").read(), ext
    for ext in (".sv.txt", ".unmapped.clip.fq"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert bamio.read_bam_records(a + ".clip.bam") == bamio.read_bam_records(b + ".clip.bam")
    assert sorted(os.path.basename(x)[len(os.path.basename(a)):] for x in glob.glob(a + ".*")) == sorted(os.path.basename(x)[len(os.path.basename(b)):] for x in glob.glob(b + ".*"))


def closing_line(r):
    lines = [l for l in r.stderr.splitlines() if l.startswith("[seeksv] -M:")]
    assert len(lines) == 1
    return lines[0]


def chunks_decoded(r):
    return sum(1 for l in r.stderr.splitlines() if l.startswith("[timing] (chunk of ") and " 0 blocks" not in l)


@pytest.mark.parametrize("env", [{"SSV_TIMING": "2"}, {"SSV_TIMING": "2", "SSV_CHUNK_INFLATED_MB": "1"}], ids=["one-chunk", "chunks-of-1MB"])
def test_run_M_equals_run_on_the_flagged_bam(sample, env):
    d, plain, marked, fa = sample
    tag = "c" if "SSV_CHUNK_INFLATED_MB" in env else "w"
    m, f, u = str(d / f"m{tag}"), str(d / f"f{tag}"), str(d / f"u{tag}")
    rm = run(["run", "-M"] + SV_OPTS + [plain, fa, m], env)
    rf = run(["run"] + SV_OPTS + [marked, fa, f], env)
    same_outputs(m, f)
    assert rm.stdout == rf.stdout
    # the seams of tests/markdup_cli_inputs.py exist only when the file really comes in chunks of 1 MB: inside junction A's run, right behind the contig
    # change, and round a batch that is one run from end to end
    want_chunks = CI.batch_of(CI.record_ends(CI.sample()[1]))[-1] + 1
    assert chunks_decoded(rm) == chunks_decoded(rf) == (want_chunks if tag == "c" else 1) and want_chunks >= 7
    st = {}
    mm.mark(list(CI.sample()[1]), stats=st)
    assert st["heads_marked"] == st["tails_marked"] == 2 * CI.COPIES
    assert closing_line(rm) == f"[seeksv] -M: marked {st['heads_marked']} + {st['tails_marked']} duplicate records ({st['groups']} groups) of {st['records']}"
    assert "[seeksv] -M:" not in rf.stderr
    # marking changes what the passes see: without it the copies count
    ru = run(["run"] + SV_OPTS + [plain, fa, u], env)
    assert gzip.open(u + ".clip.gz", "rb").read() != gzip.open(m + ".clip.gz", "rb").read()
    # ... and both are what the real reference's getclip and getsv wrote for the flagged and for the unflagged BAM (tests/golden/make_markdup_reference.py)
    for pre, r, tag in ((m, rm, "marked"), (u, ru, "plain")):
        assert open(pre + ".sv.txt").read() == G.read_text("markdup", tag + ".sv"), tag
        assert r.stdout == G.read_text("markdup", tag + ".stdout"), tag
        assert gzip.open(pre + ".clip.gz", "rt").read() == G.read_text("markdup", tag + ".clip.txt"), tag
    # junction A: in the table while its copies count, gone once they are marked (two reads stay, below -b 3); junction B stays
    with_m, without = open(m + ".sv.txt").read(), open(u + ".sv.txt").read()
    assert CI.names_both_ends(without, CI.JUNCTION_A) and CI.names_both_ends(without, CI.JUNCTION_B)
    assert not CI.names_both_ends(with_m, CI.JUNCTION_A) and CI.names_both_ends(with_m, CI.JUNCTION_B)
    # -M on a BAM that is marked already changes nothing
    m2 = str(d / f"m2{tag}")
    run(["run", "-M"] + SV_OPTS + [marked, fa, m2], env)
    same_outputs(m2, f)


def test_somatic_K_M_equals_somatic_K_on_the_flagged_normal(sample, tmp_path):
    d, plain, marked, fa = sample
    pre = str(tmp_path / "t")
    run(["run"] + SV_OPTS + [plain, fa, pre])
    tumor = pre + ".sv.txt"
    outs = {}
    for tag, args in (("m", ["-M", plain]), ("f", [marked]), ("u", [plain])):
        out = str(tmp_path / f"{tag}.somatic.sv")
        r = run(["somatic", "-K"] + args + [tumor, out])
        outs[tag] = (open(out).read(), r.stderr)
    assert outs["m"][0] == outs["f"][0]
    assert "[seeksv] -M: marked 6 + 6 duplicate records" in outs["m"][1] and "[seeksv] -M:" not in outs["f"][1]


def test_refusals(sample, tmp_path):
    d, plain, marked, fa = sample
    sam = str(tmp_path / "in.sam")
    with open(sam, "w") as f:
        f.write("".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(CI.NAMES, CI.LENS)))
    cases = [(["run", "-M", "-N", "2", plain, fa], "-N"), (["run", "-M", sam, fa], "SAM text"), (["somatic", "-M", plain, "x.clip.gz", "t.sv"], "-K")]
    for k, (args, word) in enumerate(cases):
        pre = str(tmp_path / f"refused{k}")
        r = subprocess.run([SEEKSV] + args + [pre], capture_output=True, text=True)
        lines = [l for l in r.stderr.splitlines() if not l.startswith("[stamp]")]
        assert r.returncode == 1 and len(lines) == 1 and "-M" in lines[0] and word in lines[0], (args, r.stderr)
        assert not glob.glob(pre + "*")
    # getclip and getsv have no such option
    r = subprocess.run([SEEKSV, "getclip", "-M", plain], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage: seeksv getclip" in r.stderr
    # an unsorted BAM: the library's message, status 1, and no output with anything in it
    contigs, recs = CI.sample()
    unsorted = str(tmp_path / "disorder.bam")
    bamio.write_bam(unsorted, list(CI.NAMES), list(CI.LENS), recs[200:400] + recs[:200])
    pre = str(tmp_path / "refused_unsorted")
    r = subprocess.run([SEEKSV, "run", "-M", unsorted, fa, pre], capture_output=True, text=True)
    lines = [l for l in r.stderr.splitlines() if l.startswith("[seeksv]")]
    assert r.returncode == 1 and len(lines) == 1 and "not coordinate sorted" in lines[0], r.stderr
    assert not glob.glob(pre + "*")                      # what the run had created is taken away again
    # the first usage line of both commands stays as it was, and both usage texts name the option
    for cmd, first in (("run", "Usage: seeksv run [options] <input.sorted.bam> <reference fasta(.gz)> <output prefix>"), ("somatic", "Usage: seeksv somatic [options] <input normal original bam>")):
        r = subprocess.run([SEEKSV, cmd], capture_output=True, text=True)
        assert r.stderr.splitlines()[0].startswith(first) and "         -M  " in r.stderr
