"""GPU, through the binary: `seeksv somatic -K` - the normal's clusters from its BAM, looked up on the GPU where they lie - writes what `seeksv getclip` on the
normal followed by `seeksv somatic` writes (the real reference's output where a golden exists), and no other file."""
import gzip
import os
import subprocess

import pytest

import bamio
import golden_util as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
SYNTH_FULL = dict(genome_frac=1 / 8192, depth=40, n_sv=24)
HBV_NORMAL = dict(genome_frac=1 / 8192, depth=30, n_sv=8, hbv=True)
SOMATIC_VARIANTS = [("", []), (".n0", ["-n", "0"]), (".l0", ["-l", "0"]), (".l60", ["-l", "60"]), (".t05", ["-t", "0.5"]), (".m60", ["-m", "60"]), (".q0", ["-q", "0"])]
LEFTOVERS = (".clip.gz", ".clip.fq.gz", ".unmapped_1.fq.gz", ".unmapped_2.fq.gz")
_samples = {}


def _synth_bam(tmp_path_factory, name, kw):
    """a synthetic sample regenerated and written as a BAM, in a directory of its own"""
    if name not in _samples:
        from seeksv_amd import synth
        d = tmp_path_factory.mktemp(name)
        w = synth.Workload(**kw)
        bam = str(d / f"{name}.bam")
        bamio.soa_to_bam(bam, w.names, w.lens, w.generate_host(0, w.n_total))
        _samples[name] = (bam, d)
    return _samples[name]


def _somatic_stderr(text):
    """the reference prints the BAM path it was given; compare everything else"""
    return [("Bam/sam <bam>" + l[l.index("    Mean insert size"):]) if l.startswith("Bam/sam ") else l for l in text.splitlines() if l != "'CalculateInsertsizeDeviation' finished"]


def _from_bam(args, cwd, env=None):
    """`seeksv somatic -K ...` in `cwd`; nothing but the named output may appear there"""
    before = set(os.listdir(cwd))
    r = subprocess.run([SEEKSV, "somatic", "-K"] + args, capture_output=True, text=True, cwd=str(cwd), env=dict(os.environ, **(env or {})))
    new = set(os.listdir(cwd)) - before
    return r, new


def _two_commands(bam, tumor, d, tag, clip_flags=(), flags=()):
    """`getclip [clip_flags]` then `somatic [flags]`: (output text, stderr, the clip.gz)"""
    pre = str(d / f"two{tag}")
    r = subprocess.run([SEEKSV, "getclip"] + list(clip_flags) + ["-o", pre, bam], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = pre + ".somatic.sv"
    r = subprocess.run([SEEKSV, "somatic"] + list(flags) + [bam, pre + ".clip.gz", tumor, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(out).read(), r.stderr, pre + ".clip.gz"


@pytest.mark.parametrize("tag,flags", SOMATIC_VARIANTS, ids=[t[0] or "default" for t in SOMATIC_VARIANTS])
def test_synthetic_sample_equals_reference(tmp_path_factory, tmp_path, tag, flags):
    bam, _ = _synth_bam(tmp_path_factory, "synthfull", SYNTH_FULL)
    r, new = _from_bam(flags + [bam, os.path.join(G.GOLDEN, "somatic", "tumor.sv"), "out.sv"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert new == {"out.sv"}
    assert open(str(tmp_path / "out.sv")).read() == G.read_text("somatic", f"somatic{tag}.sv")
    assert _somatic_stderr(r.stderr) == _somatic_stderr(G.read_text("somatic", f"somatic{tag}.stderr"))
    assert not [f for f in os.listdir(os.path.dirname(bam)) if f.endswith(LEFTOVERS) or ".unmapped_" in f]


@pytest.mark.parametrize("tag,flags", [("", []), (".n0", ["-n", "0"]), (".q0", ["-q", "0"])], ids=["default", "n0", "q0"])
def test_virus_integration_pair_equals_reference(tmp_path_factory, tmp_path, tag, flags):
    bam, _ = _synth_bam(tmp_path_factory, "hbvnormal", HBV_NORMAL)
    r, new = _from_bam(flags + [bam, os.path.join(G.GOLDEN, "synth", "hbvfull.loose.sv"), "out.sv"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert new == {"out.sv"}
    assert open(str(tmp_path / "out.sv")).read() == G.read_text("somatic", f"hbv.somatic{tag}.sv")
    assert _somatic_stderr(r.stderr) == _somatic_stderr(G.read_text("somatic", f"hbv.somatic{tag}.stderr"))


def test_example_equals_reference(tmp_path):
    ex = os.path.join(G.GOLDEN, "example")
    r, new = _from_bam([os.path.join(ex, "normal.sort.bam"), os.path.join(ex, "cancer.sv"), str(tmp_path / "somatic.sv")], tmp_path)
    assert r.returncode == 0, r.stderr
    assert new == {"somatic.sv"}
    assert open(str(tmp_path / "somatic.sv")).read() == G.read_text("example", "cancer.somatic.temp.sv")


def test_clip_options_equal_getclip_with_them(tmp_path_factory, tmp_path):
    bam, d = _synth_bam(tmp_path_factory, "synthfull", SYNTH_FULL)
    tumor = os.path.join(G.GOLDEN, "somatic", "tumor.sv")
    plain = G.read_text("somatic", "somatic.sv")
    changed = []
    for tag, clip_flags in (("q30s", ["-q", "30", "-s"]), ("t08", ["-t", "0.8"])):
        want, want_err, _ = _two_commands(bam, tumor, tmp_path, tag, clip_flags)
        out = f"out.{tag}.sv"
        r, new = _from_bam(["-c", " ".join(clip_flags), bam, tumor, out], tmp_path)
        assert r.returncode == 0, r.stderr
        assert new == {out}
        assert open(str(tmp_path / out)).read() == want, tag
        assert _somatic_stderr(r.stderr) == _somatic_stderr(want_err)
        changed.append(want != plain)
    assert any(changed), "no clip option changed the table: the case shows nothing"


def test_dump_equals_dump_of_the_clip_file(tmp_path_factory, tmp_path):
    bam, d = _synth_bam(tmp_path_factory, "synthfull", SYNTH_FULL)
    tumor = os.path.join(G.GOLDEN, "somatic", "tumor.sv")
    _, _, clip_gz = _two_commands(bam, tumor, tmp_path, ".dump")
    r = subprocess.run([SEEKSV, "somatic", "-J", str(tmp_path / "host.dump"), "unused.bam", clip_gz, tumor, "unused.out"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    before = set(os.listdir(str(tmp_path)))
    k = subprocess.run([SEEKSV, "somatic", "-K", "-J", str(tmp_path / "gpu.dump"), bam, tumor, "unused.out"], capture_output=True, text=True, cwd=str(tmp_path))
    assert k.returncode == 0, k.stderr
    assert set(os.listdir(str(tmp_path))) - before == {"gpu.dump"}
    assert open(str(tmp_path / "gpu.dump")).read() == open(str(tmp_path / "host.dump")).read()
    assert k.stderr.splitlines() == r.stderr.splitlines()


_RC = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def _rc(s):
    return "".join(_RC.get(c, c) for c in reversed(s))


def _tumor_rows_of(clip_rows):
    """a tumor table made of a sample's own clusters: for every cluster the nine shapes of a row (three strand pairs x microhomology known / only the right /
    only the left breakend clipped) with the cluster's strings where that shape's exact probe or its anchored probe reads them"""
    lines = ["@up_chr\tup_pos\tup_strand"]
    for row in clip_rows:
        chrom, pos, side, _, aligned, _, clipped, _, _ = row.split("\t")
        pos = int(pos)
        left, right = (clipped, aligned) if side == "5" else (aligned, clipped)
        for us, ds in (("+", "+"), ("+", "-"), ("-", "+")):
            for mh, up_reads, down_reads in ((0, 3, 3), (-1, 0, 4), (-1, 4, 0)):
                for up_seq, down_seq in ((left, right), (_rc(right), _rc(left))):
                    for shift in (0, 2):
                        c = [chrom, pos + shift, us, up_reads, chrom, pos - shift, ds, down_reads, mh, 0, "DEL", 10, 10, 1, 1, 1, 1, 0.5, 0.5, "50M", "50M", up_seq, down_seq]
                        lines.append("\t".join(str(x) for x in c))
    return "\n".join(lines) + "\n"


def test_unsorted_input_in_many_passes(tmp_path):
    """tests/golden/getclip/unsorted.bam: contigs come back (c1 three times with a cluster on one key each time), every contig change ends a pass"""
    bam = os.path.join(G.GOLDEN, "getclip", "unsorted.bam")
    clip_rows = G.read_text("getclip", "unsorted.clip.txt").splitlines()
    tumor = str(tmp_path / "tumor.sv")
    with open(tumor, "w") as f:
        f.write(_tumor_rows_of(clip_rows))
    want, want_err, clip_gz = _two_commands(bam, tumor, tmp_path, "")
    assert gzip.open(clip_gz, "rt").read().splitlines() == clip_rows
    counts = [l.split("\t")[23:25] for l in want.splitlines()[1:]]
    assert sum(1 for a, b in counts if a != "0") > 10 and sum(1 for a, b in counts if b != "0") > 10, "the made-up table finds nothing: the case shows nothing"
    # every key that comes back has another support in every visit (c1:1001 '5': 3, 2, 1; c1:2000 '3' and c2:101 '5': 1, 2): the first visit's is the one found
    assert {x for ab in counts for x in ab} == {"0", "1", "3"}
    for env in ({"SSV_PASS_RECORDS": "1"}, {}):
        out = "out%d.sv" % len(env)
        r, new = _from_bam([bam, tumor, out], tmp_path, env)
        assert r.returncode == 0, r.stderr
        assert new == {out}
        assert open(str(tmp_path / out)).read() == want
        assert _somatic_stderr(r.stderr) == _somatic_stderr(want_err)
    r = subprocess.run([SEEKSV, "somatic", "-J", str(tmp_path / "host.dump"), "unused.bam", clip_gz, tumor, "unused.out"], capture_output=True, text=True)
    k = subprocess.run([SEEKSV, "somatic", "-K", "-J", str(tmp_path / "gpu.dump"), bam, tumor, "unused.out"], capture_output=True, text=True, env=dict(os.environ, SSV_PASS_RECORDS="1"))
    assert r.returncode == 0 and k.returncode == 0, (r.stderr, k.stderr)
    assert open(str(tmp_path / "gpu.dump")).read() == open(str(tmp_path / "host.dump")).read()


REFUSALS = [
    (["-c", "-s", "n.bam", "n.clip.gz", "t.sv", "out.sv"], "-c hands getclip's options to the clip pass of -K"),
    (["-K", "-c", "-N 2", "n.bam", "t.sv", "out.sv"], "-N, -G or -o inside -c is not supported"),
    (["-K", "-c", "-G 0", "n.bam", "t.sv", "out.sv"], "-N, -G or -o inside -c is not supported"),
    (["-K", "-c", "-o x", "n.bam", "t.sv", "out.sv"], "-N, -G or -o inside -c is not supported"),
    (["-K", "-N", "2", "n.bam", "t.sv", "out.sv"], "-N above 1 is not supported"),
    (["-K", "n.sam", "t.sv", "out.sv"], "the normal must be a BAM"),
]


@pytest.mark.parametrize("args,message", REFUSALS, ids=["c-without-K", "N-in-c", "G-in-c", "o-in-c", "N2", "not-bam"])
def test_refusals_write_nothing(tmp_path, args, message):
    r = subprocess.run([SEEKSV, "somatic"] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr and len(r.stderr.splitlines()) == 1
    assert os.listdir(str(tmp_path)) == []
