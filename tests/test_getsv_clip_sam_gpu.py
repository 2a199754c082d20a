"""-m gpu: `seeksv getsv <clip alignments as SAM text> ...` - the binary.  The reference opens getsv's first argument as it opens -F: a name ending in ".bam"
is BAM, every other name SAM text, plain or gzip, "-" standard input (getsv.h:437-446), so `bwa mem` output goes in as it is.  The text is parsed on the GPU
(ssv_samdec_*), packed there into the join's columns (ssv_aln_pack) and joined on the host.  The real reference writes the same bytes from the .bam and from
the text tests/clip_sam.py makes of it (tests/test_clip_sam_reference.py), so the committed outputs of the .bam runs are the expected outputs here."""
import gzip
import os
import subprocess

import pytest

import clip_sam
import golden_util as G
import readthrough_inputs as RT
import sam_text as ST
import test_cli_gpu as TC
import test_random_cli_vs_reference_gpu as RC

pytestmark = pytest.mark.gpu
SEEKSV = RC.SEEKSV
EX = os.path.join(G.GOLDEN, "example")
JOINED = "'InputSoftInfoStoreBreakpoint' finished"
OPEN_ERROR = "[main_samview] fail to open file for reading."
# name of the clip file, how its text is written, environment, where it comes from
FORMS = [("x.sam", {}, {}, "file"), ("x.sam.gz", {}, {}, "file"), ("alignments", {}, {}, "file"), ("crlf.sam", dict(crlf=True), {}, "file"),
         ("nonl.sam", dict(final_newline=False), {}, "file"), ("chunks.sam", {}, {"SSV_SAM_CHUNK_KB": "1"}, "file"), ("in.sam", {}, {}, "stdin"),
         ("in.sam.gz", {}, {"SSV_SAM_CHUNK_KB": "1"}, "stdin")]


def getsv(args, env=None, stdin=None):
    e = dict(os.environ)
    e.pop("SSV_SAM_CHUNK_KB", None)
    e.update(env or {})
    return subprocess.run([SEEKSV, "getsv"] + args, capture_output=True, text=True, env=e, stdin=stdin if stdin is not None else subprocess.DEVNULL)


def samopen_line(bam):
    return f"[samopen] SAM header is present: {len(clip_sam.bam_header(bam)[0])} sequences."


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """getclip of both bundled samples, once"""
    out = {}
    for sample in ("cancer", "normal"):
        d = tmp_path_factory.mktemp("clip_sam_" + sample)
        r = subprocess.run([SEEKSV, "getclip", "-o", str(d / "s"), os.path.join(EX, sample + ".sort.bam")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[sample] = (d, str(d / "s.clip.gz"))
    return out


@pytest.mark.parametrize("name,kw,env,source", FORMS, ids=[f[0] + ("@stdin" if f[3] == "stdin" else "") + ("+1KB" if f[2] else "") for f in FORMS])
@pytest.mark.parametrize("sample", ["cancer", "normal"])
def test_example_clip_alignments_as_sam_text(example, sample, name, kw, env, source):
    d, clip_gz = example[sample]
    bam = os.path.join(EX, sample + ".clip.bam")
    sam, sv, fq = str(d / name), str(d / (name + ".sv")), str(d / (name + ".fq"))
    clip_sam.write(sam, bam, **kw)
    if source == "stdin":
        with open(sam, "rb") as f:
            r = getsv(["-", os.path.join(EX, sample + ".sort.bam"), clip_gz, sv, fq], env=env, stdin=f)
    else:
        r = getsv([sam, os.path.join(EX, sample + ".sort.bam"), clip_gz, sv, fq], env=env)
    assert r.returncode == 0, r.stderr
    assert open(sv).read() == G.read_text("example", f"{sample}.sv")
    assert r.stdout == G.read_text("example", f"{sample}.getsv.stdout")
    err = r.stderr.splitlines()
    assert err.count(samopen_line(bam)) == 1 and sum(l.startswith("[samopen]") for l in err) == 1
    assert err.index(samopen_line(bam)) < err.index(JOINED)
    assert os.path.getsize(fq) == 0


def test_example_ranks_equal_single(example):
    d, clip_gz = example["cancer"]
    sam = str(d / "ranks.sam")
    clip_sam.write(sam, os.path.join(EX, "cancer.clip.bam"))
    r = getsv(["-N", "2", sam, os.path.join(EX, "cancer.sort.bam"), clip_gz, str(d / "ranks.sv"), str(d / "ranks.fq")])
    assert r.returncode == 0, r.stderr
    assert open(str(d / "ranks.sv")).read() == G.read_text("example", "cancer.sv")
    assert r.stdout == G.read_text("example", "cancer.getsv.stdout")
    assert r.stderr.splitlines().count(samopen_line(os.path.join(EX, "cancer.clip.bam"))) == 1


def test_with_F_as_well(tmp_path):
    """-F small.sam beside the clip alignments as SAM text: what the same command writes with the .bam clip file; the clip file's [samopen] line comes
    behind 'FindJunction' finished and in front of the join's line"""
    bg, clip_bam, clip_gz = RC.make_inputs(0, str(tmp_path))
    fsam, sam = str(tmp_path / "small.sam"), str(tmp_path / "in.clip.sam")
    ST.write(fsam, ST.clip_positions(RT.small_records(), RT.LENS), RT.NAMES, RT.LENS)
    clip_sam.write(sam, clip_bam)
    outs = []
    for tag, clip in (("bam", clip_bam), ("sam", sam)):
        sv = str(tmp_path / f"{tag}.sv")
        r = getsv(RT.LOOSE + ["-F", fsam, clip, bg, clip_gz, sv, str(tmp_path / "x.fq")])
        assert r.returncode == 0, r.stderr
        outs.append((open(sv).read(), r.stdout))
        err = r.stderr.splitlines()
        line = samopen_line(clip_bam)
        assert err.count(line) == (2 if tag == "sam" else 1)
        if tag == "sam":
            last = len(err) - 1 - err[::-1].index(line)
            assert err.index("'FindJunction' finished") < last < err.index(JOINED)
    assert outs[0] == outs[1]
    assert len([l for l in outs[0][0].splitlines() if not l.startswith("@")]) > 30


@pytest.mark.parametrize("seed", range(8))
def test_random_junction_inputs_as_sam_text(tmp_path, seed):
    """soft- and hard-clipped ends, MAPQ 0, secondary and unaligned records, 170-190 records a seed: the digests of what the real reference wrote"""
    ref = RC.reference_outputs()["getsv"][str(seed)]
    d = str(tmp_path)
    bg, clip_bam, clip_gz = RC.make_inputs(seed, d)
    sam = os.path.join(d, "in.clip.sam")
    data = clip_sam.write(sam, clip_bam)
    assert 170 <= sum(1 for l in data.split(b"\n") if l and not l.startswith(b"@")) <= 190
    for tag, flags in RC.GETSV_RUNS:
        sv = os.path.join(d, f"ours.{tag}.sv")
        r = getsv(flags + [sam, bg, clip_gz, sv, os.path.join(d, "o.fq")])
        assert r.returncode == 0, r.stderr[-400:]
        assert RC.sha(open(sv).read()) == ref[tag]["sv"], (seed, tag)
        assert RC.sha(r.stdout) == ref[tag]["stdout"], (seed, tag)


def test_synthetic_sample(tmp_path_factory):
    """synthfull (planted DEL / INV / TRA, test_cli_gpu.py) with bwa mem's committed clip.bam as SAM text: the committed table"""
    bam, clip_gz, d = TC._synth_sample(tmp_path_factory, "synthfull", TC.SYNTH_FULL["synthfull"])
    sam, sv = str(d / "synthfull.clip.sam"), str(d / "out.clipsam.sv")
    clip_sam.write(sam, os.path.join(G.GOLDEN, "synth", "synthfull.clip.bam"))
    r = getsv([sam, bam, clip_gz, sv, str(d / "u.clipsam.fq")])
    assert r.returncode == 0, r.stderr
    assert open(sv).read() == G.read_text("synth", "synthfull.sv")
    assert r.stdout == G.read_text("synth", "synthfull.stdout")


def test_refused_inputs(tmp_path):
    """a line with ten fields, a header without @SQ, a missing file: exit status 1, the message, and no table (the .bam path writes none either when
    its clip file cannot be read: the table is opened behind the BAM passes)"""
    bg, clip_bam, clip_gz = RC.make_inputs(0, str(tmp_path))
    lines = clip_sam.text(clip_bam).split("\n")
    n_hdr = sum(1 for l in lines if l.startswith("@"))
    k = n_hdr + 25
    assert len(lines[k].split("\t")) == 11
    bad = list(lines)
    bad[k] = "\t".join(lines[k].split("\t")[:10])
    cases = [("ten.sam", "\n".join(bad), [f"Parse error at line {k + 1}: fewer than 11 fields"]),
             ("nosq.sam", "@HD\tVN:1.0\n" + "\n".join(lines[n_hdr:]), ["[samopen] no @SQ lines in the header.", OPEN_ERROR]),
             ("missing.sam", None, [OPEN_ERROR])]
    for name, data, messages in cases:
        p, sv = str(tmp_path / name), str(tmp_path / (name + ".sv"))
        if data is not None:
            with open(p, "w") as f:
                f.write(data)
        for env in ({}, {"SSV_SAM_CHUNK_KB": "1"}):
            r = getsv([p, bg, clip_gz, sv, str(tmp_path / "x.fq")], env=env)
            assert r.returncode == 1, (name, r.stderr)
            err = r.stderr.splitlines()
            for m in messages:
                assert m in err, (name, r.stderr)
            assert JOINED not in err
            assert not os.path.exists(sv), name
    # ... as the .bam path leaves none
    sv = str(tmp_path / "nobam.sv")
    r = getsv([str(tmp_path / "missing.clip.bam"), bg, clip_gz, sv, str(tmp_path / "x.fq")])
    assert r.returncode == 1 and OPEN_ERROR in r.stderr.splitlines() and not os.path.exists(sv)
    # an empty standard input has no header: refused like a file without @SQ
    r = getsv(["-", bg, clip_gz, sv, str(tmp_path / "x.fq")])
    assert r.returncode == 1 and OPEN_ERROR in r.stderr.splitlines() and not os.path.exists(sv)


def test_gzip_on_standard_input_matches_the_file(tmp_path):
    """gzip text piped in (detected from the first bytes of the stream) gives what the plain file gives"""
    bg, clip_bam, clip_gz = RC.make_inputs(1, str(tmp_path))
    ref = RC.reference_outputs()["getsv"]["1"]["loose"]
    data = clip_sam.text(clip_bam).encode("latin-1")
    p = str(tmp_path / "piped")
    with open(p, "wb") as f:
        f.write(gzip.compress(data))
    sv = str(tmp_path / "o.sv")
    with open(p, "rb") as f:
        r = getsv(list(RC.GETSV_RUNS[1][1]) + ["-", bg, clip_gz, sv, str(tmp_path / "o.fq")], stdin=f)
    assert r.returncode == 0, r.stderr
    assert RC.sha(open(sv).read()) == ref["sv"] and RC.sha(r.stdout) == ref["stdout"]
