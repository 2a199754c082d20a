"""-m gpu: `seeksv getsv -F <SAM text>` - the binary.  `bwa bwasw` writes SAM text, and the reference opens every -F name that does not end in ".bam"
as text (process_bwasw.cpp:12-16): the text is parsed on the GPU (ssv_samdec_*) into the batches the -F kernels consume.  Against what the real reference
writes: for the BAM form of all records (tests/golden/readthrough/small.json, random.json, large.json - '=' and 'X' CIGARs decode as BAM's codes 7 and 8) and
for the SAM-text form of the records libbam's text reader accepts (sam.json, tests/golden/make_readthrough_sam_reference.py)."""
import os
import subprocess

import pytest

import bamio
import readthrough_inputs as RT
import sam_text as ST
import test_random_cli_vs_reference_gpu as RC
from test_readthrough_gpu import SEEKSV, check_stderr, getsv, sha, want

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("rt_sam_small")
    recs = ST.clip_positions(RT.small_records(), RT.LENS)
    fsam, fsub = str(d / "small.sam"), str(d / "small_sub.sam")
    ST.write(fsam, recs, RT.NAMES, RT.LENS)
    ST.write(fsub, ST.without_eq_x(recs), RT.NAMES, RT.LENS)
    clip_bam, clip = RT.empty_clip_inputs(str(d))
    bfile = str(d / "b.txt")
    with open(bfile, "w") as f:
        f.write(RT.b_rows())
    return dict(dir=d, recs=recs, sam=fsam, sub=fsub, clip_bam=clip_bam, clip=clip, bfile=bfile)


def run_small(small, tmp_path, fpath, flags, extra=(), env=None):
    sv = str(tmp_path / "o.sv")
    r = getsv(list(extra) + RT.flags_with(flags, small["bfile"]) + ["-F", fpath, small["clip_bam"], RT.BG, small["clip"], sv, str(tmp_path / "x.fq")], env=env)
    return r, (open(sv).read() if os.path.exists(sv) else None)


@pytest.mark.parametrize("tag,flags", RT.SMALL_RUNS, ids=[t for t, _ in RT.SMALL_RUNS])
def test_getsv_F_sam_small_equals_reference(tmp_path, small, tag, flags):
    """-F small.sam with ALL of small_records() equals what the reference writes for the BAM of them: the .sv table, stdout, the order of the stderr lines;
    the subset without '=' / 'X' CIGARs equals what the reference writes for that SAM text (its "[samopen] SAM header is present" line included)"""
    w = want("small")[tag]
    r, sv = run_small(small, tmp_path, small["sam"], flags)
    assert r.returncode == 0, r.stderr
    assert sv == w["sv"]
    assert r.stdout == w["stdout"]
    check_stderr(r.stderr, w["stderr_lines"])
    ws = want("sam")["small"][tag]
    r, sv = run_small(small, tmp_path, small["sub"], flags)
    assert r.returncode == 0, r.stderr
    assert sv == ws["sv"]
    assert r.stdout == ws["stdout"]
    check_stderr(r.stderr, ws["stderr_lines"])
    assert "[samopen] SAM header is present: 3 sequences." in r.stderr.splitlines() and "[samopen] SAM header is present: 3 sequences." in ws["stderr_lines"]


@pytest.mark.parametrize("seed", RT.RANDOM_SEEDS)
def test_getsv_F_sam_random_equals_reference(tmp_path, seed):
    """a few thousand random split alignments as SAM text beside a clip join: all records against random.json's digests (the reference on the BAM), the
    '=' / 'X'-free subset against sam.json's (the reference on that SAM text)"""
    bg, clip_bam, clip_gz = RC.make_inputs(seed, str(tmp_path))
    recs = ST.clip_positions(RT.random_records(seed), RT.LENS)
    for name, rr, w in (("f.sam", recs, want("random")[str(seed)]), ("sub.sam", ST.without_eq_x(recs), want("sam")["random"][str(seed)])):
        fsam = str(tmp_path / name)
        ST.write(fsam, rr, RT.NAMES, RT.LENS)
        assert len(rr) == w["records"]
        for tag, flags in RT.RANDOM_RUNS:
            sv = str(tmp_path / f"o.{name}.{tag}.sv")
            r = getsv(flags + ["-F", fsam, clip_bam, bg, clip_gz, sv, str(tmp_path / "x.fq")])
            assert r.returncode == 0, r.stderr
            text = open(sv).read()
            assert text.count("\n") == w[tag]["sv_lines"], (name, tag)
            assert sha(text) == w[tag]["sv"], (name, tag)
            assert sha(r.stdout) == w[tag]["stdout"], (name, tag)


@pytest.fixture(scope="module")
def large(tmp_path_factory):
    d = tmp_path_factory.mktemp("rt_sam_large")
    recs = ST.clip_positions(RT.random_records(RT.LARGE_SEED, n_names=RT.LARGE_NAMES), RT.LENS)
    fsam = str(d / "large.sam")
    ST.write(fsam, recs, RT.NAMES, RT.LENS)
    clip_bam, clip = RT.empty_clip_inputs(str(d))
    return fsam, clip_bam, clip, len(recs)


@pytest.mark.parametrize("chunk_kb", [None, "64"], ids=["default_chunk", "64KB_chunks"])
def test_getsv_F_sam_large_file(tmp_path, large, chunk_kb):
    """~137 k split alignments in read order as one chunk of text and as several hundred 64 KB chunks (lines carried over every seam, chunks announced
    ahead): the reference's output for the BAM of the same records"""
    fsam, clip_bam, clip, n = large
    w = want("large")
    assert n == w["records"]
    env = dict(os.environ)
    env.pop("SSV_SAM_CHUNK_KB", None)
    if chunk_kb:
        env["SSV_SAM_CHUNK_KB"] = chunk_kb
    sv = str(tmp_path / "o.sv")
    r = getsv(RT.LOOSE + ["-F", fsam, clip_bam, RT.BG, clip, sv, str(tmp_path / "x.fq")], env=env)
    assert r.returncode == 0, r.stderr
    text = open(sv).read()
    assert text.count("\n") == w["sv_lines"]
    assert sha(text) == w["sv"]
    assert sha(r.stdout) == w["stdout"]


def test_getsv_F_sam_forms_of_the_file(tmp_path, small):
    """gzip-compressed, CRLF line ends, no final newline, a name without ".sam", lower-case bases / hex flags / optional fields, and -Z: all equal the plain form"""
    w = want("small")["loose"]
    recs = small["recs"]
    forms = (("s.sam.gz", {}), ("crlf.sam", dict(crlf=True)), ("nonl.sam", dict(final_newline=False)), ("x.txt", {}), ("crlf_nonl.sam.gz", dict(crlf=True, final_newline=False)),
             ("variants.sam", dict(lower=True, dot_n=True, hex_flags=True, tags=True)))
    for name, kw in forms:
        p = str(tmp_path / name)
        ST.write(p, recs, RT.NAMES, RT.LENS, **kw)
        for env in (None, dict(os.environ, SSV_SAM_CHUNK_KB="1")):
            r, sv = run_small(small, tmp_path, p, RT.LOOSE, env=env)
            assert r.returncode == 0, (name, r.stderr)
            assert sv == w["sv"] and r.stdout == w["stdout"], name
    r, sv = run_small(small, tmp_path, small["sam"], RT.LOOSE, extra=["-Z"])
    assert r.returncode == 0 and sv == w["sv"] and r.stdout == w["stdout"]


def test_getsv_F_sam_without_sq_lines(tmp_path, small):
    """a SAM without any @SQ line, with and without records: refused at open - two messages, exit status 1"""
    line = ST.line(small["recs"][0], RT.NAMES)
    for name, data in (("nosq.sam", "@HD\tVN:1.0\n" + line + "\n"), ("nosq_norec.sam", "@HD\tVN:1.0\n@PG\tID:bwa\n"), ("bare.sam", line + "\n"), ("empty.sam", "")):
        p = str(tmp_path / name)
        with open(p, "w") as f:
            f.write(data)
        r, sv = run_small(small, tmp_path, p, RT.LOOSE)
        assert r.returncode == 1, name
        err = r.stderr.splitlines()
        assert "[samopen] no @SQ lines in the header." in err and "[main_samview] fail to open file for reading." in err, name
        assert err.index("[samopen] no @SQ lines in the header.") < err.index("[main_samview] fail to open file for reading.")
    r, _ = run_small(small, tmp_path, str(tmp_path / "not_there.sam"), RT.LOOSE)
    assert r.returncode == 1 and "[main_samview] fail to open file for reading." in r.stderr


def test_getsv_F_sam_header_only_file(tmp_path, small):
    """@SQ lines and no record: an empty -F file, like an empty BAM"""
    p = str(tmp_path / "hdr.sam")
    with open(p, "w") as f:
        f.write(ST.header(RT.NAMES, RT.LENS))
    r, sv = run_small(small, tmp_path, p, RT.LOOSE)
    assert r.returncode == 0, r.stderr
    assert "[samopen] SAM header is present: 3 sequences." in r.stderr and "'FindJunction' finished" in r.stderr
    assert [l for l in sv.splitlines() if not l.startswith("@")] == []


@pytest.mark.parametrize("chunk_kb", [None, "1"], ids=["one_chunk", "1KB_chunks"])
def test_getsv_F_sam_malformed_line(tmp_path, small, chunk_kb):
    """a malformed line: the reference's message form with the line's number in the file (header lines count), exit status 1"""
    lines = ST.text(small["recs"], RT.NAMES, RT.LENS).split("\n")
    n_hdr = sum(1 for l in lines if l.startswith("@"))
    k = n_hdr + 40
    f = lines[k].split("\t")
    f[5] = f[5][:-1] + "Q"
    lines[k] = "\t".join(f)
    p = str(tmp_path / "bad.sam")
    with open(p, "w") as fh:
        fh.write("\n".join(lines))
    env = dict(os.environ, SSV_SAM_CHUNK_KB=chunk_kb) if chunk_kb else None
    r, _ = run_small(small, tmp_path, p, RT.LOOSE, env=env)
    assert r.returncode == 1
    assert f"Parse error at line {k + 1}: invalid CIGAR character" in r.stderr.splitlines()
    assert "'FindJunction' finished" not in r.stderr


def test_getsv_F_sam_ranks_equal_single(tmp_path, small):
    """getsv -N 2 -F small.sam equals -N 1"""
    outs = []
    for n in (1, 2):
        r, sv = run_small(small, tmp_path, small["sam"], RT.LOOSE, extra=["-N", str(n)])
        assert r.returncode == 0, r.stderr
        outs.append((sv, r.stdout))
    assert outs[0] == outs[1]
    assert outs[0][0] == want("small")["loose"]["sv"]


def test_run_passes_F_sam_to_getsv(tmp_path):
    """`seeksv run -v "-F f.sam ..."` writes what the run with f.bam writes"""
    from seeksv_amd import synth
    w = synth.Workload(genome_frac=1 / 8192, depth=20, n_sv=8)
    bam = str(tmp_path / "s.bam")
    bamio.soa_to_bam(bam, w.names, w.lens, w.generate_host(0, w.n_total))
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        f.write(w.reference_fasta())
    lens = [int(x) for x in w.lens]
    recs = ST.clip_positions(RT.random_records(11, n_names=800, lens=lens), lens)
    fbam, fsam = str(tmp_path / "f.bam"), str(tmp_path / "f.sam")
    RT.write_f_bam(fbam, recs, names=w.names, lens=lens)
    ST.write(fsam, recs, list(w.names), lens)
    outs = []
    for tag, ff in (("bam", fbam), ("sam", fsam)):
        pre = str(tmp_path / tag)
        r = subprocess.run([SEEKSV, "run", "-v", " ".join(["-F", ff, "-w", "0"] + RT.LOOSE), bam, fa, pre], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "'FindJunction' finished" in r.stderr
        outs.append((open(pre + ".sv.txt").read(), open(pre + ".unmapped.clip.fq").read(), r.stdout))
    assert outs[0] == outs[1]
    assert len([l for l in outs[1][0].splitlines() if not l.startswith("@")]) > 0
