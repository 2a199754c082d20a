"""-m gpu: `seeksv getclip` and `seeksv run` on the original alignments as SAM text (a name without ".bam": plain, gzip, "-" for standard input; decoded on the
GPU, ssv_samdec_sorted): the four outputs of the bundled samples against the committed goldens of the real reference, everything else against this binary's
own run on the BAM of the same records - every file byte for byte after gunzip, stdout, and stderr behind libbam's [samopen] line.  Every test here fails on
the parent commit, which opens the name as a BAM and ends with "[main_samview] fail to open file for reading."."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bamio
import golden_util as G
import original_sam
import realign_split_inputs as SI
import sam_text as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
GZ = (".clip.gz", ".clip.fq.gz", ".unmapped_1.fq.gz", ".unmapped_2.fq.gz")
OPEN_ERROR = "[main_samview] fail to open file for reading.\n"


def samopen(n):
    return f"[samopen] SAM header is present: {n} sequences.\n"


def gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def getclip(args, env=None, stdin=None):
    return subprocess.run([SEEKSV, "getclip"] + args, capture_output=True, env=None if env is None else dict(os.environ, **env), input=stdin)


def outputs(prefix):
    return [gunzip(prefix + ext) for ext in GZ]


_texts = {}


def text_of(path, **kw):
    key = (path, tuple(sorted(kw.items())))
    if key not in _texts:
        _texts[key] = original_sam.sam_of_bam(path, **kw)
    return _texts[key]


def write_form(d, name, data, form):
    """the text as a file of the form -> (the <input> argument, what goes to standard input)"""
    if form == "stdin":
        return "-", data
    p = str(d / (name + (".sam.gz" if form == "gzip" else ".sam")))
    with (gzip.open(p, "wb") if form == "gzip" else open(p, "wb")) as f:
        f.write(data)
    return p, None


# ---- the bundled samples against the reference's goldens ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunks", [None, "64"], ids=["one-chunk", "64KB-chunks"])
@pytest.mark.parametrize("form", ["plain", "gzip", "stdin", "crlf", "no-final-newline"])
@pytest.mark.parametrize("sample", ["cancer", "normal"])
def test_example_samples(tmp_path, sample, form, chunks):
    data, _, names = text_of(os.path.join(G.GOLDEN, "example", sample + ".sort.bam"), crlf=form == "crlf", final_newline=form != "no-final-newline")
    arg, stdin = write_form(tmp_path, sample, data, form)
    out = str(tmp_path / "o")
    r = getclip(["-o", out, arg], env={"SSV_SAM_CHUNK_KB": chunks} if chunks else None, stdin=stdin)
    assert r.returncode == 0, r.stderr
    got = outputs(out)
    assert got[0].decode() == G.read_text("example", sample + ".clip.txt")
    assert got[1].decode() == G.read_text("example", sample + ".clip.fq.txt")
    assert got[2].decode() == G.read_text("example", sample + ".unmapped_1.fq.txt") and got[3].decode() == G.read_text("example", sample + ".unmapped_2.fq.txt")
    assert r.stderr.decode() == samopen(len(names)) + G.read_text("example", sample + ".getclip.stderr")


# ---- against this binary's own run on the BAM -----------------------------------------------------------------------------------------------------------------

def both_ways(d, bam, data, n_names, flags=(), env=None, form="plain"):
    a, b = str(d / "from_bam"), str(d / "from_text")
    arg, stdin = write_form(d, "in", data, form)
    r1 = getclip(list(flags) + ["-Z", "-o", a, bam], env=env)
    r2 = getclip(list(flags) + ["-o", b, arg], env=env, stdin=stdin)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
    for x, y, ext in zip(outputs(a), outputs(b), GZ):
        assert x == y, ext
    assert r2.stderr.decode() == samopen(n_names) + r1.stderr.decode() and r1.stdout == r2.stdout
    return outputs(a), r2.stderr.decode()


@pytest.mark.parametrize("seed", [200, 201])
def test_random_samples(tmp_path, seed):
    """the first two seeds of test_random_cli_vs_reference_gpu's getclip samples, with both of its option sets"""
    from test_random_cli_vs_reference_gpu import GETCLIP_RUNS, getclip_sample
    bam = str(tmp_path / "s.bam")
    getclip_sample(bam, seed)
    data, _, names = original_sam.sam_of_bam(bam)
    for tag, flags in GETCLIP_RUNS:
        d = tmp_path / tag
        d.mkdir()
        got, _ = both_ways(d, bam, data, len(names), flags, env={"SSV_SAM_CHUNK_KB": "32"})
        assert len(got[0]) > 1000


def test_synthfull(tmp_path, tmp_path_factory):
    import test_cli_gpu as TC
    bam, _, _ = TC._synth_sample(tmp_path_factory, "synthfull", TC.SYNTH_FULL["synthfull"])
    data, _, names = original_sam.sam_of_bam(bam)
    got, err = both_ways(tmp_path, bam, data, len(names), form="gzip")
    assert len(got[0]) > 1000


def test_unmapped_pairs(tmp_path):
    """a sample whose pairs have unmapped ends: the side channel's two files"""
    from test_random_cli_vs_reference_gpu import unmapped_pairs_sample
    bam = str(tmp_path / "u.bam")
    n_un = unmapped_pairs_sample(bam)
    data, _, names = original_sam.sam_of_bam(bam)
    got, err = both_ways(tmp_path, bam, data, len(names), env={"SSV_SAM_CHUNK_KB": "64"}, form="stdin")
    assert got[2].count(b"\n") == got[3].count(b"\n") and got[2].count(b"\n") > n_un // 2


@pytest.mark.parametrize("sub,bam,prefix,flags", [("getclip", "filters.bam", "filters.s", ["-s"]), ("getclip", "filters.bam", "filters.q30", ["-q", "30"]),
                                                  ("getclip", "stress1.bam", "stress1.t08", ["-t", "0.8"]), ("getclip", "unsorted.bam", "unsorted", [])], ids=lambda v: v if isinstance(v, str) and "." in v else "")
def test_options_on_hand_made_records(tmp_path, sub, bam, prefix, flags):
    """-s on records with XC:i:, -q, -t, contigs that come back (a pass per visit): the reference's goldens.  (lone_s.bam and lone_s2.bam hold records whose
    CIGAR and SEQ lengths disagree: text cannot say them - libbam's reader refuses such a line, and so does the decoder.)"""
    path = os.path.join(G.GOLDEN, sub, bam)
    data, _, names = original_sam.sam_of_bam(path)
    if "-s" in flags:
        assert b"XC:i:" in data
    got, err = both_ways(tmp_path, path, data, len(names), flags)
    assert got[0].decode() == G.read_text(sub, prefix + ".clip.txt") and got[1].decode() == G.read_text(sub, prefix + ".clip.fq.txt")


def test_q5_on_cancer(tmp_path):
    path = os.path.join(G.GOLDEN, "example", "cancer.sort.bam")
    data, _, names = text_of(path)
    got, err = both_ways(tmp_path, path, data, len(names), ["-q", "5"], env={"SSV_SAM_CHUNK_KB": "64", "SSV_PASS_RECORDS": "1"})
    assert got[0].decode() != G.read_text("example", "cancer.clip.txt")


def test_header_only(tmp_path):
    bam = str(tmp_path / "e.bam")
    bamio.write_bam(bam, ["c1", "c2"], [1000, 2000], [])
    data = b"@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:c1\tLN:1000\n@SQ\tSN:c2\tLN:2000\n"
    got, err = both_ways(tmp_path, bam, data, 2)
    assert got == [b"", b"", b"", b""]


def test_contig_comes_back(tmp_path):
    """records of c1, c2, then c1 again: two passes, three flushes"""
    rng = np.random.RandomState(5)
    import readthrough_inputs as RT
    names, lens = ["c1", "c2"], [5000, 5000]
    recs = []
    for tid, base in ((0, 100), (1, 200), (0, 3000)):
        for k in range(6):
            r = RT.rec(rng, f"r{tid}_{base}_{k}", tid, base + (k % 2), "30M20S" if k < 3 else "20S30M")
            r["qual"] = bytes(rng.randint(20, 40, 50).astype(np.uint8).tolist())
            recs.append(r)
    bam = str(tmp_path / "back.bam")
    bamio.write_bam(bam, names, lens, recs)
    data = ST.text(recs, names, lens).encode()
    got, err = both_ways(tmp_path, bam, data, 2)
    assert got[0].count(b"\n") > 0
    assert err.count("Output merged soft-clipped reads of c1\n") == 2 and err.count("Output merged soft-clipped reads of c2\n") == 1


# ---- seeksv run -----------------------------------------------------------------------------------------------------------------------------------------------

RUN_FILES_GZ = GZ + (".clip.bam",)
RUN_FILES = (".sv.txt", ".unmapped.clip.fq")


def run_cmd(args, stdin=None):
    return subprocess.run([SEEKSV, "run"] + args, capture_output=True, input=stdin)


def same_run(a, b, ra, rb):
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr[-600:], rb.stderr[-600:])
    for ext in RUN_FILES_GZ:
        assert gunzip(a + ext) == gunzip(b + ext), ext
    for ext in RUN_FILES:
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert ra.stdout == rb.stdout


@pytest.mark.parametrize("split", [[], ["-P"]], ids=["run", "run-P"])
def test_run_on_cancer(tmp_path, split):
    """`seeksv run` on the sample as a text file and on standard input against `run` on the .bam (a reference of random bases with the contigs' names and lengths)"""
    path = os.path.join(G.GOLDEN, "example", "cancer.sort.bam")
    data, _, _ = text_of(path)
    _, names, lens = original_sam.bam_header(path)
    rng = np.random.RandomState(17)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for n, l in zip(names, lens):
            s = "".join(rng.choice(list("ACGT"), l))
            f.write(f">{n}\n" + "\n".join(s[i:i + 60] for i in range(0, l, 60)) + "\n")
    sam = str(tmp_path / "cancer.sam")
    open(sam, "wb").write(data)
    a, b, c = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    ra = run_cmd(split + [path, fa, a])
    rb = run_cmd(split + [sam, fa, b])
    rc = run_cmd(split + ["-", fa, c], stdin=data)
    same_run(a, b, ra, rb)
    same_run(a, c, ra, rc)
    assert gunzip(b + ".clip.gz").decode() == G.read_text("example", "cancer.clip.txt")
    assert samopen(len(names)) in rb.stderr.decode() and samopen(len(names)) in rc.stderr.decode() and "[samopen]" not in ra.stderr.decode()


def test_run_P_with_unmapped_pairs(tmp_path):
    """the sample of test_run_split_gpu (ten split reads among the unmapped pairs): `run -P` on its text prints the table of `run -P` on its BAM"""
    from test_run_split_gpu import write_sample
    bam, fa = write_sample(tmp_path, SI.e2e_sample())
    data, _, names = original_sam.sam_of_bam(bam)
    sam = str(tmp_path / "s.sam.gz")
    with gzip.open(sam, "wb") as f:
        f.write(data)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ra, rb = run_cmd(["-P", bam, fa, a]), run_cmd(["-P", sam, fa, b])
    same_run(a, b, ra, rb)
    assert open(b + ".sv.txt").read() == G.read_text("realign_split", "e2e.F.sv") and rb.stdout.decode() == G.read_text("realign_split", "e2e.F.stdout")
    assert len(gunzip(b + ".unmapped_1.fq.gz")) > 0


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------

def nothing_written(d):
    return sorted(os.listdir(str(d))) == []


def test_refused_ranks(tmp_path):
    """-N 2 on a text input: one line, status 1, before any file is created - getclip and run"""
    data, _, _ = text_of(os.path.join(G.GOLDEN, "example", "cancer.sort.bam"))
    sam = str(tmp_path / "in" / "cancer.sam")
    os.makedirs(os.path.dirname(sam))
    open(sam, "wb").write(data)
    out = tmp_path / "out"
    out.mkdir()
    r = getclip(["-N", "2", "-o", str(out / "o"), sam])
    assert r.returncode == 1 and r.stderr.decode().count("\n") == 1 and "-N" in r.stderr.decode() and "SAM text" in r.stderr.decode() and nothing_written(out)
    r = run_cmd(["-N", "2", sam, str(tmp_path / "in" / "no.fa"), str(out / "o")])
    assert r.returncode == 1 and r.stderr.decode().count("\n") == 1 and "-N" in r.stderr.decode() and "SAM text" in r.stderr.decode() and nothing_written(out)


def test_refused_inputs(tmp_path):
    """a header without @SQ and a missing file end the command like a BAM that cannot be opened, before any file is created"""
    out = tmp_path / "out"
    out.mkdir()
    nosq = str(tmp_path / "nosq.sam")
    open(nosq, "wb").write(b"@HD\tVN:1.0\nr\t0\tc1\t1\t60\t5M\t*\t0\t0\tACGTA\tIIIII\n")
    r = getclip(["-o", str(out / "o"), nosq])
    assert r.returncode == 1 and r.stderr.decode() == "[samopen] no @SQ lines in the header.\n" + OPEN_ERROR and nothing_written(out)
    r = getclip(["-o", str(out / "o"), str(tmp_path / "missing.sam")])
    assert r.returncode == 1 and r.stderr.decode() == OPEN_ERROR and nothing_written(out)
    r = getclip(["-Z", "-C", "-o", str(out / "o"), str(tmp_path / "missing.sam.gz")])   # (-Z and -C are accepted and change nothing)
    assert r.returncode == 1 and r.stderr.decode() == OPEN_ERROR and nothing_written(out)


def incomplete(path):
    """the output does not look like a finished gzip file: it is not there, or gzip refuses it"""
    if not os.path.exists(path) or os.path.getsize(path) == 0:
        return True
    try:
        gunzip(path)
    except (EOFError, OSError):
        return True
    return False


def test_malformed_line(tmp_path):
    """a malformed line 3 (the message names the line of the FILE), and a malformed last line behind passes that were written: no output claims completeness"""
    bad = b"@SQ\tSN:c1\tLN:1000\nr1\t0\tc1\t1\t60\t5M\t*\t0\t0\tACGTA\tIIIII\nr2\t0\tc1\t2\t60\t5M\t*\t0\t0\tACGTA\n"
    sam = str(tmp_path / "bad.sam")
    open(sam, "wb").write(bad)
    out = str(tmp_path / "o")
    r = getclip(["-o", out, sam])
    assert r.returncode == 1 and r.stderr.decode() == samopen(1) + "Parse error at line 3: fewer than 11 fields\n"
    assert all(incomplete(out + ext) for ext in GZ)
    data, n_head, names = text_of(os.path.join(G.GOLDEN, "example", "cancer.sort.bam"))
    lines = data.split(b"\n")
    assert lines[-1] == b"" and lines[-2].count(b"\t") >= 10
    lines[-2] = lines[-2].replace(b"\t", b" ", 3)
    sam2 = str(tmp_path / "late.sam")
    open(sam2, "wb").write(b"\n".join(lines))
    out2 = str(tmp_path / "o2")
    r = getclip(["-o", out2, sam2], env={"SSV_SAM_CHUNK_KB": "64", "SSV_PASS_RECORDS": "1"})
    assert r.returncode == 1 and r.stderr.decode().endswith(f"Parse error at line {len(lines) - 1}: fewer than 11 fields\n")
    assert "Output merged soft-clipped reads of" in r.stderr.decode()   # (a pass had been written out)
    assert all(incomplete(out2 + ext) for ext in GZ)
