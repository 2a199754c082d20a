"""-m gpu: `seeksv run -N n` - the one-decode path over n ranks: every rank decodes its run of the BAM once and keeps it in its own context's memory
(on a one-GPU box the ranks share the GPU and the exchange goes through host memory), the aligner step runs on the first device, the getsv pass scans
the ranks' records where they lie and the tallies meet in one all-gather.  Every file and stdout must be what `seeksv run` on one GPU writes."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bamio
import golden_util as G
import readthrough_inputs as RT
import test_cli_gpu as T
from seeksv_amd import host

pytestmark = pytest.mark.gpu

SEEKSV = T.SEEKSV
GZ = (".clip.gz", ".clip.fq.gz", ".unmapped_1.fq.gz", ".unmapped_2.fq.gz")
PLAIN = (".sv.txt", ".unmapped.clip.fq")
OPTS = ["-c", "-q 5 -t 0.85", "-v", "-b 2 -L 100 -q 10"]
SMALL_CHUNKS = {"SSV_CHUNK_INFLATED_MB": "1", "SSV_STAGE_MB": "1"}   # a rank keeps several batches, records straddle chunks
RANK_LINE = re.compile(r"^\[timing\] \(run -N rank (\d+)/(\d+): device (\d+), (\d+) records kept, (\d+) halo records\)$")

_samples = {}
_plain = {}


def _sample(tmp_path_factory, name):
    """(bam, fasta, directory, workload) of a synthetic sample, written once"""
    if name not in _samples:
        from seeksv_amd import synth
        kw = T.SYNTH_FULL[name]
        bam, _, d = T._synth_sample(tmp_path_factory, name, kw)
        w = synth.Workload(**kw)
        fa = str(d / "ref_ranks.fa")
        with open(fa, "w") as f:
            f.write(w.reference_fasta())
        _samples[name] = (bam, fa, d, w)
    return _samples[name]


def _run(args, env=None):
    return subprocess.run([SEEKSV, "run"] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))


def _bam_columns(path):
    cols = []
    with host.BamReader(path) as r:
        while True:
            b = r.read_batch(1 << 22, keep_all_seq=True)
            if b is None:
                break
            cols.append(tuple(b[k].tobytes() for k in ("tid", "pos", "flag", "mapq", "n_cigar", "l_qseq", "cigar")))
        return r.target_names, [int(x) for x in r.target_lens], cols


def _outputs(prefix):
    """every file of a run: .gz files decompressed, plain files as they are, clip.bam record for record; a file that is not there is None"""
    out = {}
    for ext in GZ:
        out[ext] = gzip.open(prefix + ext, "rb").read() if os.path.exists(prefix + ext) else None
    for ext in PLAIN:
        out[ext] = open(prefix + ext, "rb").read() if os.path.exists(prefix + ext) else None
    out[".clip.bam"] = _bam_columns(prefix + ".clip.bam") if os.path.exists(prefix + ".clip.bam") else None
    return out


def _plain_run(tmp_path_factory, name, opts=(), tag="d"):
    """`seeksv run` without -N on a sample: (outputs, stdout), computed once per option set"""
    key = (name, tag)
    if key not in _plain:
        bam, fa, d, _ = _sample(tmp_path_factory, name)
        p = str(d / f"plain_{tag}")
        r = _run(list(opts) + [bam, fa, p])
        assert r.returncode == 0, r.stderr
        _plain[key] = (_outputs(p), r.stdout)
    return _plain[key]


def _same(got, want):
    for ext in want:
        assert got[ext] is not None and got[ext] == want[ext], ext


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("name", list(T.SYNTH_FULL))
def test_run_ranks_equals_run(tmp_path_factory, tmp_path, name, n):
    """default options: six files, clip.bam and stdout of `run -N n` are `run`'s; synthfull's table is the real reference's (tests/golden/synth)"""
    bam, fa, _, _ = _sample(tmp_path_factory, name)
    want, want_stdout = _plain_run(tmp_path_factory, name)
    p = str(tmp_path / "r")
    r = _run(["-N", str(n), bam, fa, p])
    assert r.returncode == 0, r.stderr
    _same(_outputs(p), want)
    assert r.stdout == want_stdout
    assert not os.path.exists(p + ".clip.bam.tmp")
    assert "[timing]" not in r.stderr
    if name == "synthfull":
        assert open(p + ".sv.txt").read() == G.read_text("synth", "synthfull.sv")


@pytest.mark.parametrize("variant,name,n,opts,env", [("options", "synthfull", 3, OPTS, {}), ("small-chunks", "synthfull", 2, [], SMALL_CHUNKS),
                                                     ("sorted-index", "hbvfull", 2, ["-a", "-c 500"], {})], ids=["options", "small-chunks", "sorted-index"])
def test_run_ranks_variants(tmp_path_factory, tmp_path, variant, name, n, opts, env):
    """options of all three steps reach the ranks; chunks of 1 MB: a rank retains several batches; -a "-c 500": the aligner step's sorted index"""
    bam, fa, _, _ = _sample(tmp_path_factory, name)
    want, want_stdout = _plain_run(tmp_path_factory, name, opts, tag="d" if not opts else variant)
    p = str(tmp_path / "r")
    r = _run(["-N", str(n)] + opts + [bam, fa, p], env)
    assert r.returncode == 0, r.stderr
    _same(_outputs(p), want)
    assert r.stdout == want_stdout
    assert len([l for l in open(p + ".sv.txt") if not l.startswith("@")]) > 0


def _records(path):
    n = 0
    with host.BamReader(path) as r:
        while True:
            b = r.read_batch(1 << 20)
            if b is None:
                return n
            n += len(b["tid"])


@pytest.mark.parametrize("n,env", [(3, {}), (8, SMALL_CHUNKS)], ids=["3", "8-small-chunks"])
def test_run_ranks_accounting(tmp_path_factory, tmp_path, n, env):
    """SSV_TIMING=1: one line per rank; the records the ranks kept add up to the file's - none scanned twice, none dropped - and the exchange ran"""
    bam, fa, _, _ = _sample(tmp_path_factory, "synthfull")
    want, want_stdout = _plain_run(tmp_path_factory, "synthfull")
    p = str(tmp_path / "r")
    r = _run(["-N", str(n), bam, fa, p], dict(env, SSV_TIMING="1"))
    assert r.returncode == 0, r.stderr
    lines = [RANK_LINE.match(l) for l in r.stderr.splitlines() if l.startswith("[timing] (run -N rank ")]
    assert all(lines) and [int(m.group(1)) for m in lines] == list(range(n)) and all(int(m.group(2)) == n for m in lines)
    kept = [int(m.group(4)) for m in lines]
    assert sum(kept) == _records(bam)
    assert sum(1 for k in kept if k > 0) >= 2
    assert int(lines[0].group(5)) == 0   # rank 0 has nothing before its run
    assert len([l for l in r.stderr.splitlines() if l.startswith("[timing] exchange over ")]) == 1
    _same(_outputs(p), want)
    assert r.stdout == want_stdout


def test_run_ranks_empty_ranks(tmp_path_factory, tmp_path):
    """five records for eight ranks: most ranks own nothing, and the outputs are still `run`'s"""
    _, fa, _, w = _sample(tmp_path_factory, "synthfull")
    bam = str(tmp_path / "five.bam")
    bamio.soa_to_bam(bam, w.names, w.lens, w.generate_host(0, 5))
    assert _records(bam) == 5
    a, b = str(tmp_path / "one"), str(tmp_path / "eight")
    r1 = _run([bam, fa, a])
    assert r1.returncode == 0, r1.stderr
    r8 = _run(["-N", "8", bam, fa, b])
    assert r8.returncode == 0, r8.stderr
    _same(_outputs(b), _outputs(a))
    assert r8.stdout == r1.stdout


def _stderr_lines(r):
    return [l for l in r.stderr.splitlines() if not l.startswith("[stamp]")]


def test_run_ranks_halo_too_small_is_refused(tmp_path_factory, tmp_path):
    bam, fa, _, _ = _sample(tmp_path_factory, "synthfull")
    p = str(tmp_path / "r")
    r = _run(["-N", "2", "-c", "-H 10", bam, fa, p])
    assert r.returncode == 1 and "rerun with -H" in r.stderr, r.stderr
    assert not os.path.exists(p + ".sv.txt") and not os.path.exists(p + ".clip.bam")


@pytest.mark.parametrize("args,words", [(["-N", "2", "-P"], ("-P", "-N")), (["-N", "2", "-c", "-N 2"], ("-N", "-c")), (["-N", "2", "-v", "-G 1"], ("-G", "-v"))],
                         ids=["with-P", "N-in-c", "G-in-v"])
def test_run_ranks_refusals(tmp_path_factory, tmp_path, args, words):
    """one line on stderr, status 1, nothing written"""
    bam, fa, _, _ = _sample(tmp_path_factory, "synthfull")
    d = tmp_path / "out"
    d.mkdir()
    r = _run(args + [bam, fa, str(d / "r")])
    lines = _stderr_lines(r)
    assert r.returncode == 1 and len(lines) == 1 and all(w in lines[0] for w in words), r.stderr
    assert os.listdir(str(d)) == []


def test_run_ranks_usage_for_zero_ranks(tmp_path):
    r = _run(["-N", "0", "a.bam", "ref.fa", str(tmp_path / "r")])
    assert r.returncode == 1 and r.stderr.startswith("Usage: seeksv run")
    assert os.listdir(str(tmp_path)) == []


def test_run_ranks_contigs_that_come_back(tmp_path):
    """a file whose contigs come back: the ranks give way to one GPU, and `run -N 2` ends as `run` ends on that file - same status, same files"""
    bam = os.path.join(G.GOLDEN, "getclip", "unsorted.bam")
    with host.BamReader(bam) as r:
        names, lens = r.target_names, [int(x) for x in r.target_lens]
    rng = np.random.default_rng(17)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for name, ln in zip(names, lens):
            f.write(f">{name}\n" + "".join("ACGT"[k] for k in rng.integers(0, 4, ln)) + "\n")
    da, db = tmp_path / "one", tmp_path / "two"
    da.mkdir()
    db.mkdir()
    r1 = _run([bam, fa, str(da / "r")])
    r2 = _run(["-N", "2", bam, fa, str(db / "r")])
    assert r2.returncode == r1.returncode, r2.stderr
    assert sorted(os.listdir(str(da))) == sorted(os.listdir(str(db)))
    assert _outputs(str(db / "r")) == _outputs(str(da / "r"))
    assert r2.stdout == r1.stdout
    extra = [l for l in _stderr_lines(r2) if l not in _stderr_lines(r1)]
    assert len(extra) == 1 and "run -N" in extra[0]   # the one line that says so


def test_run_ranks_passes_F_to_getsv(tmp_path):
    """`run -N 2 -v "-F f.bam ..."`: the -F pass runs once, on the first device, and the outputs are `run -v "-F ..."`'s"""
    from seeksv_amd import synth
    w = synth.Workload(genome_frac=1 / 8192, depth=20, n_sv=8)
    bam = str(tmp_path / "s.bam")
    bamio.soa_to_bam(bam, w.names, w.lens, w.generate_host(0, w.n_total))
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        f.write(w.reference_fasta())
    fbam = str(tmp_path / "f.bam")
    RT.write_f_bam(fbam, RT.random_records(11, n_names=800, lens=w.lens), names=w.names, lens=w.lens)
    sv_o = " ".join(["-F", fbam, "-w", "0"] + RT.LOOSE)
    a, b = str(tmp_path / "one"), str(tmp_path / "two")
    r1 = _run(["-v", sv_o, bam, fa, a])
    assert r1.returncode == 0, r1.stderr
    r2 = _run(["-N", "2", "-v", sv_o, bam, fa, b])
    assert r2.returncode == 0, r2.stderr
    _same(_outputs(b), _outputs(a))
    assert r2.stdout == r1.stdout
    assert "'FindJunction' finished" in r2.stderr
    assert len([l for l in open(b + ".sv.txt") if not l.startswith("@")]) > 0
