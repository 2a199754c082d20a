"""-m gpu: `seeksv getsv -F` - junctions from read-through split alignments (FindJunction, process_bwasw.cpp:5-227): selection, pairing by read
name and the junction of every pair on the GPU (ssv_rt_*), the pairs applied to the junction map on the host.  Against what the real reference
writes for the same seeded inputs (tests/golden/readthrough/, tests/golden/make_readthrough_reference.py)."""
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import bamio
import readthrough_inputs as RT
import test_random_cli_vs_reference_gpu as RC
from seeksv_amd import _abi, host
from seeksv_amd.device import Context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")


@pytest.fixture(autouse=True, params=["host-inflate", "device-inflate"])
def inflate_mode(request, monkeypatch):
    """every test runs twice: the -F file (and the original BAM) inflated + decoded by the host threads, and on the GPU with 1 MB chunks"""
    if request.param == "device-inflate":
        monkeypatch.setenv("SSV_DEVICE_INFLATE", "1")
        monkeypatch.setenv("SSV_CHUNK_INFLATED_MB", "1")
        monkeypatch.setenv("SSV_STAGE_MB", "1")
    else:
        monkeypatch.delenv("SSV_DEVICE_INFLATE", raising=False)
    return request.param


def want(name):
    with open(os.path.join(RT.GOLDEN, "readthrough", name + ".json")) as f:
        return json.load(f)


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


@pytest.fixture(scope="module")
def small_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("rt_small")
    fbam = str(d / "small.bam")
    RT.write_f_bam(fbam, RT.small_records())
    clip_bam, clip = RT.empty_clip_inputs(str(d))
    bfile = str(d / "b.txt")
    with open(bfile, "w") as f:
        f.write(RT.b_rows())
    return fbam, clip_bam, clip, bfile


def getsv(args, env=None):
    return subprocess.run([SEEKSV, "getsv"] + args, capture_output=True, text=True, env=env)


def check_stderr(stderr, ref_lines):
    """the reference's stderr lines that this build prints too come in the reference's order, and its phase markers are all there"""
    ours = [RT.unpath(l) for l in stderr.splitlines()]
    assert [l for l in ours if l in set(ref_lines)] == [l for l in ref_lines if l in set(ours)]
    for marker in ("[ReadBreakpoint] finish", "'FindJunction' finished", "'InputSoftInfoStoreBreakpoint' finished"):
        assert (marker in ref_lines) == (marker in ours), marker


@pytest.mark.parametrize("tag,flags", RT.SMALL_RUNS, ids=[t for t, _ in RT.SMALL_RUNS])
def test_getsv_F_small_equals_reference(tmp_path, small_inputs, tag, flags):
    """every construction case, the hold / pair / drop machine, each filter rule under -w 0 / 1 / 20, 3'-branch records without S, the counting
    rule, a junction that is also a -B row: the .sv table and stdout byte for byte"""
    fbam, clip_bam, clip, bfile = small_inputs
    w = want("small")[tag]
    sv = str(tmp_path / "o.sv")
    r = getsv(RT.flags_with(flags, bfile) + ["-F", fbam, clip_bam, RT.BG, clip, sv, str(tmp_path / "x.fq")])
    assert r.returncode == 0, r.stderr
    assert open(sv).read() == w["sv"]
    assert r.stdout == w["stdout"]
    check_stderr(r.stderr, w["stderr_lines"])


@pytest.mark.parametrize("seed", RT.RANDOM_SEEDS)
def test_getsv_F_random_equals_reference(tmp_path, seed):
    """a few thousand random split alignments beside a clip join (clip.gz x clip.bam) and MergeJunction: digests of the reference's outputs"""
    bg, clip_bam, clip_gz = RC.make_inputs(seed, str(tmp_path))
    fbam = str(tmp_path / "f.bam")
    RT.write_f_bam(fbam, RT.random_records(seed))
    w = want("random")[str(seed)]
    for tag, flags in RT.RANDOM_RUNS:
        sv = str(tmp_path / f"o.{tag}.sv")
        r = getsv(flags + ["-F", fbam, clip_bam, bg, clip_gz, sv, str(tmp_path / "x.fq")])
        assert r.returncode == 0, r.stderr
        text = open(sv).read()
        assert text.count("\n") == w[tag]["sv_lines"], tag
        assert sha(text) == w[tag]["sv"], tag
        assert sha(r.stdout) == w[tag]["stdout"], tag


@pytest.fixture(scope="module")
def large_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("rt_large")
    fbam = str(d / "large.bam")
    recs = RT.random_records(RT.LARGE_SEED, n_names=RT.LARGE_NAMES)
    RT.write_f_bam(fbam, recs)
    clip_bam, clip = RT.empty_clip_inputs(str(d))
    return fbam, clip_bam, clip, RT.contig_changes(recs)


@pytest.mark.parametrize("cuts", ["coarse", "fine"])
def test_getsv_F_large_file_in_read_order(tmp_path, large_inputs, inflate_mode, cuts):
    """~137 k split alignments in read order (89 k contig changes), as bwasw writes them: host reader in one batch or in 5000-record batches
    (read-ahead: the names of three batch sets in turn); -Z in one 64 MB chunk (more than 65536 contig changes in it: a coordinate-sorted file's limit
    that -F lifts) or in 1 MB chunks (records carried over chunk seams, their names inside the next chunk's stream) - all equal the reference's output"""
    fbam, clip_bam, clip, changes = large_inputs
    w = want("large")
    assert changes == w["contig_changes"] and changes > 65536
    env = dict(os.environ)
    if inflate_mode == "host-inflate" and cuts == "fine":
        env["SSV_HOST_BATCH_RECORDS"] = "5000"
    if inflate_mode == "device-inflate" and cuts == "coarse":
        env.update(SSV_CHUNK_INFLATED_MB="64", SSV_STAGE_MB="64")
    sv = str(tmp_path / "o.sv")
    r = getsv(RT.LOOSE + ["-F", fbam, clip_bam, RT.BG, clip, sv, str(tmp_path / "x.fq")], env=env)
    assert r.returncode == 0, r.stderr
    text = open(sv).read()
    assert text.count("\n") == w["sv_lines"]
    assert sha(text) == w["sv"]
    assert sha(r.stdout) == w["stdout"]


def test_getsv_F_hash_collisions(tmp_path, small_inputs):
    """SSV_RT_HASH_BITS=4: read names collide in 16 hash values, so every run of equal hashes holds many names - the pairing compares full names"""
    fbam, clip_bam, clip, bfile = small_inputs
    env = dict(os.environ, SSV_RT_HASH_BITS="4")
    for tag, flags in RT.SMALL_RUNS[:3]:
        sv = str(tmp_path / f"o.{tag}.sv")
        r = getsv(RT.flags_with(flags, bfile) + ["-F", fbam, clip_bam, RT.BG, clip, sv, str(tmp_path / "x.fq")], env=env)
        assert r.returncode == 0, r.stderr
        assert open(sv).read() == want("small")[tag]["sv"], tag
    bg, cb, cg = RC.make_inputs(3, str(tmp_path))
    f3 = str(tmp_path / "f3.bam")
    RT.write_f_bam(f3, RT.random_records(3))
    sv = str(tmp_path / "r3.sv")
    r = getsv(RT.LOOSE + ["-F", f3, cb, bg, cg, sv, str(tmp_path / "x.fq")], env=env)
    assert r.returncode == 0, r.stderr
    assert sha(open(sv).read()) == want("random")["3"]["loose"]["sv"]


def _file_batch(path):
    """the whole file as one host batch with every record's bases, and its read names"""
    with host.BamReader(path) as rd:
        b = rd.read_batch(1 << 22, keep_all_seq=True)
        names = rd.target_names
    _, recs = bamio.read_bam_records(path)
    return b, [r["qname"] for r in recs], names


def _cut(b, a, e):
    n = len(b["tid"])
    out = {k: (v[a:e] if isinstance(v, np.ndarray) and k not in ("cigar", "seqqual") and len(v) == n else v) for k, v in b.items() if k != "tid_runs"}
    return out


def _readthrough(ctx, b, qn, names, cuts, min_mapq=1):
    bounds = [0] + list(cuts) + [len(qn)]
    bs = [_cut(b, bounds[k], bounds[k + 1]) for k in range(len(bounds) - 1) if bounds[k + 1] > bounds[k]]
    ns = [qn[bounds[k]:bounds[k + 1]] for k in range(len(bounds) - 1) if bounds[k + 1] > bounds[k]]
    return ctx.readthrough(bs, ns, min_mapq=min_mapq, target_names=names)


def test_readthrough_abi_batch_cuts(tmp_path, inflate_mode):
    """Context.readthrough: the pairs - junction, seqs, CIGAR sources - do not depend on where the batches are cut: one batch, one record per
    batch, random cuts, and a cut between the two records of every name of the small file (its second records follow all first ones)"""
    if inflate_mode != "host-inflate":
        pytest.skip("the ABI is driven with host batches here")
    fbam = str(tmp_path / "small.bam")
    recs = RT.small_records()
    RT.write_f_bam(fbam, recs)
    b, qn, names = _file_batch(fbam)
    n = len(qn)
    with Context(0) as ctx:
        whole, n_cand = ctx.readthrough([b], [qn], target_names=names, raw=True)
        assert len(whole) > 20 and n_cand > len(whole)
        assert whole == _readthrough(ctx, b, qn, names, range(1, n))
        assert whole == _readthrough(ctx, b, qn, names, [n // 2])  # (the interleaved file: first records, then second records)
        rng = np.random.RandomState(5)
        for _ in range(3):
            assert whole == _readthrough(ctx, b, qn, names, sorted(set(rng.randint(1, n, 7).tolist())))
        for q in (0, 20):
            assert _readthrough(ctx, b, qn, names, [], q) == _readthrough(ctx, b, qn, names, range(3, n, 3), q)
        # the random files: thousands of records, names up to 4 times
        f0 = str(tmp_path / "r0.bam")
        RT.write_f_bam(f0, RT.random_records(0))
        b0, q0, n0 = _file_batch(f0)
        w0 = ctx.readthrough([b0], [q0], target_names=n0)
        assert len(w0) > 500
        assert w0 == _readthrough(ctx, b0, q0, n0, range(1, len(q0), 1))
        assert w0 == _readthrough(ctx, b0, q0, n0, range(97, len(q0), 97))
    by = {p["key"]: p for p in whole}
    ss = by[("chrA", 1040, "+", "chrA", 5001, "+")]       # ss_mh: up = the 3'-clipped record at 1000 (70M), microhomology 30
    assert ss["microhomology"] == 30 and ss["kind"] == 0 and len(ss["up_seq"]) == 40 and len(ss["down_seq"]) == 60 and ss["edits"] == (1, 0)


def test_readthrough_abi_sequence_and_arguments():
    """calls out of sequence return SSV_E_STATE; bad arguments SSV_E_ARG"""
    lib = _abi.hip_lib()
    with Context(0) as ctx:
        b, keep = _abi.make_batch({k: np.zeros(0, dt) for k, dt in _abi.BATCH_FIELDS})
        nm = _abi.Names(_abi.MEM_HOST, 0, 0, None, None, 0)
        res = _abi.RtResult()
        assert lib.ssv_rt_scan(ctx._h, C.byref(b), C.byref(nm)) == -4
        assert lib.ssv_rt_finish(ctx._h, C.byref(res)) == -4
        rank = np.zeros(1, np.int32)
        p = _abi.RtParams(1, 1, rank.ctypes.data_as(C.POINTER(C.c_int32)))
        assert lib.ssv_rt_begin(ctx._h, None) == -3
        assert lib.ssv_rt_begin(ctx._h, C.byref(p)) == 0
        assert lib.ssv_rt_scan(ctx._h, None, C.byref(nm)) == -3
        assert lib.ssv_rt_scan(ctx._h, C.byref(b), C.byref(nm)) == 0
        assert lib.ssv_rt_finish(ctx._h, C.byref(res)) == 0 and res.n_pairs == 0
        assert lib.ssv_rt_finish(ctx._h, C.byref(res)) == -4
        assert lib.ssv_rt_scan(ctx._h, C.byref(b), C.byref(nm)) == -4


def test_getsv_F_refuses_non_bam(tmp_path, small_inputs):
    """a -F file that is not BAM: the reference's message, exit status 1 (SAM text input is not read by this build)"""
    fbam, clip_bam, clip, bfile = small_inputs
    for name, data in (("x.sam", "@HD\tVN:1.0\n"), ("y.bam", "not a bam file\n")):
        p = str(tmp_path / name)
        with open(p, "w") as f:
            f.write(data)
        r = getsv(["-F", p, clip_bam, RT.BG, clip, str(tmp_path / "o.sv"), str(tmp_path / "x.fq")])
        assert r.returncode == 1
        assert "[main_samview] fail to open file for reading." in r.stderr


def test_getsv_F_ranks_equal_single(tmp_path, small_inputs):
    """getsv -N 2 -F: the -F pass runs once, on the first device; the output equals -N 1 (the two ranks share this GPU)"""
    fbam, clip_bam, clip, bfile = small_inputs
    outs = []
    for n in (1, 2):
        sv = str(tmp_path / f"o{n}.sv")
        r = getsv(["-N", str(n)] + RT.LOOSE + ["-F", fbam, clip_bam, RT.BG, clip, sv, str(tmp_path / "x.fq")])
        assert r.returncode == 0, r.stderr
        outs.append((open(sv).read(), r.stdout))
    assert outs[0] == outs[1]
    assert outs[0][0] == want("small")["loose"]["sv"]


def test_run_passes_F_to_getsv(tmp_path, inflate_mode):
    """`seeksv run -v "-F f.bam ..."` writes what getclip, realign and getsv -F write one after the other"""
    if inflate_mode != "device-inflate":
        pytest.skip("`seeksv run` always decodes on the GPU")
    from seeksv_amd import synth
    w = synth.Workload(genome_frac=1 / 8192, depth=20, n_sv=8)
    bam = str(tmp_path / "s.bam")
    bamio.soa_to_bam(bam, w.names, w.lens, w.generate_host(0, w.n_total))
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        f.write(w.reference_fasta())
    fbam = str(tmp_path / "f.bam")
    RT.write_f_bam(fbam, RT.random_records(11, n_names=800, lens=w.lens), names=w.names, lens=w.lens)
    sv_o = ["-F", fbam, "-w", "0"] + RT.LOOSE
    a = str(tmp_path / "three")
    for args in (["getclip", "-o", a, bam], ["realign", fa, a + ".clip.fq.gz", a + ".clip.bam"],
                 ["getsv"] + sv_o + [a + ".clip.bam", bam, a + ".clip.gz", a + ".sv.txt", a + ".unmapped.clip.fq"]):
        r3 = subprocess.run([SEEKSV] + args, capture_output=True, text=True)
        assert r3.returncode == 0, r3.stderr
    b = str(tmp_path / "one")
    r = subprocess.run([SEEKSV, "run", "-v", " ".join(sv_o), bam, fa, b], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for ext in (".sv.txt", ".unmapped.clip.fq"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert gzip.open(a + ".clip.gz", "rb").read() == gzip.open(b + ".clip.gz", "rb").read()
    assert r.stdout == r3.stdout
    assert "'FindJunction' finished" in r.stderr
    assert len([l for l in open(b + ".sv.txt") if not l.startswith("@")]) > 0
