"""-m gpu: the gapped re-aligner (k_ra_gap behind the query kernel with its candidate floor at 20; ssv_realign_query_gapped; `seeksv realign -g`;
`seeksv run -a "-g"`) against the model of tests/realign_gapped_model.py: every field of every hit and both fields of every gap, none exempt, on
the hash index and on the sorted one.  Inputs: tests/realign_gapped_inputs.py (held to their properties on the CPU in
tests/test_realign_gapped_inputs.py) and tests/realign_inputs.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bamio
import golden_util as G
import realign_gapped_inputs as GI
import realign_gapped_model as GM
import realign_inputs as I
import realign_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
E_ARG, E_STATE = -3, -4
KEYS = M.FIELDS + ("flags",) + GM.GAP_FIELDS
CAP = 500


@pytest.fixture(scope="module")
def ctx():
    from seeksv_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def index(ctx, contigs, max_occ=None):
    words, off = M.pack_2bit(contigs)
    return ctx.realign_index(words, off) if max_occ is None else ctx.realign_index_sorted(words, off, max_occ)


@functools.lru_cache(maxsize=None)
def model():
    return M.Reference(GI.reference())


@functools.lru_cache(maxsize=None)
def expected(max_occ):
    """the model's hits of GI.all_queries(), computed once per kind of index"""
    return tuple(GM.align_gapped(model(), q, max_occ) for q in GI.all_queries()[0])


def as_dict(h, g):
    return dict({k: int(h[k]) for k in M.FIELDS}, flags=int(h["pad"][0]), gap_at=int(g["q_at"]), gap_len=int(g["len"]))


def compare(hits, gaps, want, labels, skip=()):
    assert len(hits) == len(gaps) == len(want)
    bad = []
    for i, (h, g, w) in enumerate(zip(hits, gaps, want)):
        if i in skip:
            continue
        got = as_dict(h, g)
        assert int(h["pad"][1]) == 0
        diff = {k: (got[k], w[k]) for k in KEYS if got[k] != w[k]}
        if diff:
            bad.append((labels[i], diff))
    for b in bad:
        print("kernel / model:", b)
    assert not bad, f"{len(bad)} of {len(want)} queries differ, (kernel, model): {bad[:8]}"


def test_error_codes_come_first():
    """(before the shared context has an index) the gapped query's error returns are the plain query's"""
    from seeksv_amd import _abi
    from seeksv_amd.device import Context
    words, off = M.pack_2bit(GI.reference())
    with Context(0) as c:
        lib = c._lib
        hits = np.zeros(1, dtype=np.dtype(_abi.REALIGN_HIT))
        gaps = np.zeros(1, dtype=np.dtype(_abi.REALIGN_GAP))
        qoff = np.array([0, 4], np.uint64)
        seq = C.c_char_p(b"ACGT")
        assert lib.ssv_realign_query_gapped(c._h, seq, qoff.ctypes.data, 1, hits.ctypes.data, gaps.ctypes.data) == E_STATE
        assert lib.ssv_realign_query_gapped(None, seq, qoff.ctypes.data, 1, hits.ctypes.data, gaps.ctypes.data) == E_ARG
        assert lib.ssv_realign_index(c._h, words.ctypes.data, 0, int(off[-1]), off.ctypes.data, len(off) - 1, None) == 0
        assert lib.ssv_realign_query_gapped(c._h, seq, qoff.ctypes.data, -1, hits.ctypes.data, gaps.ctypes.data) == E_ARG
        assert lib.ssv_realign_query_gapped(c._h, None, qoff.ctypes.data, 1, hits.ctypes.data, gaps.ctypes.data) == E_ARG
        assert lib.ssv_realign_query_gapped(c._h, seq, None, 1, hits.ctypes.data, gaps.ctypes.data) == E_ARG
        assert lib.ssv_realign_query_gapped(c._h, seq, qoff.ctypes.data, 1, None, gaps.ctypes.data) == E_ARG
        assert lib.ssv_realign_query_gapped(c._h, seq, qoff.ctypes.data, 1, hits.ctypes.data, None) == E_ARG
        assert lib.ssv_realign_query_gapped(c._h, None, None, 0, None, None) == 0
        assert lib.ssv_realign_query_gapped(c._h, seq, qoff.ctypes.data, 1, hits.ctypes.data, gaps.ctypes.data) == 0
        assert int(hits["tid"][0]) == -1 and int(gaps["len"][0]) == 0
        assert lib.ssv_realign_free(c._h) == 0
        assert lib.ssv_realign_query_gapped(c._h, seq, qoff.ctypes.data, 1, hits.ctypes.data, gaps.ctypes.data) == E_STATE
        assert c.realign([], gapped=True)[1].shape == (0,)


@pytest.mark.parametrize("max_occ", [None, CAP], ids=["hash", "sorted"])
def test_every_field_of_every_query(ctx, max_occ):
    """the acceptance condition: all fields, the flags and the gap of every query of every set; and no query scores less than without gaps"""
    queries, labels = GI.all_queries()
    index(ctx, GI.reference(), max_occ)
    hits, gaps = ctx.realign(list(queries), gapped=True)
    compare(hits, gaps, expected(max_occ), labels)
    plain = ctx.realign(list(queries))
    assert (hits["score"] >= plain["score"]).all()
    same = gaps["len"] == 0
    aligned = plain["tid"] >= 0
    assert (hits[same & aligned] == plain[same & aligned]).all()   # no gap: the ungapped hit, untouched
    assert (gaps["len"] != 0).sum() > 300 and (hits["tid"][~aligned] >= 0).sum() >= 24   # (the rescue set)


def test_random_set_gapped(ctx):
    """the hash index's differential set (substitutions, junk bytes, unrelated heads and tails, contig boundaries, the length limits; no planted gap):
    the gapped query against the model wherever the plain model determines the first stage, and never below the ungapped score"""
    contigs, queries = I.random_set("odd")
    ref = M.Reference(contigs)
    index(ctx, contigs)
    hits, gaps = ctx.realign(list(queries), gapped=True)
    want = [GM.align_gapped(ref, q) for q in queries]
    skip = {i for i, w in enumerate(want) if w["overflow"] or w["tie"]}
    assert len(skip) <= 4
    compare(hits, gaps, want, list(range(len(queries))), skip)
    plain = ctx.realign(list(queries))
    keep = np.array([i not in skip for i in range(len(queries))])
    assert (hits["score"] >= plain["score"])[keep].all()


def write_inputs(tmp_path, names, contigs, fq):
    fa, fq_path = str(tmp_path / "ref.fa"), str(tmp_path / "s.clip.fq")
    with open(fa, "w") as f:
        for name, c in zip(names, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 60] for i in range(0, len(c), 60)) + "\n")
    with open(fq_path, "w") as f:
        for i, (s, q) in enumerate(fq):
            f.write(f"@clip{i}\n{s}\n+\n{q}\n")
    return fa, fq_path


@pytest.mark.parametrize("opts", [["-g"], ["-c", str(CAP), "-g"]], ids=["hash", "sorted"])
def test_cli_realign_g(tmp_path, opts):
    """`seeksv realign -g`: every record is the model's bam_record (M, D / I, M between the soft clips, in reference order on either strand), the
    closing line counts the records with a gap; without -g the same input has no I and no D and the closing line is the one it was"""
    fq = GI.cli_set()
    by_query = dict(zip(GI.all_queries()[0], expected(CAP if "-c" in opts else None)))
    fa, fq_path = write_inputs(tmp_path, GI.NAMES, GI.reference(), fq)
    out = str(tmp_path / "g.clip.bam")
    r = subprocess.run([SEEKSV, "realign"] + opts + [fa, fq_path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names, recs = bamio.read_bam_records(out)
    assert names == GI.NAMES and len(recs) == len(fq)
    n_gap = n_al = 0
    for (s, q), rec in zip(fq, recs):
        e = GM.bam_record(s, q, by_query[s])
        assert rec["qname"] == s and rec["l_qseq"] == len(s)
        assert (rec["flag"], rec["tid"], rec["pos"], rec["mapq"], rec["cigar"]) == (e["flag"], e["tid"], e["pos"], e["mapq"], e["cigar"]), (s, rec, e)
        n_gap += any(op in "ID" for _, op in e["cigar"])
        n_al += e["tid"] >= 0
    assert n_gap > 250
    assert f"[seeksv realign] {len(fq)} clipped sequences, {n_al} aligned, {n_gap} with a gap" in r.stderr.splitlines()
    plain = str(tmp_path / "p.clip.bam")
    r = subprocess.run([SEEKSV, "realign"] + [o for o in opts if o != "-g"] + [fa, fq_path, plain], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, precs = bamio.read_bam_records(plain)
    assert len(precs) == len(fq) and not any(op in "ID" for rec in precs for _, op in rec["cigar"])
    ref = model()
    n_plain = sum(M.align(ref, s)["tid"] >= 0 for s, _ in fq)
    assert f"[seeksv realign] {len(fq)} clipped sequences, {n_plain} aligned" in r.stderr.splitlines()
    assert "-g " in subprocess.run([SEEKSV, "realign"], capture_output=True, text=True).stderr


def sv_rows(path):
    return [l.split("\t") for l in open(path).read().splitlines() if not l.startswith("@")]


def test_cli_run_g_places_the_junction(tmp_path):
    """`seeksv run -a "-g"` on the sample whose clips cross a 3-base deletion 26 bases behind the breakpoint: the SV table is the one the real
    reference's getsv makes from the model's gapped records (tests/golden/realign_gapped); without -g the planted row is not in the table"""
    contigs, recs = GI.e2e_sample()
    bam, fa = str(tmp_path / "s.bam"), str(tmp_path / "ref.fa")
    bamio.write_bam(bam, list(GI.E2E_NAMES), list(GI.E2E_LENS), recs)
    with open(fa, "w") as f:
        for name, c in zip(GI.E2E_NAMES, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 70] for i in range(0, len(c), 70)) + "\n")
    planted = ("tA", str(GI.E2E_A + 1), "tB", str(GI.E2E_B + 1))
    for tag, aln in (("gap", ["-a", "-g"]), ("gapc", ["-a", f"-c {CAP} -g"]), ("plain", [])):
        pre = str(tmp_path / tag)
        r = subprocess.run([SEEKSV, "run", "-v", " ".join(GI.E2E_SV_OPTS)] + aln + [bam, fa, pre], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        rows = sv_rows(pre + ".sv.txt")
        if aln:
            assert open(pre + ".sv.txt").read() == G.read_text("realign_gapped", "e2e.sv")
            assert r.stdout == G.read_text("realign_gapped", "e2e.stdout")
            assert [(x[0], x[1], x[4], x[5]) for x in rows] == [planted]
            assert any(l.startswith("[seeksv realign]") and l.endswith(" with a gap") for l in r.stderr.splitlines())
        else:
            assert planted not in [(x[0], x[1], x[4], x[5]) for x in rows]
            assert not any("with a gap" in l for l in r.stderr.splitlines())
