"""-m gpu: the re-aligner's sorted index (k_ras_*, ssv_realign_index_sorted, `seeksv realign -c`, `seeksv run -a`) against the model of
tests/realign_sorted_model.py: the index statistics, and every field and the flags of EVERY query - part repeat, part unique; wholly repeat; masked;
over the candidate limit - with no class of queries left to "whatever was kept".  Where no repeat is in play it returns the hash index's hits.
Inputs: tests/realign_sorted_inputs.py (held against the model alone in tests/test_realign_sorted_model.py) and tests/realign_inputs.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bamio
import golden_util as G
import realign_inputs as I
import realign_model as M
import realign_sorted_inputs as SI
import realign_sorted_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
MEMS = ["host", "device"]
E_ARG, E_STATE = -3, -4
KEYS = M.FIELDS + ("flags",)


@pytest.fixture(scope="module")
def ctx():
    from seeksv_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def packed(contigs):
    return M.pack_2bit(contigs)


def index(ctx, contigs, mem, max_occ=None):
    """max_occ None: the hash index.  -> (dropped or the statistics, what has to stay alive while the index is used)"""
    from seeksv_amd import _abi
    words, off = packed(tuple(contigs))
    build = ctx.realign_index if max_occ is None else lambda w, o, **kw: ctx.realign_index_sorted(w, o, max_occ, **kw)
    if mem == "host":
        return build(words, off), None
    import torch
    t = torch.from_numpy(words.view(np.int64)).to("cuda:0")   # the slack word is the array's last
    torch.cuda.synchronize()
    return build(t.data_ptr(), off, mem=_abi.MEM_DEVICE), t


def as_dict(h):
    return dict({k: int(h[k]) for k in M.FIELDS}, flags=int(h["pad"][0]))


def test_error_codes_come_first():
    """(before the shared context has an index) a query without an index, a cap outside 1..65535"""
    from seeksv_amd import _abi
    from seeksv_amd.device import Context
    assert (_abi.RA_F_MASKED, _abi.RA_F_OVERFLOW) == (SM.F_MASKED, SM.F_OVERFLOW)
    words, off = packed(SI.repeat_reference()[1])
    with Context(0) as c:
        lib = c._lib
        hits = np.zeros(1, dtype=np.dtype(_abi.REALIGN_HIT))
        qoff = np.array([0, 4], np.uint64)
        assert lib.ssv_realign_query(c._h, C.c_char_p(b"ACGT"), qoff.ctypes.data, 1, hits.ctypes.data) == E_STATE
        for bad in (0, -1, 65536, 1 << 20):
            assert lib.ssv_realign_index_sorted(c._h, words.ctypes.data, 0, int(off[-1]), off.ctypes.data, len(off) - 1, bad, None) == E_ARG
        assert lib.ssv_realign_query(c._h, C.c_char_p(b"ACGT"), qoff.ctypes.data, 1, hits.ctypes.data) == E_STATE   # a refused build leaves no index
        assert lib.ssv_realign_index_sorted(c._h, words.ctypes.data, 0, int(off[-1]) - 1, off.ctypes.data, len(off) - 1, 500, None) == E_ARG
        assert lib.ssv_realign_index_sorted(c._h, words.ctypes.data, 0, int(off[-1]), off.ctypes.data, len(off) - 1, 65535, None) == 0   # stats may be NULL
        assert lib.ssv_realign_free(c._h) == 0
        assert lib.ssv_realign_query(c._h, C.c_char_p(b"ACGT"), qoff.ctypes.data, 1, hits.ctypes.data) == E_STATE


@pytest.mark.parametrize("mem", MEMS)
def test_index_statistics(ctx, mem):
    contigs = SI.repeat_reference()[1]
    ref = SI.repeat_model()
    for cap in SI.CAPS:
        st, keep = index(ctx, contigs, mem, cap)
        del keep
        assert st == SM.index_stats(ref, cap), cap
    for shape in I.SHAPES:   # contigs shorter than a seed, offsets that are no multiples of 4 or 32, a full / a one-base last word
        c = I.shape_reference(shape)
        st, keep = index(ctx, c, mem, 500)
        del keep
        assert st == SM.index_stats(M.Reference(c), 500), shape


def compare(ctx, queries, want, labels):
    hits = ctx.realign(list(queries))
    bad = []
    for i, (h, w) in enumerate(zip(hits, want)):
        got = as_dict(h)
        assert int(h["pad"][1]) == 0
        diff = {k: (got[k], w[k]) for k in KEYS if got[k] != w[k]}
        if diff:
            bad.append((labels[i], len(queries[i]), diff))
    for b in bad:
        print("kernel / model:", b)
    assert not bad, f"{len(bad)} of {len(queries)} queries differ, (kernel, model): {bad[:8]}"
    return hits


@pytest.mark.parametrize("mem,cap", [("host", 500), ("device", 500), ("host", 299), ("host", 300), ("device", 65535), ("host", 1)])
def test_every_query_of_the_repeat_reference(ctx, mem, cap):
    """the acceptance condition: all fields and the flags of every query, no exemption.  cap 500: the element (300 copies) is seeded, poly-A masked;
    299: the element is masked too; 300 = 500; 65535: poly-A is seeded; 1: only unique 20-mers seed"""
    contigs = SI.repeat_reference()[1]
    queries, labels = SI.repeat_queries()
    _, keep = index(ctx, contigs, mem, cap)
    hits = compare(ctx, queries, SI.repeat_expected(cap), labels)
    del keep
    if cap == 500:
        for lab in ("E36+spacer24", "spacer24+E36"):   # the case the admission rule exists for: placed at copy 250 of 300
            for strand in ("fwd", "rev"):
                h = hits[labels.index(f"{lab}/{strand}")]
                assert (int(h["tid"]), int(h["score"]), int(h["mapq"])) == (SI.NAMES.index("E"), 60, 60)
                assert SI.e_copy_start(SI.E_COPY) <= int(h["pos"]) < SI.e_copy_start(SI.E_COPY + 1)


SETS = {"random-even": lambda: I.random_set("even"), "random-odd": lambda: I.random_set("odd"), "threshold-even": lambda: I.threshold_set("even"),
        "threshold-odd": lambda: I.threshold_set("odd"), "two-locus": I.two_locus_set, "sweep": I.sweep_set, "tandem": I.tandem_set}


@pytest.mark.parametrize("name", list(SETS))
def test_equals_the_hash_index_without_repeats(ctx, name):
    """the sets of the hash index's differential tests: at cap 500 the sorted index returns the hash index's hits (same context, one index after
    the other) wherever the plain model determines them - and the sorted model's hits everywhere"""
    s = SETS[name]()
    contigs, queries = s[0], s[1]
    labels = s[2] if len(s) > 2 else list(range(len(queries)))
    ref = M.Reference(contigs)
    dropped, _ = index(ctx, contigs, "host")
    assert dropped == 0
    by_hash = ctx.realign(list(queries))
    st, _ = index(ctx, contigs, "host", 500)
    assert st["n_indexed"] == ref.n_sampled and st["n_over_cap"] == 0
    by_sorted = compare(ctx, queries, [SM.align_sorted(ref, q, 500) for q in queries], labels)
    n = 0
    for q, a, b in zip(queries, by_hash, by_sorted):
        w = M.align(ref, q)
        if w["overflow"] or w["tie"]:
            continue
        assert {k: int(a[k]) for k in M.FIELDS} == {k: int(b[k]) for k in M.FIELDS}, q
        assert int(a["pad"][0]) == 0
        n += 1
    assert n >= len(queries) - 4


def test_index_kinds_alternate_on_one_context(ctx):
    """hash (a random reference), sorted (the repeat reference), hash, sorted on one context: building one kind replaces the other, the hits of each
    kind are the same every time, and the hash index writes no flags"""
    rc, rq = I.random_set("odd")
    sc, (sq, _) = SI.repeat_reference()[1], SI.repeat_queries()
    rref = M.Reference(rc)
    settled = [i for i, q in enumerate(rq) if not M.align(rref, q)["overflow"]]   # (what the hash index kept of more than 192 seeds is a race)
    seen = {}
    for kind in ("hash", "sorted", "hash", "sorted"):
        if kind == "hash":
            assert index(ctx, rc, "host")[0] == 0
            hits = ctx.realign(list(rq))[settled]
            assert not hits["pad"].any() and (hits["tid"] >= 0).sum() >= 500
        else:
            index(ctx, sc, "host", 500)
            hits = ctx.realign(list(sq))
            assert hits["pad"][:, 0].any()
        if kind in seen:
            assert (hits == seen[kind]).all(), kind
        seen[kind] = hits


def write_inputs(tmp_path, names, contigs, fq):
    fa, fq_path = str(tmp_path / "ref.fa"), str(tmp_path / "s.clip.fq")
    with open(fa, "w") as f:
        for name, c in zip(names, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 60] for i in range(0, len(c), 60)) + "\n")
    with open(fq_path, "w") as f:
        for i, (s, q) in enumerate(fq):
            f.write(f"@clip{i}\n{s}\n+\n{q}\n")
    return fa, fq_path


def records(path):
    names, recs = bamio.read_bam_records(path)
    return names, [(r["qname"], r["flag"], r["tid"], r["pos"], r["mapq"], r["cigar"], r["l_qseq"]) for r in recs]


def test_cli_realign_c_equals_realign_without_repeats(tmp_path):
    """`seeksv realign -c 500` on the hash index's end-to-end set: the records `seeksv realign` writes; nothing masked, nothing over the limit"""
    names, contigs, fq = I.cli_set()
    fa, fq_path = write_inputs(tmp_path, names, contigs, fq)
    a, b = str(tmp_path / "hash.bam"), str(tmp_path / "sorted.bam")
    r1 = subprocess.run([SEEKSV, "realign", fa, fq_path, a], capture_output=True, text=True)
    assert r1.returncode == 0, r1.stderr
    r2 = subprocess.run([SEEKSV, "realign", "-c", "500", fa, fq_path, b], capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr
    assert records(a) == records(b) and len(records(a)[1]) == len(fq)
    assert open(a, "rb").read() == open(b, "rb").read()
    line = [l for l in r2.stderr.splitlines() if l.startswith("[seeksv realign]")]
    assert line == [l for l in r1.stderr.splitlines() if l.startswith("[seeksv realign]")] and len(line) == 1 and line[0].endswith(" aligned")
    for bad in ("0", "65536", "x", "-3", "12x"):
        r = subprocess.run([SEEKSV, "realign", "-c", bad, fa, fq_path, b], capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("Usage: seeksv realign") and "-c <int>" in r.stderr, bad


def test_cli_realign_c_on_the_repeat_reference(tmp_path):
    """the repeat reference as a FASTA: every record is what the model's hit implies, and the closing line counts the masked and the over-limit queries"""
    names, contigs = SI.repeat_reference()
    queries, labels = SI.repeat_queries()
    keep = [i for i, q in enumerate(queries) if 0 < len(q) <= 254]   # (the read name is the sequence: 254 characters at most)
    rng = np.random.RandomState(7)
    fq = [(queries[i], "".join(chr(33 + int(x)) for x in rng.randint(2, 41, len(queries[i])))) for i in keep]
    want = [SI.repeat_expected(500)[i] for i in keep]
    fa, fq_path = write_inputs(tmp_path, names, contigs, fq)
    out = str(tmp_path / "s.clip.bam")
    r = subprocess.run([SEEKSV, "realign", "-c", "500", fa, fq_path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got_names, recs = bamio.read_bam_records(out)
    assert got_names == list(names) and len(recs) == len(fq)
    for (s, q), w, rec, i in zip(fq, want, recs, keep):
        e = M.bam_record(s, q, w)
        assert rec["qname"] == s and rec["l_qseq"] == len(s)
        assert (rec["flag"], rec["tid"], rec["pos"], rec["mapq"], rec["cigar"]) == (e["flag"], e["tid"], e["pos"], e["mapq"], e["cigar"]), (labels[i], rec, e)
    n_al = sum(w["tid"] >= 0 for w in want)
    n_masked, n_over = sum(bool(w["flags"] & SM.F_MASKED) for w in want), sum(bool(w["flags"] & SM.F_OVERFLOW) for w in want)
    assert n_masked > 0 and n_over > 0
    assert f"[seeksv realign] {len(fq)} clipped sequences, {n_al} aligned, {n_masked} with repetitive seeds masked, {n_over} over the candidate limit" in r.stderr.splitlines()


def test_cli_run_a_reproduces_the_golden_table(tmp_path_factory):
    """`seeksv run -a "-c 500"` on the synthetic sample whose SV table and stdout are committed (made by the reference program from bwa mem's
    clip.bam; `seeksv run` reproduces them): the aligner thread builds the sorted index and the table and stdout are the committed ones"""
    import test_cli_gpu as TC
    from seeksv_amd import synth
    bam, _, d = TC._synth_sample(tmp_path_factory, "synthfull", TC.SYNTH_FULL["synthfull"])
    fa = str(d / "ref_sorted.fa")
    with open(fa, "w") as f:
        f.write(synth.Workload(**TC.SYNTH_FULL["synthfull"]).reference_fasta())
    pre = str(d / "sorted_run")
    r = subprocess.run([SEEKSV, "run", "-a", "-c 500", bam, fa, pre], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(pre + ".sv.txt").read() == G.read_text("synth", "synthfull.sv")
    assert r.stdout == G.read_text("synth", "synthfull.stdout")
    assert any(l.startswith("[seeksv realign]") and "dropped" not in l for l in r.stderr.splitlines())
    r = subprocess.run([SEEKSV, "run", "-a", "-c 0", bam, fa, pre], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Usage: seeksv realign")
