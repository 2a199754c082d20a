"""-m gpu: the `getsv -F` kernels (ssv_rt_begin / ssv_rt_scan / ssv_rt_finish) against the Python model of FindJunction
(tests/readthrough_model.py, anchored on the real reference's output by tests/test_readthrough_model.py), pair for pair: every field of every
ssv_rt_pair, the seqs, the CIGAR sources and the candidate count.  All comparisons are exact.  Inputs come from the model's generator
(random_rt_sample): every CIGAR shape the selection lets through, names from 1 to 254 bytes that come up to hundreds of times, reads of 0 to ~1500
bases, all sixteen base codes, tids outside the header, every MAPQ edge - far beyond what bwasw writes, and always inside the ABI's contract."""
import functools

import numpy as np
import pytest

import bamio
import oracle_lib as O
import readthrough_model as M
from seeksv_amd import device, host
from test_hip_golden import assert_tables_equal
from test_random_differential_gpu import random_sample

pytestmark = pytest.mark.gpu
SEEDS = tuple(range(48))
MAPQS = (0, 1, 20, 255)


@pytest.fixture(scope="module")
def ctx():
    c = device.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=8)
def sample(seed, **kw):
    return M.random_rt_sample(seed, **kw)


@functools.lru_cache(maxsize=64)
def _want_cached(seed, kw, min_mapq, n_contigs):
    s = sample(seed, **dict(kw))
    return M.find_junction([s["batch"]], [s["qnames"]], min_mapq, s["contigs"][:n_contigs])


def want_of(seed, min_mapq=1, n_contigs=None, **kw):
    """the model's (pairs, n_candidates) for a whole sample (where the batches are cut changes nothing: tests/test_readthrough_model.py)"""
    return _want_cached(seed, tuple(sorted(kw.items())), min_mapq, len(sample(seed, **kw)["contigs"]) if n_contigs is None else n_contigs)


def describe(s, rec):
    b = s["batch"]
    return (f"record {rec}: name {s['qnames'][rec][:40]!r} flag {int(b['flag'][rec])} mapq {int(b['mapq'][rec])} tid {int(b['tid'][rec])} pos {int(b['pos'][rec])} "
            f"l_qseq {int(b['l_qseq'][rec])} cigar {M.cigar_text([(l, M.OPS[op]) for l, op in M.record_ops(b, rec)])[:200]}")


def assert_equal(got, want, s, what=""):
    """(pairs, n_candidates) of the library == the model's; on a mismatch the first differing pair with its two records"""
    (gp, gn), (wp, wn) = got, want
    for k, (g, w) in enumerate(zip(gp, wp)):
        if g != w:
            fields = [f for f in w if g[f] != w[f]]
            recs = sorted(set(w["records"]) | set(g["records"]))
            lines = [f"{what}: pair {k} differs in {fields}", f"  library: { {f: g[f] for f in fields} }", f"  model:   { {f: w[f] for f in fields} }",
                     f"  model pair: kind {w['kind']} key {w['key']} microhomology {w['microhomology']}"] + ["  " + describe(s, r) for r in recs if r < len(s["qnames"])]
            pytest.fail("\n".join(lines))
    assert len(gp) == len(wp), f"{what}: {len(gp)} pairs, the model has {len(wp)}"
    assert gn == wn, f"{what}: {gn} candidates, the model has {wn}"


def run(ctx, s, cuts=(), min_mapq=1, contigs=None):
    batches, names = M.split(s, cuts)
    return ctx.readthrough(batches, names, min_mapq=min_mapq, target_names=s["contigs"] if contigs is None else contigs, raw=True)


def take(s, idx):
    """the records idx of a sample, in that order, as a sample of their own (the CIGAR and base pools stay whole)"""
    b, n = s["batch"], len(s["qnames"])
    idx = np.asarray(idx, dtype=np.int64)
    nb = {k: (v[idx] if isinstance(v, np.ndarray) and k not in ("cigar", "seqqual") and len(v) == n else v) for k, v in b.items()}
    return dict(s, batch=nb, qnames=[s["qnames"][i] for i in idx], records=[s["records"][i] for i in idx], cuts=[])


def model_of(s, min_mapq=1, contigs=None):
    return M.find_junction([s["batch"]], [s["qnames"]], min_mapq, s["contigs"] if contigs is None else contigs)


# ---- small things first: they say most about a wrong kernel in the least time ------------------------------------------------------------------
def test_pair_counts_of_zero_and_one_empty_batches_and_batches_without_candidates(ctx):
    s = sample(0)
    n, nt = len(s["qnames"]), len(s["contigs"])
    pairs, _ = want_of(0)
    kept = [i for i in range(n) if M.selected(s["batch"], i, 1, nt)]
    junk = [i for i in range(n) if not M.selected(s["batch"], i, 0, nt)]
    assert len(junk) > 20
    # one pair; no pair (the first kept record of every name); no candidate at all; no record at all
    one = take(s, sorted(pairs[3]["records"]))
    first, seen = [], set()
    for i in kept:
        if s["qnames"][i] not in seen:
            seen.add(s["qnames"][i])
            first.append(i)
    for t, n_pairs in ((one, 1), (take(s, first), 0), (take(s, junk), 0), (take(s, []), 0)):
        w = model_of(t)
        assert len(w[0]) == n_pairs
        assert_equal(run(ctx, t), w, t, f"{n_pairs} pair(s)")
    assert model_of(take(s, junk))[1] == 0 and model_of(take(s, first))[1] == len(first)
    # a batch with n == 0 in the middle, a batch without a candidate in the middle
    assert_equal(run(ctx, s, [1000, 1000, 2000]), want_of(0), s, "empty batch")
    mid = take(s, list(range(1000)) + junk + list(range(1000, n)))
    assert_equal(run(ctx, mid, [1000, 1000 + len(junk)]), model_of(mid), mid, "batch without a candidate")


def test_errors_leave_a_usable_context(ctx):
    """a kept record without bases: SSV_E_ARG from ssv_rt_scan, and the context serves the next file; fewer contigs than the batch's tids name"""
    s = sample(1)
    n, nt = len(s["qnames"]), len(s["contigs"])
    b = dict(s["batch"])
    k = [i for i in range(n) if M.selected(b, i, 1, nt) and int(b["l_qseq"][i]) > 0][5]
    so = b["seq_off"].copy()
    so[k] = M.NO_SEQ
    bad = dict(s, batch=dict(b, seq_off=so))
    with pytest.raises(device.SeeksvError, match=r"ssv_rt_scan failed \(-3\)"):
        run(ctx, bad)
    assert_equal(run(ctx, s), want_of(1), s, "after the error")
    with pytest.raises(device.SeeksvError, match=r"ssv_rt_scan failed \(-3\)"):
        run(ctx, bad, [k, k + 1])                      # ... in a batch of its own, after a good one
    assert_equal(run(ctx, s, s["cuts"]), want_of(1), s, "after the second error")
    # n_targets smaller than the largest tid: the records of the contigs beyond are no candidates
    for keep in (1, nt - 1):
        w = want_of(1, n_contigs=keep)
        assert w[1] < want_of(1)[1]
        assert_equal(run(ctx, s, contigs=s["contigs"][:keep]), w, s, f"{keep} contigs")


def test_long_cigars_and_long_reads(ctx):
    """every candidate has more than five operations (the cigar[] path behind the line's cigar_head[5]), many more than 64 (the second ballot round
    of the gather), some a single operation once S is dropped"""
    for seed in (0, 1):
        s = sample(seed, long_cigars=True, n_records=1500, big_name=60)
        w = want_of(seed, long_cigars=True, n_records=1500, big_name=60)
        cand = sorted({r for p in w[0] for r in p["records"]})
        nc = [int(s["batch"]["n_cigar"][r]) for r in cand]
        assert min(nc) > 5 and sum(1 for x in nc if x > 64) > 100 and max(int(s["batch"]["l_qseq"][r]) for r in cand) > 1000
        assert_equal(run(ctx, s), w, s, f"long CIGARs, seed {seed}")
        assert_equal(run(ctx, s, s["cuts"]), w, s, f"long CIGARs in batches, seed {seed}")
    s = sample(2)
    w = want_of(2)
    assert any(len(p["up_cigar"]) == 1 or len(p["down_cigar"]) == 1 for p in w[0])


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sample_equals_model(ctx, seed):
    s = sample(seed)
    a, b = MAPQS[seed % 4], MAPQS[(seed % 4 + 1 + seed // 4 % 3) % 4]
    assert_equal(run(ctx, s, min_mapq=a), want_of(seed, a), s, f"seed {seed}, one batch, min_mapq {a}")
    assert_equal(run(ctx, s, s["cuts"], min_mapq=b), want_of(seed, b), s, f"seed {seed}, cuts {s['cuts']}, min_mapq {b}")
    if a != 1 and b != 1:
        assert_equal(run(ctx, s, s["cuts"][:1]), want_of(seed), s, f"seed {seed}, two batches, min_mapq 1")


@pytest.mark.parametrize("seed", (0, 17))
def test_one_record_per_batch(ctx, seed):
    s = sample(seed, n_records=900, big_name=80)
    assert_equal(run(ctx, s, range(1, len(s["qnames"]))), want_of(seed, n_records=900, big_name=80), s, "one record per batch")


@pytest.mark.parametrize("bits", (64, 12, 8, 1))
def test_hash_runs(ctx, monkeypatch, bits):
    """SSV_RT_HASH_BITS: the name hash cut to its low bits - runs of equal hashes that hold many names, down to two lanes that walk the whole file"""
    monkeypatch.setenv("SSV_RT_HASH_BITS", str(bits))
    if bits == 1:      # the walk is quadratic in the run: small samples
        for seed in (0, 1):
            kw = dict(n_records=1500, big_name=100)
            s = sample(seed, **kw)
            w = want_of(seed, **kw)
            assert 1000 < w[1] <= 2000
            assert_equal(run(ctx, s, s["cuts"]), w, s, f"1 hash bit, seed {seed}")
    else:
        for seed in (0, 1, 2, 3):
            s = sample(seed)
            assert_equal(run(ctx, s, s["cuts"][:2]), want_of(seed), s, f"{bits} hash bits, seed {seed}")


TILE_KW = dict(n_records=8200, big_name=200)
EDGES = (1, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 1)


def test_tile_edges(ctx):
    """candidate counts and batch sizes on both sides of BLOCK (256) and of the scan's and the sort's 2048-element tiles"""
    s = sample(3, **TILE_KW)
    n, nt = len(s["qnames"]), len(s["contigs"])
    kept = np.cumsum([M.selected(s["batch"], i, 1, nt) for i in range(n)])
    assert kept[-1] >= EDGES[-1]
    whole = want_of(3, **TILE_KW)
    for e in EDGES:
        assert_equal(run(ctx, s, [e]), whole, s, f"first batch of {e} records")
        m_len = int(np.searchsorted(kept, e)) + 1       # the shortest prefix with e candidates
        t = take(s, range(m_len))
        w = model_of(t)
        assert w[1] == e
        assert_equal(run(ctx, t), w, t, f"{e} candidates")
    assert_equal(run(ctx, s, [2048, 4096, 6144]), whole, s, "batches of 2048")


def test_one_context_many_files(ctx):
    """big, small, big again on one context with a getclip and a getsv pass in between (the store the finish hands back is grown again; scan scratch is
    shared): every result equals the model and what a fresh context gives, the passes in between equal the oracle"""
    big, small = sample(3, **TILE_KW), sample(5, n_records=300, big_name=0)
    wb, ws = want_of(3, **TILE_KW), want_of(5, n_records=300, big_name=0)
    names, lens, b, rng = random_sample(7)
    got = []
    got.append(run(ctx, big, big["cuts"]))
    assert_tables_equal(ctx.getclip([b]), O.getclip([b]))
    got.append(run(ctx, small))
    hdr = host.Header(names, lens)
    juncs = sorted([(names[0], 500, "+", names[1], 900, "+"), (names[1], 700, "+", names[2], 1500, "-")], key=lambda j: (j[0], j[3], j[2], j[5], j[1], j[4]))
    plan = host.Plan(hdr, juncs, 300, 40, flank_length=50)
    c, r, p = ctx.discordant_and_depth([b], plan, 300, 40, 20, hdr.target_lens)
    ors, opd, _ = O.depth([b], plan.windows, plan.ranges, plan.points, 20)
    assert np.array_equal(c, O.discordant([b], plan.junctions, 300, 40, 4, 20)) and np.array_equal(r, ors) and np.array_equal(p, opd)
    plan.close()
    hdr.close()
    got.append(run(ctx, big))
    got.append(run(ctx, small, small["cuts"]))
    for g, w, s in zip(got, (wb, ws, wb, ws), (big, small, big, small)):
        assert_equal(g, w, s, "shared context")
    with device.Context(0) as fresh:
        assert run(fresh, big) == got[0] and run(fresh, small) == got[1]


def test_result_outlives_other_passes(ctx):
    """ssv_rt_result is valid until the next ssv_rt_begin: decoded only after a getclip pass has used the context (and the freed store's memory)"""
    s = sample(4)
    ctx.rt_begin(1, s["contigs"])
    for b, nm in zip(*M.split(s, s["cuts"])):
        ctx.rt_scan(b, nm)
    r = ctx.rt_finish()
    names, lens, b, rng = random_sample(9)
    assert_tables_equal(ctx.getclip([b]), O.getclip([b]))
    assert ctx.isize_stats([b], 20, 5000000) == O.isize_stats([b], 20, 5000000)
    assert_equal((ctx.rt_decode(r, s["contigs"]), r.n_candidates), want_of(4), s, "decoded after a getclip pass")


@pytest.mark.parametrize("chunk_mb", (1, 64))
def test_device_decoded_file_with_names_in_place(ctx, tmp_path, chunk_mb):
    """the device leg: a generated file decoded on the GPU (any record order, every record's bases), scanned where it lies with the read names
    of ssv_bamdec_names - in 1 MB chunks (records and names carried over chunk seams) and in one chunk"""
    kw = dict(safe=True, n_records=6000, big_name=300)
    s = sample(6, **kw)
    path = str(tmp_path / "f.bam")
    bamio.write_bam(path, s["contigs"], s["lens"], M.sample_records(s))
    n_chunks = n_records = 0
    with host.BamReader(path) as rd:
        assert rd.target_names == s["contigs"]
        ctx.rt_begin(1, s["contigs"])
        for b, info in ctx.bam_batches(rd, chunk_bytes=chunk_mb << 20, keep_all_seq=True, chunk_inflated=chunk_mb << 20, any_order=True):
            nm = ctx.bamdec_names()
            assert nm.mem == 1 and nm.bias > 0
            ctx.rt_scan(b, nm)
            n_chunks += 1
            n_records += info["n_records"]
        r = ctx.rt_finish()
    assert n_records == len(s["qnames"]) and (n_chunks > 1 if chunk_mb == 1 else n_chunks == 1)
    assert_equal((ctx.rt_decode(r, s["contigs"]), r.n_candidates), want_of(6, **kw), s, f"device decode, {n_chunks} chunks")
