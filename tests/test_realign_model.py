"""CPU: the Python model of the clipped-sequence re-aligner (tests/realign_model.py) anchored three ways, and the input sets of
tests/test_realign_differential_gpu.py held against the conditions that make an exact comparison with the kernel meaningful.

1. bwa mem 0.7.10's own records for the clipped sequences of the synthetic samples (tests/golden/synth/*.clip.bam), under the acceptance rules
   and thresholds of tests/test_realign_gpu.py::test_realign_agrees_with_bwa_mem.
2. Cases small enough to work out by eye, one per rule: segment, extension threshold, floor, contig edge, same-locus window, MAPQ ladder.
3. Every generated set: no `overflow` and no `tie` query (the named overflow set excepted), and the edge the set is built for is really there."""
import os

import pytest

import bamio
import golden_util as G
import realign_inputs as I
import realign_model as M

SAMPLES = {"synthfull": dict(genome_frac=1 / 8192, depth=40, n_sv=24), "hbvfull": dict(genome_frac=1 / 8192, depth=60, n_sv=8, n_integrations=10)}


def run(contigs, queries):
    ref = M.Reference(contigs)
    return ref, [M.align(ref, q) for q in queries]


def fields(h):
    return tuple(h[k] for k in M.FIELDS)


# ---- 1. bwa mem ----
@pytest.mark.parametrize("name", list(SAMPLES))
def test_model_agrees_with_bwa_mem(name):
    from seeksv_amd import synth
    w = synth.Workload(**SAMPLES[name])
    contigs = [("".join(part.splitlines()[1:])) for part in w.reference_fasta().split(">")[1:]]
    ref = M.Reference(contigs)
    names, recs = bamio.read_bam_records(os.path.join(G.GOLDEN, "synth", f"{name}.clip.bam"))
    assert names == list(w.names)
    prim = [r for r in recs if not r["flag"] & 0x900]
    n_conf = n_same = n_unal = n_unal_same = 0
    for r in prim:
        h = M.align(ref, r["qname"])
        M.check_hit(ref.text, ref.off, r["qname"], h)
        ops = "".join(op for _, op in r["cigar"])
        if r["flag"] & 4:
            n_unal += 1
            n_unal_same += int(h["tid"] == -1 or h["mapq"] < 60)
            continue
        aligned = sum(l for l, op in r["cigar"] if op == "M")
        if r["mapq"] < 20 or aligned < 30 or "I" in ops or "D" in ops:
            continue
        lead = r["cigar"][0][0] if r["cigar"][0][1] in "SH" else 0
        n_conf += 1
        n_same += int(h["tid"] == r["tid"] and bool(h["reverse"]) == bool(r["flag"] & 16) and h["pos"] - h["q_beg"] == r["pos"] - lead and h["mapq"] > 0)
    assert n_conf >= 30, n_conf
    assert n_same >= 0.98 * n_conf, (n_same, n_conf)
    assert n_unal_same >= 0.9 * n_unal, (n_unal_same, n_unal)


# ---- 2. by hand ----
C = "TGTCGGACAATGTAGATATCCTATACTCTGAGCGGCCGCCGCGTAGCGAAAGACTTTGAGCTTG"   # contig 0, 64 bases
D = "CCTAACGGTTTACTTTGTCCCCTAGGGTCGTACGCTACGT"                           # contig 1, 40 bases
X = "ATAAACGTGGATTGTAAAGAGCGTCCGACGATCAACATGTTACTAAGCATTGACGGTATATCAG"   # 64 bases, cut in two at 34 in contigs 2 and 3
P, S = "TACAAGTTAGGCTGGGGCTAAATCTAATAG", "GAAATGCTGTTAAGGCTCCTTCTGGTGAAC"   # 30 bases in front of / behind X's parts
J32, J33 = "G" * 32, "G" * 33   # X[34] = 'A' and X[33] = 'C': the insert matches neither of its neighbours along either diagonal
HAND_REF = [C, D, P + X[:34] + J32 + X[34:] + S, P + X[:34] + J33 + X[34:] + S]


def hit(tid, pos, q_beg, q_end, score, second, n_mismatch, reverse, mapq):
    return (tid, pos, q_beg, q_end, score, second, n_mismatch, reverse, mapq)


NONE = hit(-1, -1, 0, 0, 0, 0, 0, 0, 0)
q40 = C[4:44]
HAND = [
    # the floor: 30 matches are reported, 29 are not; a reverse hit's q_beg / q_end count along the reverse-complemented query
    ("exact 30", C[4:34], hit(0, 4, 0, 30, 30, 0, 0, 0, 60)),
    ("exact 29", C[4:33], NONE),
    ("exact 30, reverse", I.revcomp(C[4:34]), hit(0, 4, 0, 30, 30, 0, 0, 1, 60)),
    # 5 matches, a mismatch, 29 matches: the sum never falls to 0, so one segment of 5 - 4 + 29 = 30; with 28 behind it 29 is the best
    ("5 X 29", I.sub(C[4:39], [5]), hit(0, 4, 0, 35, 30, 0, 1, 0, 60)),
    ("5 X 28", I.sub(C[4:38], [5]), NONE),
    # 4 matches and a mismatch bring the sum to 0: the segment starts anew behind them (35); the head sums to 0 > -5 and is taken back in
    ("4 X 35", I.sub(q40, [4]), hit(0, 4, 0, 40, 35, 0, 1, 0, 60)),
    # the end-extension threshold: a lost end of -4 is kept (39 - 4), one of -8 is clipped; -5 (XXMMM) is clipped, -4 (XXMMMM) kept
    ("tail X", I.sub(q40, [39]), hit(0, 4, 0, 40, 35, 0, 1, 0, 60)),
    ("tail XX", I.sub(q40, [38, 39]), hit(0, 4, 0, 38, 38, 0, 0, 0, 60)),
    ("head X", I.sub(q40, [0]), hit(0, 4, 0, 40, 35, 0, 1, 0, 60)),
    ("head XX", I.sub(q40, [0, 1]), hit(0, 6, 2, 40, 38, 0, 0, 0, 60)),
    ("tail XXMMM", I.sub(q40, [35, 36]), hit(0, 4, 0, 35, 35, 0, 0, 0, 60)),
    ("tail XXMMMM", I.sub(q40, [34, 35]), hit(0, 4, 0, 40, 30, 0, 2, 0, 60)),
    ("head MMMXX", I.sub(q40, [3, 4]), hit(0, 9, 5, 40, 35, 0, 0, 0, 60)),
    ("head MMMMXX", I.sub(q40, [4, 5]), hit(0, 4, 0, 40, 30, 0, 2, 0, 60)),
    # the floor holds for what is reported: 30 matches and a mismatch on the last base are extended to 26 and not reported, with two
    # mismatches the end is clipped and the 30 stay
    ("30 X", I.sub(C[4:35], [30]), NONE),
    ("30 XX", I.sub(C[4:36], [30, 31]), hit(0, 4, 0, 30, 30, 0, 0, 0, 60)),
    # the maximum is strict: 35, X, 4 matches reaches 35 again and does not move the end; the tail -4 + 4 = 0 is then taken back in
    ("lower case, N", q40[:35].lower() + "N" + q40[36:].lower(), hit(0, 4, 0, 40, 35, 0, 1, 0, 60)),
    # an end outside the contig: 34 bases of C's end and 10 of D's start.  Inside C the segment ends at the edge although the text goes on
    # matching; D's share is shorter than a seed and is not scored
    ("over the edge", C[30:] + D[:10], hit(0, 30, 0, 34, 34, 0, 0, 0, 60)),
    ("over the edge, reverse", I.revcomp(C[30:] + D[:10]), hit(0, 30, 0, 34, 34, 0, 0, 1, 60)),
    # 24 of C and 30 of D: D wins, C's share is the runner-up at another contig (same diagonal): gap 6
    ("two contigs", C[40:] + D[:30], hit(1, 0, 24, 54, 30, 0, 0, 0, 60)),
    ("two contigs 30 + 34", C[34:] + D[:34], hit(1, 0, 30, 64, 34, 30, 0, 0, 24)),
]


def test_model_by_hand():
    ref = M.Reference(HAND_REF)
    for label, q, want in HAND:
        h = M.align(ref, q)
        assert fields(h) == want, (label, fields(h), want)
        assert not h["tie"] and not h["overflow"]
        M.check_hit(ref.text, ref.off, q, h)


def test_model_same_locus_window():
    """X[:34] and X[34:] on two diagonals of one contig, 32 (contig 2) or 33 (contig 3) apart: the 30-base part is the runner-up only
    outside the window.  The same query finds both contigs: the exact copy of 34 is there twice (score 34, second 34)."""
    ref = M.Reference(HAND_REF[2:3])
    assert fields(M.align(ref, X)) == hit(0, 30, 0, 34, 34, 0, 0, 0, 60)
    ref = M.Reference(HAND_REF[3:4])
    assert fields(M.align(ref, X)) == hit(0, 30, 0, 34, 34, 30, 0, 0, 24)
    assert fields(M.align(ref, I.revcomp(X))) == hit(0, 30, 0, 34, 34, 30, 0, 1, 24)
    ref = M.Reference(HAND_REF)
    assert fields(M.align(ref, X)) == hit(2, 30, 0, 34, 34, 34, 0, 0, 0)   # equal scores: strand, then the smaller diagonal


def test_model_mapq_ladder_and_limits():
    assert [M.mapq_of(50, s) for s in (60, 50, 49, 48, 45, 41, 40, 30, 0)] == [0, 0, 6, 12, 30, 54, 60, 60, 60]
    ref = M.Reference(HAND_REF)
    assert fields(M.align(ref, C[:19])) == NONE and fields(M.align(ref, "")) == NONE
    long_ref = M.Reference([C * 20])
    assert fields(M.align(long_ref, (C * 20)[:1025])) == NONE
    assert M.align(long_ref, (C * 20)[:1025])["n_seeds"] == 0
    # the index: positions 0 mod 4 of the concatenation whose 20-mer stays inside one contig
    assert ref.n_sampled == sum(1 for p in range(0, len(ref.text), 4) if p + 20 <= ref.off[ref.contig_of(p) + 1])
    assert M.Reference(["A" * 17, "C" * 23]).n_sampled == 1   # only p = 20 (0, 4 .. 16 run into the next contig; 24 and on are too close to the end)
    words, off = M.pack_2bit(["ACGT" * 9, "ttg"])
    assert [int(x) for x in words] == [0xe4e4e4e4e4e4e4e4, 0x2fe4, 0] and list(off) == [0, 36, 39]


def test_check_hit_refuses_wrong_fields():
    ref = M.Reference(HAND_REF)
    q = I.sub(q40, [39])
    good = M.align(ref, q)
    M.check_hit(ref.text, ref.off, q, good)
    for k, v in (("score", 36), ("n_mismatch", 0), ("q_end", 41), ("pos", 5), ("mapq", 30), ("second", 36), ("reverse", 1), ("tid", 1)):
        with pytest.raises(AssertionError):
            M.check_hit(ref.text, ref.off, q, dict(good, **{k: v}))
    with pytest.raises(AssertionError):
        M.check_hit(ref.text, ref.off, q, dict(M.UNALIGNED, score=1))


# ---- 3. the generated sets ----
def no_flags(hits, labels=None):
    bad = [(i if labels is None else labels[i]) for i, h in enumerate(hits) if h["overflow"] or h["tie"]]
    assert not bad, bad


@pytest.mark.parametrize("shape", list(I.SHAPES))
def test_random_and_threshold_sets(shape):
    contigs, queries = I.random_set(shape)
    off = I.offsets(contigs)
    assert any(o % 4 for o in off[1:]) and any(o % 32 for o in off[1:]) and min(len(c) for c in contigs) < M.K
    ref, hits = run(contigs, queries)
    no_flags(hits)
    assert 550 <= len(queries) <= 700
    al = [h for h in hits if h["tid"] >= 0]
    assert len(al) >= 500 and sum(h["reverse"] for h in al) >= 200
    assert any(0 < h["mapq"] < 60 for h in al) and any(h["mapq"] == 60 for h in al) and sum(h["n_mismatch"] > 0 for h in al) >= 150 and sum(h["second"] > 0 for h in al) >= 5
    assert sum(h["q_beg"] > 0 for h in al) >= 50 and sum(h["q_end"] < len(q) for q, h in zip(queries, hits) if h["tid"] >= 0) >= 50
    assert {len(q) for q in queries} >= {0, 19, 20, 49, 50, 1024, 1025}
    contigs, queries, labels = I.threshold_set(shape)
    ref, hits = run(contigs, queries)
    no_flags(hits, labels)
    by = dict(zip(labels, hits))
    for st in ("/fwd", "/rev"):
        assert by["exact29" + st]["tid"] == -1 and by["exact30" + st]["score"] == 30
        assert by["mismatch-at-5-of-34" + st]["tid"] == -1 and by["mismatch-at-5-of-35" + st]["score"] == 30
        assert by["flanked29" + st]["tid"] == -1 and by["flanked30" + st]["score"] == 30
        for end in ("tail-", "head-"):
            span = lambda pat: by[end + pat + st]["q_end"] - by[end + pat + st]["q_beg"]
            assert (span("X"), span("XX"), span("XXMMM"), span("XXMMMM"), span("XMXMM"), span("XMXMMM")) == (61, 60, 60, 66, 60, 66)
            assert by[end + "XMMMMX" + st]["score"] == 56 and by[end + "XMMMMMX" + st]["score"] == 57
        over = [l for l in labels if l.startswith("over-") and l.endswith(st)]
        assert len(over) >= 24 and all(by[l]["score"] == 45 and by[l]["q_end"] - by[l]["q_beg"] == 45 for l in over)


def test_two_locus_and_sweep_sets():
    contigs, queries, labels = I.two_locus_set()
    ref, hits = run(contigs, queries)
    no_flags(hits, labels)
    by = dict(zip(labels, hits))
    for opp in ("same", "opp"):
        for where in ("other", "same"):
            assert [by[f"copy-m{m}-{opp}-{where}-contig/fwd"]["score"] - by[f"copy-m{m}-{opp}-{where}-contig/fwd"]["second"] for m in range(4)] == [0, 5, 10, 15]
        assert [by[f"partial-gap{g}-{opp}/rev"]["mapq"] for g in range(1, 10)] == [6 * g for g in range(1, 10)]
    for kind in ("ins", "del"):
        assert all(by[f"{kind}{d}-64/56/fwd"]["second"] == 0 for d in (4, 8, 31, 32))
        assert all(by[f"{kind}{d}-64/56/fwd"]["second"] >= 56 for d in (33, 34, 64))
    contigs, queries, labels = I.sweep_set()
    ref, hits = run(contigs, queries)
    no_flags(hits, labels)
    assert [len(q) for q in queries] == 2 * list(range(255, 301))
    assert sum(h["n_seeds_fwd"] == 64 for h in hits[:46]) >= 1 and sum(h["n_seeds_fwd"] == 64 for h in hits[46:]) >= 1
    assert all(h["second"] == h["score"] and h["mapq"] == 0 for h in hits[:46])
    assert all(h["second"] == h["score"] - 5 and h["mapq"] == 30 for h in hits[46:])
    assert all(h["n_seeds"] <= M.MAX_CAND for h in hits)


def test_tandem_and_overflow_sets():
    contigs, queries, labels = I.tandem_set()
    ref, hits = run(contigs, queries)
    no_flags(hits, labels)
    assert all(h["n_seeds"] <= M.MAX_CAND for h in hits)
    assert sum(h["n_candidates"] > 64 for h in hits) >= 60 and max(h["n_candidates"] for h in hits) > 80
    assert sum(0 < h["mapq"] < 60 for h in hits) >= 4   # a unique locus whose runner-up is one of the array's diagonals
    assert any(h["tid"] == 1 and h["n_candidates"] > 64 for h in hits)   # a query of the diverged array that also seeds in the first
    contigs, queries, labels = I.overflow_set()
    ref, hits = run(contigs, queries)
    assert not any(h["tie"] for h in hits)
    exact = [h for h in hits if not h["overflow"]]
    assert len(exact) == 3 and all(h["n_seeds"] > M.MAX_CAND and h["n_candidates"] == 1 for h in exact)   # 251 seeds of one diagonal
    assert sum(h["overflow"] for h in hits) >= 6


def test_low_complexity_many_contigs_and_cli_sets():
    contigs, queries, expect = I.low_complexity_set()
    ref = M.Reference(contigs)
    assert len(ref.index["A" * M.K]) == I.poly_a_sampled(contigs) > 1400   # the poly-A contig's sampled positions: all but 256 find no slot
    assert sum(e is not None for e in expect) >= 100 and all(len(q) >= 60 for q, e in zip(queries, expect) if e is not None)
    for q, e in zip(queries, expect):
        if e is not None:
            h = M.align(ref, q)
            assert (h["tid"], h["pos"] - h["q_beg"], h["reverse"]) == e, (q, h)
    contigs, queries = I.many_contigs_set()
    assert len(contigs) == 66500 > 1 << 16
    ref, hits = run(contigs, queries)
    no_flags(hits)
    assert [h["tid"] for h in hits] == [t for t in I.MANY_QUERY_CONTIGS for _ in range(3)]
    assert all(h["mapq"] == 60 and h["n_mismatch"] == 0 for h in hits)
    names, contigs, fq = I.cli_set()
    ref, hits = run(contigs, [s for s, _ in fq])
    no_flags(hits)
    recs = [M.bam_record(s, q, h) for (s, q), h in zip(fq, hits)]
    assert {r["flag"] for r in recs} == {0, 4, 16} and any(len(r["cigar"]) == 3 for r in recs) and any(len(r["cigar"]) == 1 for r in recs)
    assert any("N" in r["seq"] and r["flag"] == 16 for r in recs) and len(fq) >= 55
