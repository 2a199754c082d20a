"""The gapped re-aligner's model (tests/realign_gapped_model.py) alone, on the CPU: cases whose answer is worked out by hand below, and an independent
brute force that scores every two-piece alignment of short queries directly."""
import numpy as np
import pytest

import realign_gapped_model as GM
import realign_model as M
from realign_inputs import dna, other, revcomp

# One contig of 900 random bases between two others.  P is where the hand-made queries come from; the bases around the planned gaps are set so that
# no gap can slide: the base before a gap differs from the last base the gap removes (or inserts), the base behind it from the first.
P = 300


def _reference():
    rng = np.random.RandomState(77)
    c = list(dna(rng, 900))
    # deletion of c[P + 32 : P + 34] after 32 bases: c[P + 31] != c[P + 33] (the gap cannot start one base earlier)
    c[P + 31], c[P + 32], c[P + 33], c[P + 34] = "A", "G", "C", "T"
    # a homopolymer of eight A between a C and a G, 28 bases behind P + 200
    c[P + 227] = "C"
    c[P + 228:P + 236] = "A" * 8
    c[P + 236] = "G"
    # the 25 | 25 rescue at P + 400: c[P + 424] != the removed base c[P + 425] != c[P + 426]
    c[P + 424], c[P + 425], c[P + 426] = "T", "G", "A"
    return (dna(rng, 333), "".join(c), dna(rng, 401))


CONTIGS = _reference()
C1 = CONTIGS[1]
REF = M.Reference(CONTIGS)


def hit(query, **kw):
    h = GM.align_gapped(REF, query, **kw)
    assert not h["overflow"] and not h["tie"]
    return {k: h[k] for k in M.FIELDS + GM.GAP_FIELDS}


def expect(pos, q_end, score, gap_at, gap_len, reverse, n_mismatch=0):
    return dict(tid=1, pos=pos, q_beg=0, q_end=q_end, score=score, second=0, n_mismatch=n_mismatch, reverse=reverse, mapq=60, gap_at=gap_at, gap_len=gap_len)


@pytest.mark.parametrize("reverse", [0, 1])
def test_deletion_of_two_bases_in_the_middle_of_60(reverse):
    """32 bases, two reference bases missing, 28 bases.  Ungapped: the left piece alone, 32 (or a point more by chance), the right piece is below 30.
    Gapped: 32 + 28 - (6 + 2) = 52 over the whole query, from P, the gap before query base 32: 32M2D28M.  The reverse complement of the query gives
    the same alignment on the other strand: the hit's coordinates are those of its own orientation, which is the reference's."""
    q = C1[P:P + 32] + C1[P + 34:P + 62]
    assert len(q) == 60
    assert hit(revcomp(q) if reverse else q) == expect(P, 60, 52, 32, 2, reverse)
    assert GM.cigar_of(60, hit(q)) == [(32, "M"), (2, "D"), (28, "M")]
    assert 32 <= M.align(REF, q)["score"] <= 34 and M.align(REF, q)["q_beg"] == 0


@pytest.mark.parametrize("reverse", [0, 1])
def test_insertion_of_three_bases_in_the_middle_of_60(reverse):
    """29 bases, three bases that are not in the reference, 28 bases: 29 + 28 - (6 + 3) = 48, 29M3I28M.  The inserted bases differ from the
    reference bases they lie on along either diagonal's continuation, and the last of them from the base before the gap, so the gap cannot slide"""
    a = P + 100
    ins = other(C1[a + 29]) + other(C1[a + 30]) + (other(C1[a + 28]) if other(C1[a + 28]) != C1[a + 31] else other(C1[a + 28], 2))
    q = C1[a:a + 29] + ins + C1[a + 29:a + 57]
    assert len(q) == 60
    assert hit(revcomp(q) if reverse else q) == expect(a, 60, 48, 29, -3, reverse)
    assert GM.cigar_of(60, hit(q)) == [(29, "M"), (3, "I"), (28, "M")]


def test_two_halves_of_25_are_rescued():
    """25 | one base missing | 25: either half alone scores 25 (below 30: unaligned without the gap); together 25 + 25 - 7 = 43"""
    a = P + 400
    q = C1[a:a + 25] + C1[a + 26:a + 51]
    assert M.align(REF, q)["tid"] == -1
    assert hit(q) == expect(a, 50, 43, 25, 1, 0)
    assert hit(revcomp(q)) == expect(a, 50, 43, 25, 1, 1)
    # 25 matching bases and nothing else stay unaligned
    assert hit(C1[a:a + 25] + other(C1[a + 25]) + dna(np.random.RandomState(5), 24))["tid"] == -1


def test_gap_in_a_homopolymer_is_left_aligned():
    """the reference has C AAAAAAAA G, the query C AAAAAA G: any of the seven places in the run gives 28 + 6 + 26 - 8 = 52; the first one, behind the
    C (query base 28), is reported.  One A more than the reference: the inserted base is the run's first"""
    a = P + 200
    q = C1[a:a + 28] + "A" * 6 + C1[a + 36:a + 62]
    assert len(q) == 60
    assert hit(q) == expect(a, 60, 52, 28, 2, 0)
    assert hit(revcomp(q)) == expect(a, 60, 52, 28, 2, 1)
    q = C1[a:a + 28] + "A" * 9 + C1[a + 36:a + 59]
    assert hit(q) == expect(a, 60, 60 - 1 - 7, 28, -1, 0)


def test_mismatches_count_over_both_pieces_only():
    """one substitution in either piece of the 2-base deletion: 52 - 2 x 5, two mismatches; the inserted bases of an insertion are not counted"""
    q = list(C1[P:P + 32] + C1[P + 34:P + 62])
    q[10], q[50] = other(q[10]), other(q[50])
    assert hit("".join(q)) == expect(P, 60, 42, 32, 2, 0, n_mismatch=2)


def test_bam_record():
    q = C1[P:P + 32] + C1[P + 34:P + 62]
    qual = "".join(chr(40 + i) for i in range(60))
    r = GM.bam_record("ttt" + revcomp(q), "!!!" + qual, GM.align_gapped(REF, "ttt" + revcomp(q)))
    assert r == dict(flag=16, tid=1, pos=P, mapq=60, cigar=[(32, "M"), (2, "D"), (28, "M"), (3, "S")], seq=q + "AAA", qual=qual[::-1] + "!!!")
    assert GM.bam_record(q[:25], qual[:25], GM.align_gapped(REF, q[:25])) == M.bam_record(q[:25], qual[:25], M.align(REF, q[:25]))


# ---- brute force ----

def pair_score(s, text, c_lo, c_hi, dl, dr, b, k, j, e):
    """the sum of a two-piece alignment, base by base; None when a base lies outside the contig"""
    total = 0
    for lo, hi, diag in ((b, k, dl), (j, e, dr)):
        if not (c_lo <= diag + lo and diag + hi <= c_hi):
            return None
        total += sum(1 if x == y else -4 for x, y in zip(s[lo:hi], text[diag + lo:diag + hi]))
    return total


def brute_force(ref, s, w):
    """the largest J of the rule: for every variant and every k all free ends are scored directly; the free end is the best one, or the query's end
    when that is inside the contig and loses less than 5 against the best"""
    n, d, qb, qe = len(s), w["diag"], w["q_beg"], w["q_end"]
    c_lo, c_hi = ref.off[w["tid"]], ref.off[w["tid"] + 1]
    top = None
    for L in range(1, 17):
        for g, ins in ((L, 0), (-L, L)):
            for k in range(1, n):
                j = k + ins
                if j > n - 1:
                    continue
                if k > qb:   # the winner is the left piece [q_beg, k)
                    sc = {e: pair_score(s, ref.text, c_lo, c_hi, d, d + g, qb, k, j, e) for e in range(j + 1, n + 1)}
                    sc = {e: v for e, v in sc.items() if v is not None}
                    if sc:
                        v = max(sc.values())
                        if n in sc and sc[n] > v - 5:
                            v = sc[n]
                        top = v - 6 - L if top is None else max(top, v - 6 - L)
                if j < qe:   # the winner is the right piece [j, q_end)
                    sc = {b: pair_score(s, ref.text, c_lo, c_hi, d - g, d, b, k, j, qe) for b in range(0, k)}
                    sc = {b: v for b, v in sc.items() if v is not None}
                    if sc:
                        v = max(sc.values())
                        if 0 in sc and sc[0] > v - 5:
                            v = sc[0]
                        top = v - 6 - L if top is None else max(top, v - 6 - L)
    return top


def short_queries():
    rng = np.random.RandomState(99)
    out = []
    for i in range(32):
        n = 38 + i % 3
        kind, L = "DI"[i & 1], 1 + (i >> 2) % 2
        short = 6 + i % 6   # one side keeps 25 bases or more (a seed), the other has 6..11: 8 pay for a 1-base gap, 9 for two bases
        at = short if i & 2 else n - short - (L if kind == "I" else 0)
        t = int(rng.randint(3))
        c = CONTIGS[t]
        p = int(rng.randint(0, len(c) - n - L)) if i % 5 else (0 if i % 10 else len(c) - n - (L if kind == "D" else 0))   # some at a contig's ends
        if kind == "D":
            q = c[p:p + at] + c[p + at + L:p + L + n]
        else:
            q = c[p:p + at] + dna(rng, L) + c[p + at:p + n - L]
        q = list(q)
        for x in rng.randint(0, n, int(rng.randint(2))):
            q[int(x)] = "ACGTN"[int(rng.randint(5))]
        q = "".join(q)
        out.append(revcomp(q) if i % 3 == 0 else q)
    return out


def test_against_the_brute_force():
    """queries of 38-40 bases with a gap of 1-2 bases and at most one changed base: the model's score is the brute force's best where that beats the
    ungapped score, and the ungapped score where it does not; the model's own pieces add up to its score"""
    n_gapped = n_first = 0
    for q in short_queries():
        w, _, overflow, tie = GM.first_stage(REF, q)
        assert not overflow and not tie
        if w is None:
            continue
        n_first += 1
        s = M.orientations(q)[w["st"]]
        best = brute_force(REF, s, w)
        r = GM.refine(REF, s, w)
        if best is not None and best > w["score"]:
            assert r is not None and r["J"] == best, (q, r, best)
            c_lo, c_hi = REF.off[w["tid"]], REF.off[w["tid"] + 1]
            assert pair_score(s, REF.text, c_lo, c_hi, r["dl"], r["dr"], r["b"], r["k"], r["j"], r["e"]) - 6 - r["L"] == best
            n_gapped += 1
        else:
            assert r is None, (q, r, best)
    assert n_gapped >= 10 and n_first - n_gapped >= 5, (n_first, n_gapped)   # both outcomes are compared
