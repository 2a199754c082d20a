"""The model of the re-aligner's alternate loci (tests/realign_alts_model.py) against cases worked out by hand.  CPU only.

The references below are random filler around planted copies; every expected hit is written out: a copy at contig position p that matches the whole
query comes back with pos p, q_beg 0, q_end n; k substitutions away from the query's ends cost 5 k (a match lost, a mismatch paid)."""
import numpy as np
import pytest

import realign_alts_model as AM
import realign_gapped_model as GM
import realign_model as M
import realign_sorted_model as SM
from realign_inputs import dna, revcomp, sub

INDEXES = [None, 500]   # hash, sorted


def hit(tid, pos, n, score, second, mm, reverse=0, mapq=0, flags=0, q_beg=0):
    return dict(tid=tid, pos=pos, q_beg=q_beg, q_end=q_beg + n, score=score, second=second, n_mismatch=mm, reverse=reverse, mapq=mapq, flags=flags)


def three_copies():
    rng = np.random.RandomState(7)
    e = dna(rng, 60)
    copy = "GG" + e + "CCCC"   # the same neighbours at every copy: what a query carries beyond the element meets the same bases at all three
    return e, M.Reference([dna(rng, 98) + copy + dna(rng, 134) + copy + dna(rng, 73), dna(rng, 31) + copy + dna(rng, 46)])


@pytest.mark.parametrize("max_occ", INDEXES)
def test_three_exact_copies(max_occ):
    """a 60-base element at a0:100, a0:300 and a1:33, queried exactly: the first copy is the primary (MAPQ 0: the others score as much), the other two
    follow by diagonal; on the other strand the same places with reverse = 1"""
    e, ref = three_copies()
    r = AM.align_alts(ref, e, 16, max_occ)
    assert r["primary"] == hit(0, 100, 60, 60, 60, 0)
    assert r["alts"] == [hit(0, 300, 60, 60, 60, 0), hit(1, 33, 60, 60, 60, 0)]
    assert not r["overflow"] and not r["tie"]
    r = AM.align_alts(ref, revcomp(e), 16, max_occ)
    assert r["primary"] == hit(0, 100, 60, 60, 60, 0, reverse=1)
    assert r["alts"] == [hit(0, 300, 60, 60, 60, 0, reverse=1), hit(1, 33, 60, 60, 60, 0, reverse=1)]


@pytest.mark.parametrize("max_occ", INDEXES)
def test_max_alt_cuts_and_flags(max_occ):
    """max_alt 1 keeps the first alternate and sets ALT_CUT on the primary and on the alternate; max_alt 2 keeps both and sets nothing"""
    e, ref = three_copies()
    r = AM.align_alts(ref, e, 1, max_occ)
    assert r["primary"] == hit(0, 100, 60, 60, 60, 0, flags=AM.F_ALT_CUT)
    assert r["alts"] == [hit(0, 300, 60, 60, 60, 0, flags=AM.F_ALT_CUT)]
    r = AM.align_alts(ref, e, 2, max_occ)
    assert r["primary"]["flags"] == 0 and len(r["alts"]) == 2
    with pytest.raises(AssertionError):
        AM.align_alts(ref, e, 0, max_occ)
    with pytest.raises(AssertionError):
        AM.align_alts(ref, e, 17, max_occ)


@pytest.mark.parametrize("max_occ", INDEXES)
def test_two_substitutions_in_three_out(max_occ):
    """best 60: a copy with 2 substitutions scores 50 (5 * 50 = 250 >= 240: in), one with 3 scores 45 (225 < 240: out); the primary's second and MAPQ
    count both (second 50, gap 10: 60)"""
    rng = np.random.RandomState(8)
    e = dna(rng, 60)
    ref = M.Reference([dna(rng, 90) + e + dna(rng, 110) + sub(e, [25, 50]) + dna(rng, 80) + sub(e, [24, 49, 54]) + dna(rng, 70)])
    r = AM.align_alts(ref, e, 16, max_occ)
    assert r["primary"] == hit(0, 90, 60, 60, 50, 0, mapq=60)
    assert r["alts"] == [hit(0, 260, 60, 50, 60, 2)]
    scores = sorted(c[0] for c in AM.scored_candidates(ref, e, max_occ))
    assert scores == [45, 50, 60]   # the third copy is a candidate; the ratio keeps it out


@pytest.mark.parametrize("max_occ", INDEXES)
def test_ratio_equality(max_occ):
    """best 50: 40 is in (200 >= 200), 39 is out (195 < 200).  40: the 50 bases with 2 substitutions.  39: the same copy at the very start of the
    second contig without its first base - 49 bases inside the contig, 47 matches - 8, and nothing to extend over a contig's start"""
    rng = np.random.RandomState(9)
    e = dna(rng, 50)
    two = sub(e, [24, 47])
    ref = M.Reference([dna(rng, 120) + e + dna(rng, 130) + two + dna(rng, 60), two[1:] + dna(rng, 100)])
    r = AM.align_alts(ref, e, 16, max_occ)
    assert r["primary"] == hit(0, 120, 50, 50, 40, 0, mapq=60)
    assert r["alts"] == [hit(0, 300, 50, 40, 50, 2)]
    assert sorted(c[0] for c in AM.scored_candidates(ref, e, max_occ)) == [39, 40, 50]
    third = [c for c in AM.scored_candidates(ref, e, max_occ) if c[0] == 39][0]
    assert third[1:] == (0, 410 - 1, 1, 1, 50, 2)   # strand 0, diagonal one base before the second contig's first (410), contig 1, segment [1, 50), 2 mismatches


@pytest.mark.parametrize("max_occ", INDEXES)
def test_primary_is_the_plain_models(max_occ):
    """the primary of align_alts is realign_model.align / realign_sorted_model.align_sorted / realign_gapped_model.align_gapped, field for field"""
    e, ref = three_copies()
    rng = np.random.RandomState(10)
    for q in (e, revcomp(e), sub(e, [30]), e[:19], dna(rng, 50), ref.contigs[0][40:130], ref.contigs[1][:40]):
        want = M.align(ref, q) if max_occ is None else SM.align_sorted(ref, q, max_occ)
        got = AM.align_alts(ref, q, 16, max_occ)["primary"]
        assert {k: got[k] for k in M.FIELDS} == {k: want[k] for k in M.FIELDS}, q
        wantg = GM.align_gapped(ref, q, max_occ)
        gotg = AM.align_alts(ref, q, 16, max_occ, gapped=True)["primary"]
        assert {k: gotg[k] for k in M.FIELDS + GM.GAP_FIELDS} == {k: wantg[k] for k in M.FIELDS + GM.GAP_FIELDS}, q


def test_unaligned_has_none_and_rows():
    """too short, too long, random: no alternates, no flag.  bam_records: the primary's row, then flag 256 (| 16), MAPQ 0, S M S"""
    e, ref = three_copies()
    rng = np.random.RandomState(11)
    for q in (e[:19], dna(rng, 1025), dna(rng, 60)):
        r = AM.align_alts(ref, q, 16)
        assert r["primary"]["tid"] == -1 and r["primary"]["flags"] == 0 and r["alts"] == []
    q = "ACGT" + revcomp(e) + "TT"   # on the reverse strand AA + e + ACGT against GG + e + CCCC: -8 and -11, dearer than clipping
    rows = AM.bam_records(q, "I" * 30 + "5" * 36, AM.align_alts(ref, q, 16))
    assert [(x["flag"], x["tid"], x["pos"], x["mapq"], x["cigar"]) for x in rows] == [
        (16, 0, 100, 0, [(2, "S"), (60, "M"), (4, "S")]), (256 | 16, 0, 300, 0, [(2, "S"), (60, "M"), (4, "S")]), (256 | 16, 1, 33, 0, [(2, "S"), (60, "M"), (4, "S")])]
    assert all(x["seq"] == revcomp(q) and x["qual"] == ("I" * 30 + "5" * 36)[::-1] for x in rows)
