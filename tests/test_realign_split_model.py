"""CPU: the model of the two-piece split alignments (tests/realign_split_model.py) against cases worked out by hand on the reference of
tests/realign_split_inputs.py: every read there was drawn first and its pieces planted between flanks that match nowhere, so a piece's segment, score
and position are known without running anything.  Then the model's rows through the read-through model's FindJunction: the planted junction."""
import pytest

import realign_model as M
import realign_sorted_model as SRT
import realign_split_inputs as SI
import realign_split_model as SM
import readthrough_model as RT
from realign_inputs import revcomp

# case -> (primary, mate or None) of the read as drawn: (planted piece, q_beg, q_end, score, second, mapq, reverse); q_beg / q_end in the hit's own
# orientation: a piece [b, e) of a 100-base read on the reverse strand is [100 - e, 100 - b)
EXPECT = {
    "ff": (("A", 0, 60, 60, 0, 60, 0), ("B", 60, 100, 40, 0, 60, 0)),
    "fr": (("A", 0, 60, 60, 0, 60, 0), ("B", 0, 40, 40, 0, 60, 1)),
    "rf": (("A", 40, 100, 60, 0, 60, 1), ("B", 60, 100, 40, 0, 60, 0)),
    "rr": (("A", 40, 100, 60, 0, 60, 1), ("B", 0, 40, 40, 0, 60, 1)),
    "overlap5": (("A", 0, 60, 60, 0, 60, 0), ("B", 55, 100, 45, 0, 60, 0)),         # 5 shared bases: microhomology
    "gap10": (("A", 0, 55, 55, 0, 60, 0), ("B", 65, 100, 35, 0, 60, 0)),            # 10 bases of neither
    "contained": (("A", 0, 100, 100, 40, 60, 0), None),                             # [30, 70) inside [0, 100): no mate, `second` as the plain call has it
    "del20": (("A", 0, 60, 60, 0, 60, 0), ("B", 60, 100, 40, 0, 60, 0)),            # diagonals 20 apart: one locus for `second`, a mate all the same
    "own20": (("A", 0, 70, 70, 0, 60, 0), ("B", 40, 90, 50, 0, 60, 0)),             # the mate keeps [70, 90): 20
    "own19": (("A", 0, 70, 70, 49, 60, 0), None),                                   # [70, 89): 19
    "own20-tie": (("A", 0, 60, 60, 0, 60, 0), ("B", 20, 80, 60, 0, 60, 0)),         # the primary keeps [0, 20): 20; equal scores: the smaller diagonal is the primary
    "own19-tie": (("A", 0, 60, 60, 60, 0, 0), None),                                # [0, 19): 19 - and the plain call's MAPQ 0
    "score30": (("A", 0, 60, 60, 0, 60, 0), ("B", 65, 100, 30, 0, 60, 0)),          # 31 - 4 + 3
    "score29": (("A", 0, 60, 60, 29, 60, 0), None),                                 # 30 - 4 + 3: scored, counted by `second`, no mate
    "comp20": (("A", 0, 60, 60, 0, 60, 0), ("B", 62, 100, 38, 30, 48, 0)),          # K = [52, 82) shares 20 bases with the mate, 8 with the primary
    "comp19": (("A", 0, 60, 60, 0, 60, 0), ("B", 62, 100, 38, 0, 60, 0)),           # K = [51, 81): 19
    "mapq5050": (("A", 0, 50, 50, 0, 60, 0), ("B", 50, 100, 50, 0, 60, 0)),
    "p-twocopy": (("A", 0, 60, 60, 60, 0, 0), ("B", 60, 100, 40, 0, 60, 0)),
    "m-twocopy": (("A", 0, 60, 60, 0, 60, 0), ("B", 60, 100, 40, 40, 0, 0)),        # forward before reverse, although the reverse copy lies in an earlier contig
}


@pytest.fixture(scope="module")
def ref():
    return M.Reference(SI.reference())


def hit_of(ref, case, spec, flip):
    label, qb, qe, score, second, mapq, rev = spec
    g = SI.where(f"{case}:{label}")
    tid = ref.contig_of(g)
    return dict(tid=tid, pos=g - ref.off[tid], q_beg=qb, q_end=qe, score=score, second=second, n_mismatch=(qe - qb - score) // 5, reverse=rev ^ flip, mapq=mapq, flags=0)


@pytest.mark.parametrize("max_occ", [None, SI.CAP], ids=["hash", "sorted"])
@pytest.mark.parametrize("case", list(EXPECT))
def test_hand_worked_cases(ref, case, max_occ):
    """the read as drawn and its reverse complement: the same pieces with the same segments in the hits' orientation, on the other strand"""
    for flip in (0, 1):
        s = revcomp(SI.read(case)) if flip else SI.read(case)
        p, m = EXPECT[case]
        if case == "m-twocopy" and flip:   # the copy on the other strand is the forward one now
            m = ("B2", 0, 40, 40, 40, 0, 1)
        got = SM.align_split(ref, s, max_occ)
        assert got["primary"] == hit_of(ref, case, p, flip), (case, flip)
        assert got["mate"] == (hit_of(ref, case, m, flip) if m else dict(M.UNALIGNED, flags=0)), (case, flip)
        assert not got["overflow"] and not got["tie"]


def test_the_case_that_motivates_the_rule(ref):
    """50 | 50: the plain call reports one half with the other as its runner-up, MAPQ 0; the split call reports both at 60"""
    s = SI.read("mapq5050")
    plain = M.align(ref, s)
    assert (plain["score"], plain["second"], plain["mapq"]) == (50, 50, 0)
    got = SM.align_split(ref, s)
    assert got["primary"]["mapq"] == got["mate"]["mapq"] == 60
    assert {k: got["primary"][k] for k in M.FIELDS if k not in ("second", "mapq")} == {k: plain[k] for k in M.FIELDS if k not in ("second", "mapq")}


def test_no_mate_is_the_plain_call(ref):
    """no mate: the primary equals realign_model.align / realign_sorted_model.align_sorted in every field; too short, too long, unaligned: no mate"""
    n = 0
    for s in SI.all_queries()[0][:400] + ("ACGT" * 4, "ACGT" * 257, SI.read("ff")[:19]):
        for max_occ in (None, SI.CAP):
            got = SM.align_split(ref, s, max_occ)
            plain = M.align(ref, s) if max_occ is None else SRT.align_sorted(ref, s, max_occ)
            if got["mate"]["tid"] < 0:
                n += 1
                assert got["mate"] == dict(M.UNALIGNED, flags=plain.get("flags", 0))
                assert {k: got["primary"][k] for k in M.FIELDS} == {k: plain[k] for k in M.FIELDS}, s
            else:
                assert {k: got["primary"][k] for k in M.FIELDS if k not in ("second", "mapq")} == {k: plain[k] for k in M.FIELDS if k not in ("second", "mapq")}, s
    assert n > 100


def test_bam_records(ref):
    """the rows of `seeksv realign -P`: the read's name on both, the mate supplementary (2048), S M S of its own segment, full-length SEQ / QUAL of its strand"""
    s = SI.read("fr")
    q = "".join(chr(40 + i % 50) for i in range(100))
    rows = SM.bam_records("r1/2", s, q, SM.align_split(ref, s))
    a, b = SI.where("fr:A"), SI.where("fr:B") - ref.off[1]
    assert rows == [dict(name="r1/2", flag=0, tid=0, pos=a, mapq=60, cigar=[(60, "M"), (40, "S")], seq=s, qual=q),
                    dict(name="r1/2", flag=2048 | 16, tid=1, pos=b, mapq=60, cigar=[(40, "M"), (60, "S")], seq=revcomp(s), qual=q[::-1])]
    s = SI.read("gap10")
    rows = SM.bam_records("x", s, q, SM.align_split(ref, s))
    assert [(r["flag"], r["cigar"]) for r in rows] == [(0, [(55, "M"), (45, "S")]), (2048, [(65, "S"), (35, "M")])]
    s = SI.read("overlap5")
    rows = SM.bam_records("x", s, q, SM.align_split(ref, s))
    assert [(r["flag"], r["cigar"]) for r in rows] == [(0, [(60, "M"), (40, "S")]), (2048, [(55, "S"), (45, "M")])]
    s = SI.read("contained")
    rows = SM.bam_records("x", s, q, SM.align_split(ref, s))
    assert rows == [dict(M.bam_record(s, q, M.align(ref, s)), name="x")]
    rows = SM.bam_records("u", "ACGT" * 10, q[:40], SM.align_split(ref, "ACGT" * 10))
    assert rows == [dict(name="u", flag=4, tid=-1, pos=-1, mapq=0, cigar=[], seq="ACGT" * 10, qual=q[:40])]


# the base of each piece next to the breakpoint, 1-based: a forward piece in front ends there, behind begins there; a reverse piece the other way round
JUNCTIONS = {"ff": (("A", 60), ("B", 1)), "fr": (("A", 60), ("B", 40)), "rf": (("A", 1), ("B", 1)), "rr": (("A", 1), ("B", 40))}


@pytest.mark.parametrize("case", list(JUNCTIONS))
def test_rows_make_the_planted_junction(ref, case):
    """the model's rows through the read-through model's FindJunction at getsv's default -w 1: one pair, its two ends the planted ones - for the read as
    drawn and for its reverse complement.  The plain call's single row makes none."""
    want = set()
    for label, k in JUNCTIONS[case]:
        g = SI.where(f"{case}:{label}")
        tid = ref.contig_of(g)
        want.add((SI.NAMES[tid], g - ref.off[tid] + k))
    for s in (SI.read(case), revcomp(SI.read(case))):
        rows = SM.bam_records("r", s, "I" * len(s), SM.align_split(ref, s))
        recs = [dict(qname=r["name"], flag=r["flag"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar="".join(f"{n}{op}" for n, op in r["cigar"]), seq=r["seq"]) for r in rows]
        batch, names = RT.batch_from_records(recs)
        pairs, n_cand = RT.find_junction([batch], [names], 1, list(SI.NAMES))
        assert n_cand == 2 and len(pairs) == 1
        key = pairs[0]["key"]
        assert {(key[0], key[1]), (key[3], key[4])} == want and pairs[0]["microhomology"] == 0, (case, key, want)
        batch, names = RT.batch_from_records(recs[:1])
        assert RT.find_junction([batch], [names], 1, list(SI.NAMES))[0] == []
