"""The re-aligner's alternate loci (ssv_realign_query_alts, `seeksv realign -S`) in plain Python, from the rule of DESIGN.md 10d and the contract in
include/seeksv_hip.h.  The candidates, their scores and the primary are those of tests/realign_model.py (hash index), realign_sorted_model.py (sorted
index) and realign_gapped_model.py (the first stage with its floor at 20, and the refinement); only the rule is written out here:

best        the primary's first-stage score (gapped: before the refinement).
qualifies   a scored candidate with score >= 30 and 5 * score >= 4 * best.
same locus  same strand, same contig, diagonals at most 32 apart.
choice      candidates in the order (score descending, strand 0 first, diagonal ascending, contig ascending); one is taken unless it is the locus of the
            primary or of an alternate taken before it.  At most max_alt are taken; one more that would have been: the flag ALT_CUT (4) on the primary
            and on every alternate.
alternate   tid, pos, q_beg, q_end, score, n_mismatch, reverse of its own candidate; second = best; mapq = 0; flags = the primary's.
none        for an unaligned primary (too short, too long, below 30, or left unaligned by the refinement): no alternates, no ALT_CUT."""
import realign_gapped_model as GM
import realign_model as M
import realign_sorted_model as SM
from realign_model import FIELDS, LOCUS, MIN_SCORE, orientations  # noqa: F401

F_ALT_CUT = 4
MAX_ALT = 16
NUM, DEN = 5, 4


def same_locus(a, b):
    """a, b: (strand, tid, diag)"""
    return a[0] == b[0] and a[1] == b[1] and abs(a[2] - b[2]) <= LOCUS


def scored_candidates(ref, query, max_occ=None, gapped=False):
    """the first stage's scored candidates -> [(score, strand, diag, tid, q_beg, q_end, n_mismatch)] in the alternates' order"""
    per, _, _ = GM.candidates(ref, query, max_occ)
    ori = orientations(query)
    out = []
    for diag, st, tid in per:
        r = GM.local_candidate(ref, ori[st], diag, tid, GM.FLOOR if gapped else MIN_SCORE)
        if r:
            out.append((r[0], st, diag, tid, r[1], r[2], r[3]))
    out.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
    return out


def choose(cands, primary, best, max_alt):
    """cands: (score, strand, diag, tid, ...) in any order; primary: (strand, tid, diag) -> (the chosen candidates in order, cut)"""
    taken, chosen, cut = [primary], [], False
    for c in sorted(cands, key=lambda c: (-c[0], c[1], c[2], c[3])):
        if c[0] < MIN_SCORE or NUM * c[0] < DEN * best or any(same_locus((c[1], c[3], c[2]), t) for t in taken):
            continue
        if len(chosen) == max_alt:
            cut = True
            break
        chosen.append(c)
        taken.append((c[1], c[3], c[2]))
    return chosen, cut


_refined = {}   # (reference, coded query, winner) -> realign_gapped_model.refine(): the same on either index whenever the first stage's winner is


def _gapped_hit(ref, query, w, flags):
    """realign_gapped_model.align_gapped from its first stage's winner w on (tests/test_realign_alts_model.py holds the two against each other); the
    refinement - the slow part, and a function of the winner alone - is computed once per winner"""
    out = dict(M.UNALIGNED, flags=flags, gap_at=0, gap_len=0)
    if w is None:
        return out
    s = orientations(query)[w["st"]]
    key = (id(ref), s, tuple(sorted(w.items())))
    if key not in _refined:
        _refined[key] = GM.refine(ref, s, w)
    r = _refined[key]
    c_lo = ref.off[w["tid"]]
    hit = dict(tid=w["tid"], pos=w["diag"] + w["q_beg"] - c_lo, q_beg=w["q_beg"], q_end=w["q_end"], score=w["score"], second=w["second"],
               n_mismatch=w["n_mismatch"], reverse=w["st"], mapq=M.mapq_of(w["score"], w["second"]), gap_at=0, gap_len=0)
    if r:
        mm = sum(1 for i in range(r["b"], r["k"]) if GM.sval(ref, s, i, r["dl"]) < 0) + sum(1 for i in range(r["j"], r["e"]) if GM.sval(ref, s, i, r["dr"]) < 0)
        hit.update(pos=r["dl"] + r["b"] - c_lo, q_beg=r["b"], q_end=r["e"], score=r["J"], n_mismatch=mm, mapq=M.mapq_of(r["J"], w["second"]),
                   gap_at=r["k"], gap_len=r["L"] if r["kind"] == "D" else -r["L"])
    if hit["score"] >= MIN_SCORE:
        out.update(hit)
    return out


def align_alts(ref, query, max_alt, max_occ=None, gapped=False):
    """-> dict(primary, alts, overflow, tie).  primary: FIELDS + flags (+ gap_at, gap_len when gapped); alts: [FIELDS + flags].  overflow / tie: the hash
    index's undetermined classes - more seeds than slots; another candidate equal to the primary in score, strand and diagonal"""
    assert 1 <= max_alt <= MAX_ALT
    w, flags, overflow, _ = GM.first_stage(ref, query, max_occ, GM.FLOOR if gapped else MIN_SCORE)
    if gapped:
        full = _gapped_hit(ref, query, w, flags)
        primary = {k: full[k] for k in FIELDS + ("flags",) + GM.GAP_FIELDS}
    else:   # (not put together from w: the ungapped `second` also counts a candidate that its end extension took below 30, first_stage's does not)
        full = M.align(ref, query) if max_occ is None else SM.align_sorted(ref, query, max_occ)
        primary = dict({k: full[k] for k in FIELDS}, flags=full.get("flags", 0))
        assert (w is None) == (full["tid"] < 0) and (w is None or (w["tid"], w["st"], w["score"], w["q_beg"], w["q_end"]) == (full["tid"], full["reverse"], full["score"], full["q_beg"], full["q_end"]))
    out = dict(primary=primary, alts=[], overflow=overflow, tie=False)
    if w is None:
        return out
    cands = scored_candidates(ref, query, max_occ, gapped)
    out["tie"] = sum(1 for c in cands if (c[0], c[1], c[2]) == (w["score"], w["st"], w["diag"])) > 1
    if primary["tid"] < 0:
        return out
    chosen, cut = choose(cands, (w["st"], w["tid"], w["diag"]), w["score"], max_alt)
    if cut:
        primary["flags"] |= F_ALT_CUT
    for score, st, diag, tid, qb, qe, mm in chosen:
        out["alts"].append(dict(tid=tid, pos=diag + qb - ref.off[tid], q_beg=qb, q_end=qe, score=score, second=w["score"], n_mismatch=mm, reverse=st, mapq=0,
                                flags=primary["flags"]))
    return out


def bam_records(query, qual, res, gapped=False):
    """the rows `seeksv realign -S` writes for one FASTQ entry: the primary's record (realign_model / realign_gapped_model bam_record), then one secondary
    record per alternate in order: flag 256 | 16 on the reverse strand, MAPQ 0, CIGAR S M S, SEQ / QUAL as a primary on that strand carries them"""
    rows = [GM.bam_record(query, qual, res["primary"]) if gapped else M.bam_record(query, qual, res["primary"])]
    for a in res["alts"]:
        r = M.bam_record(query, qual, a)
        r["flag"] |= 256
        rows.append(r)
    return rows
