"""Two-piece split alignments of whole reads (ssv_realign_query_split, `seeksv realign -P`) in plain Python, from the rule of DESIGN.md 10f and the
contract in include/seeksv_hip.h.  The candidates, their scores and segments and the primary P are those of tests/realign_model.py (hash index) and
realign_sorted_model.py (sorted index) through realign_alts_model.scored_candidates; only the rule is written out here:

intervals   in the READ's orientation: a candidate with segment [b, e) is [b, e) on strand 0 and [n - e, n - b) on strand 1.
            shared(X, Y) = the length of the intersection of the two intervals, 0 when they are disjoint.
mate        a scored candidate C with another (strand, contig, diagonal) than P, score >= 30, ordered against P (P begins before C begins and ends
            before C ends, or the reverse), len(P) - shared >= 20 and len(C) - shared >= 20.  Of several: score descending, strand 0 first, diagonal
            ascending, contig ascending.
second      with a mate, of X in {P, M}: the largest score among the scored candidates that are not X's locus (same strand, same contig, diagonals at
            most 32 apart), are not the other piece and have shared(C, X) >= 20; 0 when there is none.  mapq = mapq_of(score, second).
none        no mate: the primary is realign_model.align / realign_sorted_model.align_sorted in every field and the mate is unaligned with the
            primary's flags."""
import realign_model as M
import realign_sorted_model as SM
from realign_alts_model import same_locus, scored_candidates
from realign_model import FIELDS, K, MIN_SCORE, UNALIGNED, mapq_of

OWN = K   # bases a piece keeps for itself; also the overlap from which a candidate competes with a piece


def interval(n, c):
    """c: (score, strand, diag, tid, q_beg, q_end, ...) -> (begin, end) in the read's orientation"""
    return (n - c[5], n - c[4]) if c[1] else (c[4], c[5])


def shared(x, y):
    return max(0, min(x[1], y[1]) - max(x[0], y[0]))


def ordered(x, y):
    return (x[0] < y[0] and x[1] < y[1]) or (y[0] < x[0] and y[1] < x[1])


def qualifies(n, p, c):
    """can candidate c be the mate of the primary's candidate p?"""
    if c[0] < MIN_SCORE or (c[1], c[3], c[2]) == (p[1], p[3], p[2]):
        return False
    ip, ic = interval(n, p), interval(n, c)
    sh = shared(ip, ic)
    return ordered(ip, ic) and ip[1] - ip[0] - sh >= OWN and ic[1] - ic[0] - sh >= OWN


def second_of(n, cands, x, partner):
    ix = interval(n, x)
    return max([c[0] for c in cands if c is not partner and c is not x and not same_locus((c[1], c[3], c[2]), (x[1], x[3], x[2])) and shared(interval(n, c), ix) >= OWN],
               default=0)


def align_split(ref, query, max_occ=None):
    """-> dict(primary, mate, overflow, tie): primary and mate FIELDS + flags; overflow / tie: the hash index's undetermined classes (realign_model)"""
    full = M.align(ref, query) if max_occ is None else SM.align_sorted(ref, query, max_occ)
    flags = full.get("flags", 0)
    primary = dict({k: full[k] for k in FIELDS}, flags=flags)
    out = dict(primary=primary, mate=dict(UNALIGNED, flags=flags), overflow=bool(full.get("overflow", False)), tie=bool(full.get("tie", False)))
    if primary["tid"] < 0:
        return out
    n = len(query)
    cands = scored_candidates(ref, query, max_occ)   # in the order that also chooses between mates
    mine = [c for c in cands if (c[0], c[1], c[3], c[2] + c[4] - ref.off[c[3]]) == (primary["score"], primary["reverse"], primary["tid"], primary["pos"]) and
            (c[4], c[5]) == (primary["q_beg"], primary["q_end"])]
    p = mine[0]   # (more than one: the `tie` class)
    mates = [c for c in cands if qualifies(n, p, c)]
    if not mates:
        return out
    m = mates[0]
    sp, sm = second_of(n, cands, p, m), second_of(n, cands, m, p)
    primary.update(second=sp, mapq=mapq_of(p[0], sp))
    out["mate"] = dict(tid=m[3], pos=m[2] + m[4] - ref.off[m[3]], q_beg=m[4], q_end=m[5], score=m[0], second=sm, n_mismatch=m[6], reverse=m[1], mapq=mapq_of(m[0], sm),
                       flags=flags)
    return out


def bam_records(name, query, qual, res):
    """the rows `seeksv realign -P` writes for one FASTQ entry: the primary's record as the plain mode writes it, then - when there is a mate - a supplementary
    record: flag 2048 | 16 on the reverse strand, its own MAPQ, CIGAR S M S, full-length SEQ / QUAL of its own strand.  Every row carries the read's name."""
    rows = [dict(M.bam_record(query, qual, res["primary"]), name=name)]
    if res["mate"]["tid"] >= 0:
        r = dict(M.bam_record(query, qual, res["mate"]), name=name)
        r["flag"] |= 2048
        rows.append(r)
    return rows
