"""The re-aligner on its SORTED index (ssv_realign_index_sorted + ssv_realign_query) in plain Python, from the contract in include/seeksv_hip.h and
the header comment of seeksv_amd/csrc/realign_sorted_kernels.h.  Coding of both orientations, score_candidate, the winner's order, the `second` rule,
the MAPQ ladder and pos are tests/realign_model.py's; only the seed set is new:

look-up    every all-ACGT query 20-mer, both strands, every offset: occ = its occurrences among the indexed positions.  occ == 0: no seed.
           occ > max_occ: the 20-mer is masked - no seed, flag MASKED.  Else it belongs to class ceil(log2(occ)) (class 0: occ == 1).
admission  seeds are ordered by (class, strand, query offset, reference position) and the first 192 are followed; any left out: flag OVERFLOW.
ties       candidates equal in (score, strand, diagonal) go to the smaller contig id.

Nothing is left to the kernel: align_sorted() has no `overflow` / `tie` class, every field and the flags are compared."""
from realign_model import FIELDS, K, MAX_CAND, MAX_Q, MIN_Q, MIN_SCORE, LOCUS, UNALIGNED, Reference, check_hit, mapq_of, orientations, score_candidate  # noqa: F401

F_MASKED, F_OVERFLOW = 1, 2


def index_stats(ref, max_occ):
    """ssv_realign_index_stats of a realign_model.Reference"""
    runs = [len(v) for v in ref.index.values()]
    return dict(n_indexed=sum(runs), n_distinct=len(runs), occ_max=max(runs, default=0), n_over_cap=sum(1 for r in runs if r > max_occ))


def occ_class(occ):
    """ceil(log2(occ))"""
    return (occ - 1).bit_length()


def align_sorted(ref, query, max_occ):
    """-> dict of FIELDS + flags, n_admitted, n_masked_kmers"""
    out = dict(UNALIGNED, flags=0, n_admitted=0, n_masked_kmers=0)
    if not MIN_Q <= len(query) <= MAX_Q:
        return out
    ori = orientations(query)
    seeds = []   # (class, strand, offset, position)
    for st, s in enumerate(ori):
        for o in range(len(s) - K + 1):
            km = s[o:o + K]
            if "." in km:
                continue
            run = ref.index.get(km, ())   # positions ascend (Reference walks the text from its start)
            if len(run) > max_occ:
                out["n_masked_kmers"] += 1
            else:
                seeds.extend((occ_class(len(run)), st, o, p) for p in run)
    seeds.sort()
    admitted = seeds[:MAX_CAND]
    out["n_admitted"] = len(admitted)
    out["flags"] = (F_MASKED if out["n_masked_kmers"] else 0) | (F_OVERFLOW if len(seeds) > MAX_CAND else 0)
    scored = []
    for diag, st, tid in sorted({(p - o, st, ref.contig_of(p)) for _, st, o, p in admitted}):
        r = score_candidate(ref, ori[st], diag, tid)
        if r:
            scored.append((-r[0], st, diag, tid, r))
    if not scored:
        return out
    scored.sort()   # score, strand, diagonal, contig
    _, st, diag, tid, (score, qb, qe, mm) = scored[0]
    if score < MIN_SCORE:
        return out
    second = max([-c[0] for c in scored[1:] if not (c[1] == st and c[3] == tid and abs(c[2] - diag) <= LOCUS)], default=0)
    out.update(tid=tid, pos=diag + qb - ref.off[tid], q_beg=qb, q_end=qe, score=score, second=second, n_mismatch=mm, reverse=st, mapq=mapq_of(score, second))
    return out
