"""The gapped re-aligner (ssv_realign_query_gapped, `seeksv realign -g`) in plain Python, from the rule of DESIGN.md 10c and the contract in
include/seeksv_hip.h.  Reference, seeds() and mapq_of() are tests/realign_model.py's; everything else is written out here.

first stage   as realign_model / realign_sorted_model, with the candidate floor at K = 20 instead of 30: a candidate whose best local segment scores
              20 or more is kept and extended, and a winner (score, then strand 0, then the smaller diagonal, then the smaller contig) at 20 or
              more goes on.  `second` counts only the other loci's candidates that score 30 or more.
refinement    of the winner only: strand, contig [c_lo, c_hi), diagonal d, segment [q_beg, q_end), score.  s(i, D) = +1 when query base i is a
              base and equals the reference at D + i, else -4; a piece covers only query positions whose reference position is inside the contig.
              64 variants = {D, I} x L = 1..16 x {the winner is the left piece, the winner is the right piece}; g = +L (D) / -L (I); the left
              piece is query [b, k) on dl, the right piece [j, e) on dr = dl + g, j = k (D) or k + L (I).
              winner left:  dl = d, b = q_beg, every k > q_beg with j <= n - 1; left = sum s(i, d) over [q_beg, k); right = the best segment on dr
                            that starts exactly at j (the shortest of equal ones), run on to n when n is reachable inside the contig and the sum
                            over [j, n) is > best - 5.
              winner right: dr = d, e = q_end, every j < q_end with k >= 1; right = sum s(i, d) over [j, q_end); left = the best segment on dl that
                            ends exactly at k (the shortest of equal ones), run on to 0 when 0 is reachable and the sum over [0, k) is > best - 5.
              J = left + right - (6 + L).  Inside a variant the largest J, then the smallest k.  Across variants the largest J, then the smaller L,
              then D before I, then winner-left before winner-right.  Accepted only when J > score.
result        pos = the left piece's first reference base, q_beg = b, q_end = e, score = J, n_mismatch over both pieces (inserted bases do not
              count), mapq from the new score and the unchanged second; tid, reverse, second and the flags stay.  A hit below 30 after the
              refinement is unaligned in every field but the flags.  gap_at = k, gap_len = +L (D) / -L (I) / 0."""
from itertools import accumulate

from realign_model import FIELDS, K, LOCUS, MAX_CAND, MAX_Q, MIN_Q, MIN_SCORE, UNALIGNED, Reference, mapq_of, orientations, seeds  # noqa: F401
from realign_sorted_model import F_MASKED, F_OVERFLOW, occ_class

MATCH, MISMATCH, CLIP = 1, 4, 5
GAP_OPEN, GAP_EXT, MAX_GAP = 6, 1, 16
FLOOR = K
GAP_FIELDS = ("gap_at", "gap_len")


def sval(ref, s, i, diag):
    return MATCH if s[i] == ref.text[diag + i] else -MISMATCH   # '.' equals no base


def local_candidate(ref, s, diag, tid, floor):
    """realign_model.score_candidate with the floor as a parameter -> (score, q_beg, q_end, n_mismatch) or None"""
    n = len(s)
    c_lo, c_hi = ref.off[tid], ref.off[tid + 1]
    i_lo, i_hi = max(c_lo - diag, 0), min(c_hi - diag, n)
    if i_hi - i_lo < K:
        return None
    val = {i: sval(ref, s, i, diag) for i in range(i_lo, i_hi)}
    run, run_beg, bs, bb, be = 0, i_lo, 0, i_lo, i_lo
    for i in range(i_lo, i_hi):
        if run <= 0:
            run, run_beg = 0, i
        run += val[i]
        if run > bs:
            bs, bb, be = run, run_beg, i + 1
    if bs < floor:
        return None
    head, tail = sum(val[i] for i in range(i_lo, bb)), sum(val[i] for i in range(be, i_hi))
    if i_lo == 0 and head > -CLIP:
        bs, bb = bs + head, 0
    if i_hi == n and tail > -CLIP:
        bs, be = bs + tail, n
    return bs, bb, be, sum(1 for i in range(bb, be) if val[i] < 0)


def candidates(ref, query, max_occ):
    """the first stage's candidate set -> (set of (diag, strand, tid), flags, overflow).  max_occ None: the hash index (every seed; `overflow` as
    realign_model.align has it), else the sorted index's admission (realign_sorted_model)"""
    if not MIN_Q <= len(query) <= MAX_Q:
        return set(), 0, False
    if max_occ is None:
        sd = seeds(ref, query)
        per = {(p - o, st, ref.contig_of(p)) for st, o, p in sd}
        return per, 0, len(sd) > MAX_CAND and len(per) > 1
    sd, masked = [], False
    for st, s in enumerate(orientations(query)):
        for o in range(len(s) - K + 1):
            km = s[o:o + K]
            if "." in km:
                continue
            run = ref.index.get(km, ())
            if len(run) > max_occ:
                masked = True
            else:
                sd.extend((occ_class(len(run)), st, o, p) for p in run)
    sd.sort()
    per = {(p - o, st, ref.contig_of(p)) for _, st, o, p in sd[:MAX_CAND]}
    return per, (F_MASKED if masked else 0) | (F_OVERFLOW if len(sd) > MAX_CAND else 0), False


def first_stage(ref, query, max_occ=None, floor=FLOOR):
    """-> (winner or None, flags, overflow, tie); winner = dict(st, tid, diag, q_beg, q_end, score, second, n_mismatch)"""
    per, flags, overflow = candidates(ref, query, max_occ)
    ori = orientations(query)
    scored = []
    for diag, st, tid in per:
        r = local_candidate(ref, ori[st], diag, tid, floor)
        if r:
            scored.append((-r[0], st, diag, tid, r))
    scored.sort()
    tie = any(a[:3] == b[:3] for a, b in zip(scored, scored[1:]))
    if not scored or -scored[0][0] < floor:
        return None, flags, overflow, tie
    _, st, diag, tid, (score, qb, qe, mm) = scored[0]
    second = max([-c[0] for c in scored[1:] if -c[0] >= MIN_SCORE and not (c[1] == st and c[3] == tid and abs(c[2] - diag) <= LOCUS)], default=0)
    return dict(st=st, tid=tid, diag=diag, q_beg=qb, q_end=qe, score=score, second=second, n_mismatch=mm), flags, overflow, tie


def svals(ref, s, diag, lo, hi):
    """[s(i, diag) for i in [lo, hi)]"""
    return [MATCH if a == b else -MISMATCH for a, b in zip(s[lo:hi], ref.text[diag + lo:diag + hi])]


def peak(vals):
    """the largest sum of a stretch of vals (0 for none): no segment on this diagonal scores more"""
    C = list(accumulate(vals, initial=0))
    return max(c - low for c, low in zip(C, accumulate(C, min)))


def table_from(ref, s, diag, c_lo, c_hi):
    """{j: (score, e)}: the best segment [j, e) on diag that starts exactly at j, for every j whose base lies inside the contig.  With C the sums
    of s(x, diag) from the first such base on, it is the largest C[e] - C[j] over e > j and, of equal ones, the smallest e"""
    n = len(s)
    lo, hi = max(0, c_lo - diag), min(n, c_hi - diag)
    C = dict(zip(range(lo, hi + 1), accumulate(svals(ref, s, diag, lo, hi), initial=0)))
    out, top, arg = {}, None, None
    for j in range(hi - 1, lo - 1, -1):
        if top is None or C[j + 1] >= top:
            top, arg = C[j + 1], j + 1
        best, total = top - C[j], C[hi] - C[j]
        out[j] = (total, n) if hi == n and total > best - CLIP else (best, arg)
    return out


def table_to(ref, s, diag, c_lo, c_hi):
    """{k: (score, b)}: the mirror image, the best segment [b, k) on diag that ends exactly at k: the largest C[k] - C[b] over b < k and, of equal
    ones, the largest b"""
    n = len(s)
    lo, hi = max(0, c_lo - diag), min(n, c_hi - diag)
    C = dict(zip(range(lo, hi + 1), accumulate(svals(ref, s, diag, lo, hi), initial=0)))
    out, low, arg = {}, None, None
    for k in range(lo + 1, hi + 1):
        if low is None or C[k - 1] <= low:
            low, arg = C[k - 1], k - 1
        best, total = C[k] - low, C[k] - C[lo]
        out[k] = (total, 0) if lo == 0 and total > best - CLIP else (best, arg)
    return out


def variants():
    """in the order that decides between equal scores: the smaller L, D before I, winner-left before winner-right"""
    for L in range(1, MAX_GAP + 1):
        for kind in "DI":
            for side in ("left", "right"):
                yield L, kind, side


def refine(ref, s, w):
    """the refinement of the winner w (first_stage) of the coded query s -> None or dict(J, L, kind, side, b, k, j, e, dl, dr)"""
    n = len(s)
    d, qb, qe = w["diag"], w["q_beg"], w["q_end"]
    c_lo, c_hi = ref.off[w["tid"]], ref.off[w["tid"] + 1]
    i_lo, i_hi = max(c_lo - d, 0), min(c_hi - d, n)
    pre = dict(zip(range(i_lo, i_hi + 1), accumulate(svals(ref, s, d, i_lo, i_hi), initial=0)))   # pre[i] = sum of s(x, d) over [i_lo, i)
    most = dict(left=max(pre[k] - pre[qb] for k in range(qb + 1, i_hi + 1)), right=max(pre[qe] - pre[j] for j in range(i_lo, qe)))
    best = None
    for L, kind, side in variants():
        g = L if kind == "D" else -L
        ins = L if kind == "I" else 0
        top = None
        d2 = d + g if side == "left" else d - g
        lo2, hi2 = max(0, c_lo - d2), min(n, c_hi - d2)
        if most[side] + peak(svals(ref, s, d2, lo2, max(lo2, hi2))) - (GAP_OPEN + GAP_EXT * L) <= w["score"]:
            continue   # (only to save time: neither piece can score more than this, so no J of this variant could be accepted)
        if side == "left":
            dl, dr = d, d + g
            tab = table_from(ref, s, dr, c_lo, c_hi)
            for k in range(qb + 1, i_hi + 1):   # the left piece [q_beg, k) stays inside the contig
                j = k + ins
                if j > n - 1:
                    break
                r = tab.get(j)
                if r is None:
                    continue
                J = pre[k] - pre[qb] + r[0] - (GAP_OPEN + GAP_EXT * L)
                if top is None or J > top["J"]:
                    top = dict(J=J, L=L, kind=kind, side=side, b=qb, k=k, j=j, e=r[1], dl=dl, dr=dr)
        else:
            dl, dr = d - g, d
            tab = table_to(ref, s, dl, c_lo, c_hi)
            for j in range(max(i_lo, 1 + ins), qe):   # the right piece [j, q_end) stays inside the contig; k >= 1
                k = j - ins
                r = tab.get(k)
                if r is None:
                    continue
                J = r[0] + pre[qe] - pre[j] - (GAP_OPEN + GAP_EXT * L)
                if top is None or J > top["J"]:
                    top = dict(J=J, L=L, kind=kind, side=side, b=r[1], k=k, j=j, e=qe, dl=dl, dr=dr)
        if top and (best is None or top["J"] > best["J"]):
            best = top
    return best if best and best["J"] > w["score"] else None


def align_gapped(ref, query, max_occ=None):
    """-> dict of FIELDS + flags, gap_at, gap_len, side (which piece the winner became: "left", "right" or None), overflow, tie (the last two: the
    hash index's undetermined classes, as realign_model.align)"""
    w, flags, overflow, tie = first_stage(ref, query, max_occ)
    out = dict(UNALIGNED, flags=flags, gap_at=0, gap_len=0, side=None, overflow=overflow, tie=tie)
    if w is None:
        return out
    s = orientations(query)[w["st"]]
    c_lo = ref.off[w["tid"]]
    hit = dict(tid=w["tid"], pos=w["diag"] + w["q_beg"] - c_lo, q_beg=w["q_beg"], q_end=w["q_end"], score=w["score"], second=w["second"],
               n_mismatch=w["n_mismatch"], reverse=w["st"], mapq=mapq_of(w["score"], w["second"]))
    gap = dict(gap_at=0, gap_len=0)
    r = refine(ref, s, w)
    if r:
        mm = sum(1 for i in range(r["b"], r["k"]) if sval(ref, s, i, r["dl"]) < 0) + sum(1 for i in range(r["j"], r["e"]) if sval(ref, s, i, r["dr"]) < 0)
        hit.update(pos=r["dl"] + r["b"] - c_lo, q_beg=r["b"], q_end=r["e"], score=r["J"], n_mismatch=mm, mapq=mapq_of(r["J"], w["second"]))
        gap = dict(gap_at=r["k"], gap_len=r["L"] if r["kind"] == "D" else -r["L"], side=r["side"])
    if hit["score"] < MIN_SCORE:
        return out
    out.update(hit)
    out.update(gap)
    return out


def cigar_of(n, hit):
    """[(len, op)] of a gapped hit of an n-base query, in reference order (the hit's own orientation)"""
    if hit["tid"] < 0:
        return []
    k, L = hit["gap_at"], hit["gap_len"]
    if L == 0:
        cig = [(hit["q_beg"], "S"), (hit["q_end"] - hit["q_beg"], "M"), (n - hit["q_end"], "S")]
    else:
        j = k if L > 0 else k - L
        cig = [(hit["q_beg"], "S"), (k - hit["q_beg"], "M"), (abs(L), "D" if L > 0 else "I"), (hit["q_end"] - j, "M"), (n - hit["q_end"], "S")]
    return [c for c in cig if c[0] > 0]


def bam_record(query, qual, hit):
    """the record `seeksv realign -g` writes (realign_model.bam_record with the gap in the CIGAR)"""
    n = len(query)
    al = hit["tid"] >= 0
    rev = al and bool(hit["reverse"])
    fwd, rc = orientations(query)
    return dict(flag=(16 if rev else 0) if al else 4, tid=hit["tid"] if al else -1, pos=hit["pos"] if al else -1, mapq=hit["mapq"] if al else 0,
                cigar=cigar_of(n, hit), seq=(rc if rev else fwd).replace(".", "N"), qual=qual[::-1] if rev else qual)
