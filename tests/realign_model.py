"""The clipped-sequence re-aligner (ssv_realign_*) in plain Python: strings, dicts and ints; no hash table, no lanes, no candidate array.

Written from the contract in include/seeksv_hip.h and the header comment of seeksv_amd/csrc/realign_kernels.h:

index    every global position p of the concatenated contigs with p % 4 == 0 whose 20-mer lies inside one contig.
query    shorter than 20 or longer than 1024: unaligned (tid = pos = -1, everything else 0).  Both orientations are coded: A C G T in either
         case are bases, any other byte never matches, and neither does its complement.  A seed is (strand, query offset o, p) with an all-ACGT
         query 20-mer equal to the reference at an indexed p; its candidate is (diag = p - o, strand, contig of p).
score    per distinct candidate: the query positions inside the candidate's contig are [i_lo, i_hi), fewer than 20: skipped.  Best segment
         under +1 / -4 (the running sum restarts where it is <= 0, the maximum is strict: the earliest maximum wins), below 30: skipped.
         The segment is extended to query end 0 when i_lo == 0 and the sum over [0, q_beg) is > -5, to end n when i_hi == n and the sum over
         [q_end, n) is > -5 (cheaper than the clipping penalty).  n_mismatch is counted over the final segment.  An extension can take a
         candidate below 30 again (30 matches and a mismatch on the last base: 26): it stays a candidate, but a winner below 30 is not reported.
winner   highest score, then strand 0 before strand 1, then the smaller diagonal.  second = the highest score among the scored candidates that
         are not the winner's locus (same strand, same contig, |diag difference| <= 32), 0 when there is none.  mapq = 0 when second >= score,
         60 when the gap is >= 10, else max(6 * gap, 1).  pos = diag + q_beg - the contig's offset.

Two flags say where the kernel's answer is not determined by this description: `overflow` (more than 192 seeds, not all on one candidate: the
kernel follows the 192 it happened to keep) and `tie` (two scored candidates equal in score, strand and diagonal: which contig wins is the
kernel's order).  check_hit() is what holds for any hit whatever candidates were kept."""
import bisect

import numpy as np

K = 20
SAMPLE = 4
MIN_Q, MAX_Q = K, 1024
MAX_CAND = 192
MAX_PROBE = 256
MATCH, MISMATCH, CLIP, MIN_SCORE = 1, 4, 5, 30
LOCUS = 32

FIELDS = ("tid", "pos", "q_beg", "q_end", "score", "second", "n_mismatch", "reverse", "mapq")
UNALIGNED = dict(tid=-1, pos=-1, q_beg=0, q_end=0, score=0, second=0, n_mismatch=0, reverse=0, mapq=0)
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", ".": "."}


def pack_2bit(contigs):
    """contig strings (ACGT, either case) -> (uint64 words with one word of slack, target_off): base i at bits [2 (i % 32), +2) of word i / 32"""
    text = "".join(contigs).upper()
    assert set(text) <= set("ACGT")
    lut = np.zeros(256, np.uint64)
    lut[[ord(c) for c in "ACGT"]] = [0, 1, 2, 3]
    n_words = (len(text) + 31) // 32 + 1
    codes = np.zeros(n_words * 32, np.uint64)
    codes[:len(text)] = lut[np.frombuffer(text.encode(), np.uint8)]
    words = np.bitwise_or.reduce(codes.reshape(n_words, 32) << (2 * np.arange(32, dtype=np.uint64)), axis=1)
    off = [0]
    for c in contigs:
        off.append(off[-1] + len(c))
    return np.ascontiguousarray(words, np.uint64), np.array(off, dtype=np.int64)


class Reference:
    def __init__(self, contigs):
        self.contigs = [c.upper() for c in contigs]
        assert all(set(c) <= set("ACGT") for c in self.contigs)
        self.text = "".join(self.contigs)
        self.off = [0]
        for c in self.contigs:
            self.off.append(self.off[-1] + len(c))
        self.index = {}
        self.n_sampled = 0
        for p in range(0, len(self.text) - K + 1, SAMPLE):
            if p + K <= self.off[self.contig_of(p) + 1]:
                self.index.setdefault(self.text[p:p + K], []).append(p)
                self.n_sampled += 1

    def contig_of(self, p):
        """the contig that holds global position p (empty contigs hold nothing)"""
        return bisect.bisect_right(self.off, p) - 1


def orientations(query):
    """the query as the kernel codes it: (forward, reverse complement), upper-case bases, '.' for anything that never matches"""
    fwd = "".join(ch.upper() if ch in "ACGTacgt" else "." for ch in query)
    return fwd, "".join(_COMP[ch] for ch in reversed(fwd))


def seeds(ref, query):
    """[(strand, o, p)] in the order strand 0 first, then query offset"""
    out = []
    if not MIN_Q <= len(query) <= MAX_Q:
        return out
    for st, s in enumerate(orientations(query)):
        for o in range(len(s) - K + 1):
            km = s[o:o + K]
            if "." not in km:
                out.extend((st, o, p) for p in ref.index.get(km, ()))
    return out


def mapq_of(score, second):
    if second >= score:
        return 0
    gap = score - second
    return 60 if gap >= 10 else max(6 * gap, 1)


def score_candidate(ref, s, diag, tid):
    """-> (score, q_beg, q_end, n_mismatch) of the coded query s along diag inside contig tid, or None"""
    n = len(s)
    c_lo, c_hi = ref.off[tid], ref.off[tid + 1]
    i_lo, i_hi = max(c_lo - diag, 0), min(c_hi - diag, n)
    if i_hi - i_lo < K:
        return None
    val = [MATCH if s[i] == ref.text[diag + i] else -MISMATCH for i in range(i_lo, i_hi)]  # '.' equals no base
    run, run_beg, bs, bb, be = 0, i_lo, 0, i_lo, i_lo
    for i in range(i_lo, i_hi):
        if run <= 0:
            run, run_beg = 0, i
        run += val[i - i_lo]
        if run > bs:
            bs, bb, be = run, run_beg, i + 1
    if bs < MIN_SCORE:
        return None
    head, tail = sum(val[:bb - i_lo]), sum(val[be - i_lo:])
    if i_lo == 0 and head > -CLIP:
        bs, bb = bs + head, 0
    if i_hi == n and tail > -CLIP:
        bs, be = bs + tail, n
    return bs, bb, be, sum(1 for i in range(bb, be) if val[i - i_lo] < 0)


def align(ref, query):
    """-> dict of FIELDS + n_seeds, n_seeds_fwd, n_candidates, overflow, tie"""
    sd = seeds(ref, query)
    per = {}
    for st, o, p in sd:
        key = (p - o, st, ref.contig_of(p))
        per[key] = per.get(key, 0) + 1
    out = dict(UNALIGNED, n_seeds=len(sd), n_seeds_fwd=sum(1 for x in sd if x[0] == 0), n_candidates=len(per),
               overflow=len(sd) > MAX_CAND and len(per) > 1, tie=False)
    if not per:
        return out
    ori = orientations(query)
    scored = []
    for (diag, st, tid) in per:
        r = score_candidate(ref, ori[st], diag, tid)
        if r:
            scored.append((-r[0], st, diag, tid, r))
    if not scored:
        return out
    scored.sort()
    out["tie"] = any(a[:3] == b[:3] for a, b in zip(scored, scored[1:]))
    _, st, diag, tid, (score, qb, qe, mm) = scored[0]
    if score < MIN_SCORE:   # the floor holds for what is reported
        return out
    second = max([-c[0] for c in scored[1:] if not (c[1] == st and c[3] == tid and abs(c[2] - diag) <= LOCUS)], default=0)
    out.update(tid=tid, pos=diag + qb - ref.off[tid], q_beg=qb, q_end=qe, score=score, second=second, n_mismatch=mm, reverse=st, mapq=mapq_of(score, second))
    return out


def check_hit(ref, off, query, hit):
    """what holds for any hit of the kernel, whatever candidates it kept.  ref: the concatenated contigs (upper case), off: first base of every
    contig + total, hit: a mapping with FIELDS.  Raises AssertionError."""
    h = {k: int(hit[k]) for k in FIELDS}
    n = len(query)
    if h["tid"] == -1:
        assert h == UNALIGNED, h
        return
    assert MIN_Q <= n <= MAX_Q, (n, h)
    assert 0 <= h["tid"] < len(off) - 1 and h["reverse"] in (0, 1), h
    assert 0 <= h["q_beg"] < h["q_end"] <= n, h
    assert 0 <= h["pos"] and h["pos"] + h["q_end"] - h["q_beg"] <= off[h["tid"] + 1] - off[h["tid"]], h
    s = orientations(query)[h["reverse"]]
    g = int(off[h["tid"]]) + h["pos"]
    mm = sum(1 for i in range(h["q_beg"], h["q_end"]) if s[i] != ref[g + i - h["q_beg"]])
    assert h["n_mismatch"] == mm, (h, mm)
    assert h["score"] == (h["q_end"] - h["q_beg"] - mm) * MATCH - mm * MISMATCH, (h, mm)
    assert h["score"] >= MIN_SCORE, h
    assert 0 <= h["second"] <= h["score"], h
    assert h["mapq"] == mapq_of(h["score"], h["second"]), h


def bam_record(query, qual, hit):
    """the record `seeksv realign` writes for a FASTQ entry (read name = sequence): dict(flag, tid, pos, mapq, cigar=[(len, op)], seq, qual);
    SEQ reverse-complemented and QUAL reversed for reverse hits, anything but ACGT written as N, an unaligned record without CIGAR"""
    n = len(query)
    al = hit["tid"] >= 0
    rev = al and bool(hit["reverse"])
    fwd, rc = orientations(query)
    cig = []
    if al:
        cig = [(hit["q_beg"], "S"), (hit["q_end"] - hit["q_beg"], "M"), (n - hit["q_end"], "S")]
        cig = [c for c in cig if c[0] > 0]
    return dict(flag=(16 if rev else 0) if al else 4, tid=hit["tid"] if al else -1, pos=hit["pos"] if al else -1, mapq=hit["mapq"] if al else 0, cigar=cig,
                seq=(rc if rev else fwd).replace(".", "N"), qual=qual[::-1] if rev else qual)
