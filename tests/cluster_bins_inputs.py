"""Designed getclip samples for the consensus clustering walk (k_cluster_bins4 / k_cluster_bins and the bin lists around them): bins built so
that every place where the two kernels change path is reached on purpose, not by accident of a generator.  A sample is a list of record
dicts (the fields of test_random_differential_gpu.random_sample(..., want_records=True), plus `tag` and `ref`) and the batch made of them.

Families:
  a  threshold sweep: for every overlap n two-event bins whose second event matches in exactly minm(n) - 1 (new cluster) or minm(n) (joins)
     positions, once with the left and once with the right side deciding; one sample per match rate
  b  bins that end with exactly 1 .. 70 clusters, joiners aimed at the clusters where the storage changes, an event between an early and a
     late cluster, events that match only because a cluster grew or took a better base
  c  bins of exactly 2 .. 130 events; the first and the last slot of the sorted event list
  d  merge rules: side lengths 1 .. 5 and 255, equal against one longer, lone soft clips, both-end clips, no qualities
  e  per length class: 5 and 66 clusters of reads of that very length (and sides of 255 / 256 bases for the classes that hold them)
Every family is also given per length class with one extra clipped read of that length in the pass: the longest clipped read of a pass
decides the kernel (<= B4_CAP: k_cluster_bins4) and the storage paths of k_cluster_bins (LDS strings up to PACK_MAX_LQ, entries staged in
LDS up to BIN_ENT bytes).  Qualities stay within a valid BAM's 0 .. 93.
"""
import functools

import numpy as np

from cluster_bins_model import F_DUP, F_REV, OPS, _events_of, getclip_model, minm, rate_ok

# what the inputs rest on (seeksv_amd/csrc/clip_kernels.h and common.h; tests/test_cluster_bins_inputs.py compares them with the headers' lines)
CONSTANTS = dict(B4_CAP=256, B4_KLDS=3, BIN_KLDS=4, CL_CACHE=64, B4_DEEP=16, PACK_MAX_LQ=320, BIN_ENT=512, WAVE=64)
B4_CAP, B4_KLDS, BIN_KLDS, CL_CACHE, B4_DEEP, PACK_MAX_LQ, BIN_ENT, WAVE = (CONSTANTS[k] for k in ("B4_CAP", "B4_KLDS", "BIN_KLDS", "CL_CACHE", "B4_DEEP", "PACK_MAX_LQ", "BIN_ENT", "WAVE"))

QUALS = (0, 2, 9, 10, 40, 93)          # equal qualities meet often; 9 prints as '*'; 0 and 93 are the ends of the valid range
# (tag, the reference's flags, our parameters): seven match rates; 0.8 and 1 also move -q and -s like the other randomized tests
RUNS = (("t090", [], {}), ("t080", ["-t", "0.8", "-q", "0"], dict(match_rate=0.8, min_mapq=0)),
        ("t100", ["-s", "-q", "20", "-t", "1"], dict(match_rate=1.0, save_low_quality=True, min_mapq=20)),
        ("t055", ["-t", "0.55"], dict(match_rate=0.55)), ("t056", ["-t", "0.56"], dict(match_rate=0.56)), ("t068", ["-t", "0.68"], dict(match_rate=0.68)),
        ("t000", ["-t", "0"], dict(match_rate=0.0)))
RUN_KW = {tag: kw for tag, _, kw in RUNS}
CLASSES = (0, 256, 257, 320, 321, 337, 338, 339, 340, 341, 342, 400, 600)   # 0: the family as it is (no extra read)
SWEEP_OWN = {0: (B4_CAP - 1, B4_CAP), 257: (256, 257), 321: (320, 321)}      # class -> (longest overlap, longest read) of a sweep of its own
COUNTS = (1, 2, 3, 4, 5, 6, 63, 64, 65, 66, 70)
DEPTHS = (2, 15, 16, 17, 63, 64, 65, 66, 128, 129, 130)
SIDE_LENGTHS = (1, 2, 3, 4, 5, 255)   # of family d's merging bins (B4_CAP itself: see merge_sample)
CONTIG_LEN = 60000
NAMES = ["c0", "c1", "c2"]


def records_to_batch(recs):
    """record dicts -> a host batch (every record carries its bases and qualities)"""
    b = dict(tid=np.array([r["tid"] for r in recs], np.int32), pos=np.array([r["pos"] for r in recs], np.int32),
             flag=np.array([r["flag"] for r in recs], np.uint16), mapq=np.array([r["mapq"] for r in recs], np.uint8),
             n_cigar=np.array([len(r["ops"]) for r in recs], np.uint16), l_qseq=np.array([r["lq"] for r in recs], np.int32),
             mtid=np.array([r["mtid"] for r in recs], np.int32), mpos=np.array([r["mpos"] for r in recs], np.int32),
             isize=np.array([r["isize"] for r in recs], np.int32), xc=np.array([r["xc"] for r in recs], np.uint8))
    code = np.zeros(256, np.uint8)
    for ch, v in {"=": 0, "A": 1, "C": 2, "G": 4, "T": 8, "N": 15}.items():
        code[ord(ch)] = v
    cig, coff, soff, blob, nbytes, span = [], [], [], [], 0, 1
    for r in recs:
        coff.append(len(cig))
        cig += [(l << 4) | OPS.index(op) for l, op in r["ops"]]
        span = max(span, sum(l for l, op in r["ops"] if op in "MDN=X"))
        lq = r["lq"]
        c = code[np.frombuffer(r["seq"].encode(), np.uint8)]
        if lq & 1:
            c = np.concatenate([c, np.zeros(1, np.uint8)])
        soff.append(nbytes)
        blob += [(c[0::2] << 4) | c[1::2], np.asarray(r["qual"], np.uint8)]
        nbytes += (lq + 1) // 2 + lq
    b.update(cigar=np.array(cig, np.uint32), cigar_off=np.array(coff, np.uint32), seq_off=np.array(soff, np.uint64),
             seqqual=np.concatenate(blob + [np.zeros(16, np.uint8)]), max_ref_span=int(span))
    return b


def mutate(ch):
    return "CGTA"["ACGT".index(ch)] if ch in "ACGT" else "A"


class Builder:
    """collects records; strings are given RELATIVE TO THE BREAKPOINT: index 0 of a left and of a right side is the base next to it"""

    def __init__(self, seed, quals=QUALS):
        self.rng = np.random.RandomState(seed)
        self.recs, self.aims, self.expect, self.both = [], {}, {}, []
        self.quals = quals
        self.next_bp = [1000, 1000, 1000]
        self.placed = {}

    def bp(self, tid):
        self.next_bp[tid] += 3
        return self.next_bp[tid]

    def seq(self, n):
        return "".join("ACGTN"[x] for x in self.rng.choice(5, n, p=[0.2475, 0.2475, 0.2475, 0.2475, 0.01]))

    def qual(self, n):
        return self.rng.choice(self.quals, n).astype(np.uint8)

    def add(self, tid, pos, ops, seq, qual=None, flag=99, mapq=60, xc=0, ref=True, aim=None, rates=None):
        assert pos >= 0 and len(seq) == sum(l for l, op in ops if op in "MIS=X")
        tag = len(self.recs)
        self.recs.append(dict(tid=tid, pos=pos, flag=flag, mapq=mapq, ops=ops, lq=len(seq), seq=seq, qual=self.qual(len(seq)) if qual is None else qual,
                              mtid=tid, mpos=pos + 200, isize=300, xc=xc, tag=tag, ref=ref))
        if aim is not None:
            self.aims[tag] = (aim[0], aim[1], rates)   # bin key (tid, side, pos), cluster number, the runs it holds for (None: every rate above 0)
        return tag

    def aligned(self, n):
        """CIGAR of an aligned part of n bases: every third record with an insertion, so that records of one bin differ in their CIGAR text"""
        k = len(self.recs)
        if k % 3 == 1 and n >= 3:
            a = 1 + k % (n - 2)
            return [(a, "M"), (1, "I"), (n - a - 1, "M")]
        return [(n, "M")]

    def ev(self, tid, side, bp, left, right, ordered=True, **kw):
        """one-end clip with the breakpoint-relative sides `left` / `right` in the (tid, side, bp) bin.  The events of a '3' bin come in the
        order of their records' starts, end - reference length: `ordered` gives every record of the bin a deletion that puts its start behind
        the one before, whatever its left side's length (and makes every CIGAR of the bin another)"""
        seq = left[::-1] + right
        if side == "5":
            ops = [(len(left), "S")] + self.aligned(len(right))
            return self.add(tid, bp - 1, ops, seq, **kw)
        if ordered:
            k = self.placed[(tid, bp)] = self.placed.get((tid, bp), -1) + 1
            ref_len = 900 - k
            ops = [(1, "M"), (ref_len - len(left), "D")] + ([(len(left) - 1, "M")] if len(left) > 1 else []) + [(len(right), "S")]
            return self.add(tid, bp - ref_len, ops, seq, **kw)
        ops = self.aligned(len(left)) + [(len(right), "S")]
        return self.add(tid, bp - sum(l for l, op in ops if op == "M"), ops, seq, **kw)

    def finish(self, name, extra=0):
        for tid in (1, 2):   # the first record of another contig only flushes: a clipped read that would be a cluster of its own
            self.add(tid, 10, [(20, "S"), (30, "M")], self.seq(50))
        if extra:            # the length class: one more clipped read in the pass
            self.add(2, 50, [(extra // 3, "S"), (extra - extra // 3, "M")], self.seq(extra))
        order = sorted(range(len(self.recs)), key=lambda i: (self.recs[i]["tid"], self.recs[i]["pos"]))
        recs = [self.recs[i] for i in order]
        return dict(name=name, names=NAMES, lens=[CONTIG_LEN] * 3, recs=recs, batch=records_to_batch(recs), aims=self.aims, expect=self.expect, both=self.both)


# ---- a: threshold sweep ----
def mismatch_places(n, count, start):
    """`count` of the positions 0 .. n - 1: the breakpoint end, the far end, then 4k - 1 / 4k / 4k + 1 (a lane's four positions end and begin there)"""
    pri = [0, n - 1] + [x for k in range(1, n // 4 + 2) for x in (4 * k - 1, 4 * k, 4 * k + 1)] + list(range(n))
    seen, out = set(), []
    for x in pri[start % 3:] + pri[:start % 3]:
        if 0 <= x < n and x not in seen:
            seen.add(x); out.append(x)
    return out[:count]


def sweep_bins(B, rate, nmax, cap):
    for n in range(1, nmax + 1):
        need = minm(n, rate)
        for di, deciding in enumerate("LR"):
            for vi, verdict in enumerate(("join", "new")):
                m = need if verdict == "join" else need - 1
                if m < 0:
                    continue   # rate 0: every overlap passes
                side = "53"[(n + di + vi) & 1]
                tid = n % 3
                o = max(1, min(1 + n % 4, cap - n - 1))
                nlong = min(cap - o, n + (0 if n % 3 == 0 else 1 + 2 * (n % 4)))
                n1, n2 = (nlong, n) if n & 1 else (n, nlong)
                master, other = B.seq(nlong), B.seq(o)
                d2 = list(master[:n2])
                for x in mismatch_places(n, n - m, n + di):
                    d2[x] = mutate(d2[x])
                d1, d2 = master[:n1], "".join(d2)
                bp = B.bp(tid)
                key = (tid, side, bp)
                sides1, sides2 = ((d1, other), (d2, other)) if deciding == "L" else ((other, d1), (other, d2))
                B.ev(tid, side, bp, *sides1, aim=(key, 0), rates=(rate,))
                B.ev(tid, side, bp, *sides2, aim=(key, 0 if verdict == "join" else 1), rates=(rate,))
                B.expect.setdefault("sweep", []).append((n, deciding, verdict, key))


# ---- b / e: cluster counts ----
def cluster_bin(B, tid, side, K, lm, rm, growth=None):
    """a bin that ends with K clusters (at 0.9): K founders from unrelated masters, joiners aimed at the clusters where storage changes, all of
    them windows of the founder's masters (so they join at every rate above 0); sides of about lm / rm bases, lengths odd apart"""
    bp = B.bp(tid)
    key = (tid, side, bp)
    room_l, room_r = lm + 40, rm + 50
    ML = [B.seq(room_l) for _ in range(K)]
    MR = [B.seq(room_r) for _ in range(K)]
    early, late = (0, K - 1) if K >= 5 else (None, None)
    if early is not None:   # the late cluster's masters: the early one's, every 7th base another (they stay apart at 0.9)
        ML[late] = "".join(mutate(c) if i % 7 == 6 else c for i, c in enumerate(ML[early]))
        MR[late] = "".join(mutate(c) if i % 7 == 6 else c for i, c in enumerate(MR[early]))
    cur = []
    tags = []
    for k in range(K):
        a, b = (20, 30) if k == growth else (lm + k % 7, rm + (3 * k) % 5)
        if k in (early, late):
            a, b = lm + 2, rm + 2   # a multiple of 14 apart or not: the same overlap for both
        cur.append([a, b])
        tags.append(B.ev(tid, side, bp, ML[k][:a], MR[k][:b], aim=(key, k), rates=(0.9, 1.0) if k == late else None))
    if early is not None:   # between the two: every 14th base like the late one's - passes both at 0.9, the early cluster comes first
        a, b = cur[early]
        xl = "".join(mutate(c) if i % 14 == 13 else c for i, c in enumerate(ML[early][:a]))
        xr = "".join(mutate(c) if i % 14 == 13 else c for i, c in enumerate(MR[early][:b]))
        B.both.append((B.ev(tid, side, bp, xl, xr, qual=np.zeros(a + b, np.uint8), aim=(key, early), rates=(0.9,)), tags[late], key, early))   # (quality 0: it leaves the early cluster's bases alone)
    for t in sorted({0, B4_KLDS - 1, B4_KLDS, BIN_KLDS - 1, BIN_KLDS, CL_CACHE - 1, CL_CACHE, K - 1}):
        if not 0 <= t < K or t == growth:
            continue
        a, b = cur[t]
        for da, db in ((-3, -5), (4, 0), (0, 3), (-1, 2)):   # shorter on both sides, longer left, longer right, one of each
            B.ev(tid, side, bp, ML[t][:a + da], MR[t][:b + db], aim=(key, t), rates=(0.9, 1.0) if t == late else None)
        cur[t] = [a + 4, b + 3]
    if growth is not None:
        g = growth
        a, b = cur[g]
        B.ev(tid, side, bp, ML[g][:a + 20], MR[g][:b + 30], aim=(key, g))                 # lengthens both strings
        x = int(0.1 * a) + 1
        assert not rate_ok(a - x, a, 0.9) and rate_ok(a + 20 - x, a + 20, 0.9)
        left = "".join(mutate(c) if i < x else c for i, c in enumerate(ML[g][:a + 20]))
        B.ev(tid, side, bp, left, MR[g][:b], aim=(key, g), rates=(0.9,))                  # passes only against the longer left string
        R, i = b + 30, 5
        right = list(MR[g][:R]); right[i] = mutate(right[i])
        q = B.qual(a + 20 + R)
        q[a + 20 + i] = 93                                                                    # (the others of this bin stay below 93)
        B.ev(tid, side, bp, ML[g][:a + 20], "".join(right), qual=q, aim=(key, g), rates=(0.9,))   # its base replaces the cluster's
        for y in [y for y in mismatch_places(R, R, 1) if y != i][:R - minm(R, 0.9)]:
            right[y] = mutate(right[y])
        assert sum(1 for u in range(R) if right[u] == MR[g][u]) == minm(R, 0.9) - 1
        B.ev(tid, side, bp, ML[g][:a + 20], "".join(right), aim=(key, g), rates=(0.9,))     # passes only with the replaced base
    B.expect.setdefault("clusters", []).append((K, key))
    return key


def counts_sample(extra):
    B = Builder(11, quals=(0, 2, 9, 10, 40))
    for i, K in enumerate(COUNTS):
        for j, side in enumerate("53"):
            cluster_bin(B, (i + j) % 3, side, K, 31 + 2 * j, 40 + i % 3, growth={6: 1, 70: 67}.get(K))
    return B.finish(f"b-{extra}", extra)


# ---- c: bin depths ----
def deep_bin(B, tid, side, depth, bp=None, lm=45, rm=60):
    """`depth` events from one to three masters: windows of odd lengths, every third with two other bases (so that the better quality decides)"""
    bp = B.bp(tid) if bp is None else bp
    key = (tid, side, bp)
    nm = 1 + depth % 3
    ML, MR = [B.seq(lm + 30) for _ in range(nm)], [B.seq(rm + 30) for _ in range(nm)]
    for e in range(depth):
        k = int(B.rng.randint(nm))
        a, b = lm - 15 + int(B.rng.randint(0, 41)), rm - 15 + int(B.rng.randint(0, 41))
        left, right = list(ML[k][:a]), list(MR[k][:b])
        if e % 3 == 2:
            for s, n in ((left, a), (right, b)):
                x = int(B.rng.randint(n)); s[x] = mutate(s[x])
        B.ev(tid, side, bp, "".join(left), "".join(right), ordered=False)
    B.expect.setdefault("depths", []).append((depth, key))
    return key


def depths_sample(extra):
    B = Builder(12)
    B.expect["first"] = deep_bin(B, 0, "5", CL_CACHE + 1, bp=600)    # slot 0: the '5' bin at the smallest position of contig 0
    for i, d in enumerate(DEPTHS):
        for j, side in enumerate("35"):
            deep_bin(B, (i + j) % 3, side, d)
    # the filters: records at a bin of three that no run may count (and some that only -s / -q 0 let in)
    bp = B.bp(1)
    ml, mr = B.seq(40), B.seq(50)
    for _ in range(3):
        B.ev(1, "5", bp, ml, mr)
    B.ev(1, "5", bp, ml, mr, flag=99 | F_DUP)
    B.ev(1, "5", bp, ml, mr, mapq=0)
    B.ev(1, "5", bp, ml, mr, mapq=19)
    B.ev(1, "5", bp, ml, mr, xc=1)
    B.ev(1, "5", bp, ml, mr, flag=73)   # mate unmapped: the unmapped-pair side channel, not a clip event
    B.add(1, bp - 1, [(40, "S"), (45, "M"), (5, "H")], ml[::-1] + mr[:45])
    B.add(1, bp - 1, [(3, "H"), (40, "S"), (50, "M")], ml[::-1] + mr)
    B.add(1, bp - 1, [(90, "M")], B.seq(90))
    for flag in (99, 99 | F_REV):   # XC on a both-end clip: the strand says which end stays
        B.add(1, bp - 1, [(40, "S"), (50, "M"), (6, "S")], ml[::-1] + mr + B.seq(6), flag=flag, xc=1)
    B.expect["last"] = deep_bin(B, 2, "3", B4_DEEP, bp=20000)       # the last 16 slots: the '3' bin at the largest end of the last contig
    return B.finish(f"c-{extra}", extra)


# ---- d: merge rules ----
def merge_bins(B, lengths, cap):
    for side in "53":
        for deciding in "LR":
            for s in lengths:
                for la, lb in ((s, s), (s, s + 1), (s + 1, s)):
                    o = min(7 + 2 * (la % 3), cap - max(la, lb))
                    if o < 1:
                        continue
                    tid = s % 3
                    bp = B.bp(tid)
                    key = (tid, side, bp)
                    m, other = B.seq(max(la, lb)), B.seq(o + 1)
                    for n, oo in ((la, o), (lb, o)):
                        B.ev(tid, side, bp, *((m[:n], other[:oo]) if deciding == "L" else (other[:oo], m[:n])), aim=(key, 0))
                    if max(la, lb) + o + 1 <= cap:   # a third with the other side one longer
                        B.ev(tid, side, bp, *((m[:la], other) if deciding == "L" else (other, m[:la])), aim=(key, 0))


def merge_sample(extra):
    B = Builder(13)
    # 256 stays out here: in a pass of reads up to B4_CAP bases a side of 256 bases leaves the other side empty, and an empty side (n == 0)
    # never passes, so such an event can only found a cluster - the lone 256S below.  Sides of 256 bases that merge need longer reads:
    # class_sample builds them, equal and one longer, from 259 bases on (k_cluster_bins).
    assert max(SIDE_LENGTHS) + 1 <= B4_CAP
    merge_bins(B, list(SIDE_LENGTHS), B4_CAP)
    for side in "53":
        # chains: six events of one master, one to three other bases each, the better quality takes the base
        for c in range(16):
            tid, bp = c % 3, B.bp(c % 3)
            ml, mr = B.seq(70), B.seq(80)
            for e in range(6):
                a, b = 41 + int(B.rng.randint(0, 25)), 50 + int(B.rng.randint(0, 25))
                left, right = list(ml[:a]), list(mr[:b])
                for _ in range(1 + e % 3):
                    s = (left, right)[int(B.rng.randint(2))]
                    x = int(B.rng.randint(len(s))); s[x] = mutate(s[x])
                B.ev(tid, side, bp, "".join(left), "".join(right))
    # both-end clips: records of one start and one aligned length share a '5' and a '3' bin; the '3' event's sides begin inside the read
    for a0, c0 in ((1, 1), (2, 4), (3, 9), (7, 2), (30, 33)):
        tid, pos = a0 % 3, B.bp(a0 % 3) + 3000
        mid_len = 21 + 2 * a0
        ml, mid, mr = B.seq(a0 + 4), B.seq(mid_len), B.seq(c0 + 4)
        for a, c in ((a0, c0), (a0 + 1, c0), (a0, c0 + 2), (a0 + 3, c0 + 3), (a0, c0)):
            B.add(tid, pos, [(a, "S"), (mid_len, "M"), (c, "S")], ml[:a][::-1] + mid + mr[:c])
    # a lone soft clip: two rows with an empty part; alone in its bins the reference defines it
    for lq in (1, 2, 37, B4_CAP):
        B.add(lq % 3, B.bp(lq % 3) + 6000, [(lq, "S")], B.seq(lq))
    # ---- not sent to the reference (it reads outside its strings there) ----
    for side in "53":
        tid, bp = 1, B.bp(1)
        ml, mr = B.seq(40), B.seq(50)
        B.ev(tid, side, bp, ml[:30], mr[:35], ref=False)
        B.add(tid, bp - 1 if side == "5" else bp, [(44, "S")], B.seq(44), ref=False)       # a lone S inside a bin of several reads
        B.ev(tid, side, bp, ml, mr, ref=False)
        B.add(tid, bp - 1 if side == "5" else bp, [(44, "S")], B.seq(44), ref=False)
        for first_missing in (True, False):   # no qualities: the founder, or one that joins a cluster of reads with qualities
            bp = B.bp(tid)
            for e in range(4):
                a, b = 30 + 3 * e, 41 - 2 * e
                missing = (e == 0) == first_missing if e < 2 else e == 3 and not first_missing
                B.ev(tid, side, bp, ml[:a], mr[:b], qual=np.full(a + b, 255, np.uint8) if missing else None, ref=False)
    return B.finish(f"d-{extra}", extra)


# ---- e: reads of the class's own length ----
def class_sample(cls):
    B = Builder(14, quals=(0, 2, 9, 10, 40))
    lm = cls // 2 - 30
    for j, side in enumerate("53"):
        for K in (5, 66):
            # founders of l_qseq == cls among them: sides lm + k % 7 and cls - that
            bp = B.bp(j)
            key = (j, side, bp)
            ML, MR = [B.seq(lm + 10) for _ in range(K)], [B.seq(cls - lm + 4) for _ in range(K)]
            for k in range(K):
                a = lm + k % 7
                b = cls - a - (k % 4 if k else 0)   # (the first: the class's length itself)
                B.ev(j, side, bp, ML[k][:a], MR[k][:b], aim=(key, k))
            for t in sorted({0, B4_KLDS - 1, B4_KLDS, BIN_KLDS - 1, BIN_KLDS, CL_CACHE - 1, CL_CACHE, K - 1}):
                if t < K:
                    a = lm + t % 7
                    b = cls - a - (t % 4 if t else 0)
                    for da, db in ((-3, -5), (2, -3), (-4, 1)):
                        B.ev(j, side, bp, ML[t][:a + da], MR[t][:b + db], aim=(key, t))
            B.expect.setdefault("clusters", []).append((K, key))
    if cls >= B4_CAP + 1:
        merge_bins(B, [255, 256], cls)
    return B.finish(f"e-{cls}", 0)


def sweep_sample(tag, cls):
    rate = RUN_KW[tag].get("match_rate", 0.9)
    nmax, cap = SWEEP_OWN.get(cls, SWEEP_OWN[0])
    B = Builder(15)
    sweep_bins(B, rate, nmax, cap)
    return B.finish(f"a{tag[1:]}-{cls}", 0 if cls in SWEEP_OWN else cls)


FAMILIES = tuple("a" + tag[1:] for tag, _, _ in RUNS) + ("b", "c", "d", "e")
SAMPLE_IDS = [(f, c) for f in FAMILIES for c in CLASSES if not (f == "e" and c == 0)]


def runs_of(family):
    """the runs a family's samples go through: a sweep is built for one rate"""
    return [r for r in RUNS if r[0][1:] == family[1:]] if family[0] == "a" else list(RUNS)


@functools.lru_cache(maxsize=None)
def sample(family, cls):
    if family[0] == "a":
        s = sweep_sample("t" + family[1:], cls)
    elif family == "e":
        s = class_sample(cls)
    else:
        s = {"b": counts_sample, "c": depths_sample, "d": merge_sample}[family](cls)
    s["family"], s["cls"] = family, cls
    return s


@functools.lru_cache(maxsize=None)
def modelled(family, cls, tag, ref_only=False):
    """(table, bins, records) of the model for one run; ref_only: the part of the sample that the reference defines"""
    s = sample(family, cls)
    recs = [r for r in s["recs"] if r["ref"]] if ref_only else s["recs"]
    t, bins = getclip_model(recs, **RUN_KW[tag])
    return t, bins, recs


def cuts_of(family, cls):
    """batch cuts inside the deepest bin and inside the bin with the most clusters (at 0.9): record indices"""
    s = sample(family, cls)
    t, bins, recs = modelled(family, cls, "t090")
    deep = max(bins, key=lambda b: b["n_events"])
    many = max(bins, key=lambda b: b["n_clusters"])
    n = len(recs)
    return sorted({0, n, deep["recs"][len(deep["recs"]) // 2], many["recs"][(2 * len(many["recs"])) // 3]})


def events_of(r):
    return _events_of(r, 0, True)
