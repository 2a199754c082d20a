"""Hand-made samples for the somatic look-ups (kernel k_somatic_probe, model tests/somatic_probe_model.py).  Every wanted cluster is ONE
soft-clipped read - `kS nM` (side '5') or `nM kS` (side '3') at a chosen position -, given `support` times; two clusters on one key are reads of unrelated
random bases (a quarter of their bases agree: far below the 0.9 at which getclip merges), so a pass's cluster table is exactly the listed clusters in the
listed order (tests/test_somatic_probe_inputs.py asserts that through the oracle).  A sample lists its passes, and its probes each with the answer written
here by hand: the NAME of the cluster it must find, or None.

Sample: name, rate (somatic's -t), min_len (somatic's -m), passes = [[Cluster, ...], ...], cases = [(label, probe dict, expected cluster name or None)]."""
import collections
import zlib

import numpy as np

from cluster_bins_inputs import records_to_batch

NAMES = ["c0", "c1", "c2"]
CONTIG_LEN = 60000
Cluster = collections.namedtuple("Cluster", "name tid pos side left right support")
Sample = collections.namedtuple("Sample", "name rate min_len passes cases")


def R(tag, n):
    """n random bases that depend on `tag` alone"""
    return "".join("ACGT"[x] for x in np.random.RandomState(zlib.crc32(tag.encode())).randint(0, 4, n))


def mut(s, idx):
    """s with the bases at idx substituted (A>C>G>T>A; N>A)"""
    t = list(s)
    for i in idx:
        t[i] = "CGTA"["ACGT".index(t[i])] if t[i] in "ACGT" else "A"
    return "".join(t)


def P(tid, side, lo, hi, mode, a, b):
    return dict(tid=tid, side=side, lo=lo, hi=hi, mode=mode, a=a, b=b)


def X(tid, side, pos, a, b):
    return P(tid, side, pos, pos, 0, a, b)


def cluster_records(c):
    """the reads of one listed cluster: 0-based start, CIGAR, bases; quality 40 throughout, a proper pair of mapping quality 60"""
    seq = c.left + c.right
    if c.side == "5":
        pos0, ops = c.pos - 1, [(len(c.left), "S"), (len(c.right), "M")]
    else:
        pos0, ops = c.pos - len(c.left), [(len(c.left), "M"), (len(c.right), "S")]
    assert pos0 >= 0
    return [dict(tid=c.tid, pos=pos0, flag=99, mapq=60, ops=ops, lq=len(seq), seq=seq, qual=np.full(len(seq), 40, np.uint8), mtid=c.tid, mpos=pos0 + 200, isize=300, xc=0)
            for _ in range(c.support)]


def pass_records(clusters):
    """a pass's reads in coordinate order (equal starts in the listed order).  Every contig's visit begins with an unclipped read at its start: the first
    mapped-pair record behind a change of contig only triggers the flush and is itself not looked at (clip_reads.h:423-438)"""
    recs = [r for c in clusters for r in cluster_records(c)]
    for tid in sorted({c.tid for c in clusters}):
        seq = R(f"first.{tid}", 30)
        recs.append(dict(tid=tid, pos=0, flag=99, mapq=60, ops=[(30, "M")], lq=30, seq=seq, qual=np.full(30, 40, np.uint8), mtid=tid, mpos=200, isize=300, xc=0))
    recs.sort(key=lambda r: (r["tid"], r["pos"], len(r["ops"])))  # (the unclipped read first)
    return recs


def pass_batch(clusters):
    return records_to_batch(pass_records(clusters))


def table_order(clusters):
    """the listed clusters in the order the table must have: by contig, '5' before '3', by position, equal keys in the order of their reads in the file"""
    first = {}
    recs = sorted(((c.tid, (c.pos - 1) if c.side == "5" else c.pos - len(c.left), k) for k, c in enumerate(clusters)), key=lambda t: t[:2])  # (as pass_records sorts)
    for n, (_, _, k) in enumerate(recs):
        first[k] = n
    return sorted(clusters, key=lambda c: (c.tid, c.side != "5", c.pos, first[clusters.index(c)]))


def expected_hit(sample, name):
    """the hand-written answer as (support, pos, pass, cluster index in that pass's table)"""
    if name is None:
        return (0, 0, 0, 0)
    for n, clusters in enumerate(sample.passes):
        for k, c in enumerate(table_order(clusters)):
            if c.name == name:
                return (c.support, c.pos, n, k)
    raise KeyError(name)


# ---- rates and thresholds ----

def rates_sample():
    L, Rt = R("rates.L", 20), R("rates.R", 20)
    A = Cluster("A", 0, 1000, "5", L, Rt, 1)
    t = lambda a, b: X(0, "5", 1000, a, b)
    cases = [("equal strings", t(L, Rt), "A"),
             ("right 9 of 10", t(L, mut(Rt[:10], [3])), "A"), ("right 8 of 10", t(L, mut(Rt[:10], [3, 9])), None),
             ("left 9 of 10", t(mut(L[-10:], [0]), Rt), "A"), ("left 8 of 10", t(mut(L[-10:], [0, 9]), Rt), None),
             ("right 18 of 20", t(L, mut(Rt, [0, 19])), "A"), ("right 17 of 20", t(L, mut(Rt, [0, 10, 19])), None),
             ("empty left", t("", Rt), None), ("empty right", t(L, ""), None), ("both empty", t("", ""), None),
             ("wrong position", X(0, "5", 1001, L, Rt), None), ("wrong side", X(0, "3", 1000, L, Rt), None), ("wrong contig", X(1, "5", 1000, L, Rt), None)]
    return Sample("rates", 0.9, 10, [[A]], cases)


def half_sample():
    L, Rt = R("half.L", 12), R("half.R", 12)
    A = Cluster("A", 0, 1000, "5", L, Rt, 2)
    t = lambda a, b: X(0, "5", 1000, a, b)
    cases = [("right 1 of 2", t(L, mut(Rt[:2], [1])), "A"), ("right 0 of 2", t(L, mut(Rt[:2], [0, 1])), None),
             ("left 1 of 2", t(mut(L[-2:], [0]), Rt), "A"), ("left 0 of 2", t(mut(L[-2:], [0, 1]), Rt), None),
             ("right 6 of 12", t(L, mut(Rt, range(0, 12, 2))), "A"), ("right 5 of 12", t(L, mut(Rt, [0, 2, 4, 6, 8, 10, 11])), None),
             ("right 1 of 3", t(L, mut(Rt[:3], [0, 2])), None), ("empty right", t(L, ""), None)]
    return Sample("half", 0.5, 10, [[A]], cases)


# ---- lengths: 1, 63, 64, 65, 129 on either string; the lanes take characters 64 at a time ----

LENGTHS = (1, 63, 64, 65, 129)
MAX_MISMATCHES = {1: 0, 63: 6, 64: 6, 65: 6, 129: 12}  # the most substitutions in n characters that still reach 0.9: 57/63, 58/64, 59/65, 117/129 (56/63, 57/64, 58/65, 116/129 do not)


def spread(n, k):
    """k distinct indices of a string of n characters: its ends first, then the places around a wavefront's 64th character"""
    order = [0, n - 1, 63, 64, 62, 65, 1, n - 2, 31, 32, 100, 127, 128, 2, 3, 4]
    out = []
    for i in order:
        if 0 <= i < n and i not in out:
            out.append(i)
    return out[:k]


def lengths_sample():
    clusters, cases = [], []
    for i, n in enumerate(LENGTHS):
        k = MAX_MISMATCHES[n]
        # the clipped left side of a '5' cluster is n long
        c = Cluster(f"five.left{n}", 0, 2000 + 20 * i, "5", R(f"len.a{n}", n), R(f"len.b{n}", 30), 1)
        clusters.append(c)
        cases += [(f"{c.name} equal", X(0, "5", c.pos, c.left, c.right), c.name),
                  (f"{c.name} probe longer", X(0, "5", c.pos, R("pre", 40) + c.left, c.right + R("post", 40)), c.name),
                  (f"{c.name} {k} substitutions", X(0, "5", c.pos, mut(c.left, spread(n, k)), c.right), c.name),
                  (f"{c.name} {k + 1} substitutions", X(0, "5", c.pos, mut(c.left, spread(n, k + 1)), c.right), None)]
        if n > 1:
            cases += [(f"{c.name} probe shorter", X(0, "5", c.pos, c.left[-(n // 2):], c.right[:15]), c.name),
                      (f"{c.name} probe shorter, its far end wrong", X(0, "5", c.pos, mut(c.left[-10:], [0, 1]), c.right[:15]), None)]
        # the clipped right side of a '3' cluster is n long
        d = Cluster(f"three.right{n}", 0, 4000 + 20 * i, "3", R(f"len.c{n}", 30), R(f"len.d{n}", n), 1)
        clusters.append(d)
        cases += [(f"{d.name} equal", X(0, "3", d.pos, d.left, d.right), d.name),
                  (f"{d.name} probe longer", X(0, "3", d.pos, R("pre", 70) + d.left, d.right + R("post", 70)), d.name),
                  (f"{d.name} {k} substitutions", X(0, "3", d.pos, d.left, mut(d.right, spread(n, k))), d.name),
                  (f"{d.name} {k + 1} substitutions", X(0, "3", d.pos, d.left, mut(d.right, spread(n, k + 1))), None)]
        # the aligned right side of a '5' cluster is n long
        e = Cluster(f"five.right{n}", 1, 2000 + 20 * i, "5", R(f"len.e{n}", 30), R(f"len.f{n}", n), 1)
        clusters.append(e)
        cases += [(f"{e.name} equal", X(1, "5", e.pos, e.left, e.right), e.name),
                  (f"{e.name} {k} substitutions", X(1, "5", e.pos, e.left, mut(e.right, spread(n, k))), e.name),
                  (f"{e.name} {k + 1} substitutions", X(1, "5", e.pos, e.left, mut(e.right, spread(n, k + 1))), None)]
    return Sample("lengths", 0.9, 1, [clusters], cases)


# ---- the 10-base anchor ----

def anchor_sample():
    clusters, cases = [], []
    # probe first (mode 2): s2 = the probe's b, searched in the cluster's right side
    L, Rt = R("anc.L", 40), R("anc.R", 80)
    C = Cluster("C", 1, 3000, "3", L, Rt, 1)
    clusters.append(C)
    w = lambda mode, a, b: P(1, "3", 2990, 3010, mode, a, b)
    cases += [("probe first, |s2| 9", w(2, L, Rt[:9]), None), ("probe first, |s2| 10", w(2, L, Rt[:10]), "C"), ("probe first, |s2| 11", w(2, L, Rt[:11]), "C"),
              ("probe first, anchor at 0", w(2, L[-25:], Rt[:30]), "C")]
    for h in (54, 55, 70):  # 54 / 55: the ten bases straddle the wavefront's lane 63 / 64; 70: the last offset at which ten bases fit
        head = L + Rt[:h]
        cases += [(f"probe first, anchor at {h}", w(2, head[-30:], Rt[h:h + 20]), "C"),
                  (f"probe first, anchor at {h}, the head wrong", w(2, mut(head[-30:], [0, 9, 19, 29]), Rt[h:h + 20]), None)]
    cases += [("probe first, anchor absent", w(2, L, R("anc.other", 30)), None),
              ("probe first, anchor found, the tail wrong", w(2, L, Rt[:10] + R("anc.junk", 20)), None)]
    # cluster first (mode 1): s2 = the cluster's right side, searched in the probe's b; |s2| = 9 / 10 / 11 are clusters of their own
    for n in (9, 10, 11):
        c = Cluster(f"right{n}", 1, 3200 + 20 * n, "3", R(f"anc.l{n}", 30), R(f"anc.r{n}", n), 1)
        clusters.append(c)
        cases.append((f"cluster first, |s2| {n}", P(1, "3", c.pos - 5, c.pos + 5, 1, c.left, c.right + R("anc.more", 12)), None if n < 10 else c.name))
    L2, R2 = R("anc.L2", 40), R("anc.R2", 30)
    D = Cluster("D", 1, 3600, "3", L2, R2, 3)
    clusters.append(D)
    v = lambda a, b: P(1, "3", 3590, 3610, 1, a, b)
    cases += [("cluster first, anchor at 0", v(L2, R2), "D")]
    for h in (54, 55):
        cases += [(f"cluster first, anchor at {h}", v(R("anc.any", 7), R("anc.y", h - 40) + L2 + R2[:20]), "D"),
                  (f"cluster first, anchor at {h}, the head wrong", v(R("anc.any", 7), R("anc.y", h - 40) + mut(L2, [0, 10, 20, 30, 39]) + R2[:20]), None)]
    cases += [("cluster first, anchor at the last offset", v(L2[:20], L2[20:] + R2[:10]), "D"),
              ("cluster first, anchor absent", v(L2, R2[1:]), None)]
    # the anchor twice in s4: only the second occurrence would satisfy the rates, and it is never tried
    anchor, junk, tail, L3 = R("anc.a", 10), R("anc.j", 20), R("anc.t", 30), R("anc.L3", 30)
    E = Cluster("E", 1, 4000, "3", L3, anchor + junk + anchor + tail, 1)
    clusters.append(E)
    cases += [("anchor twice, the second would match", P(1, "3", 3990, 4010, 2, (L3 + anchor + junk)[-20:], anchor + tail[:20]), None),
              ("anchor twice, the first matches", P(1, "3", 3990, 4010, 2, L3[-20:], anchor + junk), "E")]
    # the same strings in modes 1 and 2: the probe's junction lies five bases before the cluster's
    L4, R4 = R("anc.L4", 30), R("anc.R4", 30)
    F = Cluster("F", 1, 4400, "3", L4, R4, 2)
    clusters.append(F)
    cases += [("junction five bases earlier, cluster first", P(1, "3", 4390, 4410, 1, L4[:25], L4[25:] + R4), "F"),
              ("junction five bases earlier, probe first", P(1, "3", 4390, 4410, 2, L4[:25], L4[25:] + R4), None)]
    return Sample("anchor", 0.9, 1, [clusters], cases)


# ---- walking the candidates ----

def walk_sample():
    clusters, cases = [], []
    # three clusters at one position: the 1st and the 3rd share the ten bases on either side of the breakpoint
    sl, sr = R("walk.sl", 10), R("walk.sr", 10)
    W1 = Cluster("W1", 0, 5000, "5", R("walk.1l", 30) + sl, sr + R("walk.1r", 30), 1)
    W2 = Cluster("W2", 0, 5000, "5", R("walk.2l", 40), R("walk.2r", 40), 2)
    W3 = Cluster("W3", 0, 5000, "5", R("walk.3l", 30) + sl, sr + R("walk.3r", 30), 3)
    clusters += [W1, W2, W3]
    cases += [("only the third matches", X(0, "5", 5000, W3.left, W3.right), "W3"), ("only the second matches", X(0, "5", 5000, W2.left, W2.right), "W2"),
              ("the first and the third match", X(0, "5", 5000, sl, sr), "W1"), ("none of three matches", X(0, "5", 5000, R("walk.x", 20), R("walk.y", 20)), None),
              ("the first and the third match, anchored", P(0, "5", 4990, 5000, 2, sl, sr), "W1")]
    # a window over several positions: the same strings at 7000 and 7031, other clusters between
    gl, gr = R("walk.gl", 30), R("walk.gr", 30)
    G1, G2 = Cluster("G1", 0, 7000, "5", gl, gr, 4), Cluster("G2", 0, 7031, "5", gl, gr, 5)
    mids = [Cluster(f"mid{p}", 0, p, "5", R(f"walk.ml{p}", 30), R(f"walk.mr{p}", 30), 1) for p in (7005, 7015, 7030)]
    clusters += [G1] + mids + [G2]
    g = lambda lo, hi: P(0, "5", lo, hi, 2, gl, gr)
    cases += [("a match just outside each end", g(7001, 7030), None), ("the first match at lo", g(7000, 7030), "G1"), ("the first match at hi", g(7001, 7031), "G2"),
              ("both ends inside: the smaller position", g(6990, 7040), "G1"), ("an exact probe inside the window's positions", X(0, "5", 7015, mids[1].left, mids[1].right), "mid7015"),
              ("an empty window", g(7016, 7029), None), ("lo above hi", g(7031, 7000), None)]
    # lo <= 0, and windows that reach over a run's ends: contig 2 has '5' clusters only, contig 1 '3' clusters only
    H = Cluster("H", 2, 5, "5", R("walk.hl", 20), R("walk.hr", 30), 2)
    H2 = Cluster("H2", 2, 900, "5", R("walk.h2l", 20), R("walk.h2r", 30), 1)
    T1 = Cluster("T1", 1, 800, "3", R("walk.t1l", 30), R("walk.t1r", 20), 1)
    T2 = Cluster("T2", 1, 59000, "3", R("walk.t2l", 30), R("walk.t2r", 20), 6)
    clusters += [H, H2, T1, T2]
    cases += [("lo negative", P(2, "5", -25, 5, 2, H.left, H.right), "H"), ("lo zero", P(2, "5", 0, 4, 2, H.left, H.right), None),
              ("an exact probe at zero", X(2, "5", 0, H.left, H.right), None), ("an exact probe below zero", X(2, "5", -3, H.left, H.right), None),
              ("a window from before the run's first cluster", P(2, "5", -1000, 899, 2, H.left, H.right), "H"),
              ("a window to behind the run's last cluster", P(1, "3", 801, 2000000000, 1, T2.left, T2.right), "T2"),
              ("a window over a whole run", P(2, "5", -2000000000, 2000000000, 2, H2.left, H2.right), "H2"),
              ("the last run's last cluster", P(2, "5", 900, 900, 2, H2.left, H2.right), "H2"),
              ("a contig with clusters of the other side only, '3'", X(2, "3", 5, H.left, H.right), None),
              ("a contig with clusters of the other side only, '5'", P(1, "5", 0, 60000, 2, T1.left, T1.right), None),
              ("a contig the header does not have", P(-1, "5", -25, 5, 2, H.left, H.right), None),
              ("a contig without clusters", X(3, "5", 5, H.left, H.right), None)]
    return Sample("walk", 0.9, 10, [clusters], cases)


# ---- the length filter and N ----

def filter_sample():
    clusters, cases = [], []
    shapes = (("five.clip9", "5", 9, 30, None), ("five.clip10", "5", 10, 30, True), ("five.aligned9", "5", 10, 9, True),
              ("three.clip9", "3", 30, 9, None), ("three.clip10", "3", 30, 10, True), ("three.aligned9", "3", 9, 10, True))
    for i, (name, side, ll, lr, seen) in enumerate(shapes):
        c = Cluster(name, 0, 9000 + 50 * i, side, R(name + ".l", ll), R(name + ".r", lr), 1)
        clusters.append(c)
        cases.append((name, X(0, side, c.pos, c.left, c.right), name if seen else None))
    # an N on both sides counts as a match: with it 9 of 10, without it 8 of 10
    ln = R("n.l", 20)
    ln = ln[:15] + "N" + ln[16:]
    Nc = Cluster("withN", 0, 9500, "5", ln, R("n.r", 30), 1)
    clusters.append(Nc)
    cases += [("N equals N", X(0, "5", 9500, mut(ln[-10:], [0]), Nc.right), "withN"), ("N against a base", X(0, "5", 9500, mut(ln[-10:], [0, 5]), Nc.right), None)]
    return Sample("filter", 0.9, 10, [clusters], cases)


# ---- passes: contig 0 comes back behind contig 1 ----

def passes_sample():
    xl, xr, yl, yr = R("pass.xl", 30), R("pass.xr", 30), R("pass.yl", 30), R("pass.yr", 30)
    p0 = [Cluster("X0", 0, 8000, "5", xl, xr, 1), Cluster("Y0", 0, 8120, "5", yl, yr, 2), Cluster("Z0", 1, 100, "5", R("pass.zl", 20), R("pass.zr", 20), 1)]
    p1 = [Cluster("X1", 0, 8000, "5", xl, xr, 3), Cluster("Y1", 0, 8110, "5", yl, yr, 4), Cluster("V1", 0, 8300, "5", R("pass.vl", 20), R("pass.vr", 20), 5)]
    cases = [("the same position in two passes: the earlier pass", P(0, "5", 7990, 8010, 2, xl, xr), "X0"),
             ("a smaller position in the later pass", P(0, "5", 8100, 8130, 2, yl, yr), "Y1"),
             ("the later pass's position outside the window", P(0, "5", 8115, 8130, 2, yl, yr), "Y0"),
             ("an exact probe that matches in both passes", X(0, "5", 8000, xl, xr), "X0"),
             ("a cluster of the later pass only", X(0, "5", 8300, p1[2].left, p1[2].right), "V1"),
             ("a cluster of the earlier pass only", X(1, "5", 100, p0[2].left, p0[2].right), "Z0"),
             ("other strings at a position of the later pass", X(0, "5", 8110, xl, xr), None),
             ("a window between the clusters of both passes", P(0, "5", 8001, 8109, 2, xl, xr), None)]
    return Sample("passes", 0.9, 10, [p0, p1], cases)


def samples():
    return [rates_sample(), half_sample(), lengths_sample(), anchor_sample(), walk_sample(), filter_sample(), passes_sample()]
