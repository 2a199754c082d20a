"""Designed getclip inputs for the event stage (ssv_clip_scan_range through cluster_sort: the CIGAR-end scan, the per-candidate filter, the
placing of the events, the copy of their bytes, the order of the two side lists): every size comes from the constants the kernels work in, so
that a candidate, an event or a key sits on purpose where a tile, a load, a wavefront or a sort window ends.

An input is a dict: name, family, names / lens (the contigs), recs (record dicts with the fields of
test_random_differential_gpu.random_sample(..., want_records=True), plus `ref`: the reference defines what the record gives), runs (tags of
RUNS), and what to do with it:
  kind "getclip"  the records as one batch and cut at every list of `cutsets`, through Context.getclip with `own` / `initial_last_tid`
  kind "passes"   `passes`: a list of passes, each dict(initial_last_tid, scans [(lo, hi, r0, r1)]): the batch recs[lo:hi] scanned with
                  ssv_clip_scan_range(r0, r1); their tables follow each other
Families: ends, tile_edges, candidate_counts, contig_switch, ranges_and_ownership, side_order, gather (see the functions).  In every family each
event is a cluster of its own: events that share a bin come from homopolymer reads of different bases and carry different CIGARs, so the table
shows the event list itself and the order inside a bin.  Reads are 30 bases long where length does not matter.
"""
import functools

import numpy as np

import clip_events_model as M
from cluster_bins_model import F_DUP, F_MUNMAP, F_REV, F_UNMAP, OPS

# what the inputs rest on (seeksv_amd/csrc: clip_kernels.h, tile_sort.h, common.h; tests/test_clip_events_inputs.py reads them out of the headers)
CONSTANTS = dict(CC_TILE=8192, CE_ITEMS=16, CE_SUB=2, BLOCK=256, WAVE=64, FILTER_WAVE=16, WS_W=32, WS_TILE=1024, LINE_OPS=5, GROUP=16, GATHER_BATCH=8)
CC_TILE, CE_ITEMS, CE_SUB, BLOCK, WAVE, FILTER_WAVE, WS_W, WS_TILE, LINE_OPS, GROUP, GATHER_BATCH = (CONSTANTS[k] for k in (
    "CC_TILE", "CE_ITEMS", "CE_SUB", "BLOCK", "WAVE", "FILTER_WAVE", "WS_W", "WS_TILE", "LINE_OPS", "GROUP", "GATHER_BATCH"))
SUB_TILE = BLOCK * CE_ITEMS              # 4,096 records: what the 256 lanes load at once
FILTER_BLOCK = BLOCK // 4                # 64 candidates a workgroup of k_clip_filter (four lanes each)
GATHER_DWORDS = GROUP * GATHER_BATCH     # 128 dwords: what k_clip_gather's unrolled batch covers
MAX_RECORDS = 5 * CC_TILE + 17

# (tag, the reference's flags, our parameters)
RUNS = (("d", [], {}), ("q0", ["-q", "0"], dict(min_mapq=0)), ("s", ["-s"], dict(save_low_quality=True)))
RUN_KW = {tag: kw for tag, _, kw in RUNS}
RUN_FLAGS = {tag: flags for tag, flags, _ in RUNS}
NO_SEQ = 0xFFFFFFFFFFFFFFFF
LQ = 30
FILL_SEQ = ("ACGTTGCAAC" * 3)[:LQ]
FILL_QUAL = np.full(LQ, 30, np.uint8)
TILE_DELTAS = (-17, -16, -15, -1, 0, 1, 15, 16, 17)
TILE_PLACES = (0, CE_ITEMS - 1, CE_ITEMS, WS_TILE - 1, WS_TILE, SUB_TILE - 1, SUB_TILE, CC_TILE - 1)   # inside every tile
CAND_COUNTS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025)
LONE_PLACES = (0, 15, 16, 63)
GAPS = (0, 1, 15, 16, 300)
CONTIG_IDS = (1, 2, 255, 256, 257, 4096, 70000)
GATHER_LQ = (1, 2, 3, 5, 340, 341, 342, 343, 600)
GATHER_NCIG = (5, 6, 7, 21, 300)
RADIX_BITS = 8                           # radix_sort.h: the sort takes the keys' bits a digit of 8 at a time, so their count matters per 8
KEY_BITS_CONTIG = 1 << (5 * RADIX_BITS - 33)   # 128: the first contig whose keys (tid << 33 | side << 32 | pos) have more than 40 bits


# ---------------------------------------------------------------------------------------------------------------------
# records and batches
# ---------------------------------------------------------------------------------------------------------------------
def rec(tid, pos, ops, seq=None, qual=None, flag=99, mapq=60, xc=0, ref=True):
    lq = sum(l for l, op in ops if op in "MIS=X") if ops else LQ
    if seq is None:
        seq, qual = (FILL_SEQ, FILL_QUAL) if lq == LQ else ((FILL_SEQ * (lq // LQ + 1))[:lq], None)
    if qual is None:
        qual = np.full(lq, 30, np.uint8)
    assert len(seq) == lq == len(qual) and pos >= 0
    return dict(tid=tid, pos=pos, flag=flag, mapq=mapq, ops=ops, lq=lq, seq=seq, qual=qual, mtid=tid, mpos=pos + 200, isize=300, xc=xc, ref=ref,
                span=sum(l for l, op in ops if op in "MDN=X"))


FILL_OPS = [(LQ, "M")]


def filler(tid, pos, **kw):
    return rec(tid, pos, FILL_OPS, **kw)


class Seqs:
    """random bases and qualities for the clipped reads (two of them never pass a match rate of 0.9 by chance: table() checks)"""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def seq(self, n=LQ):
        return "".join("ACGT"[x] for x in self.rng.randint(0, 4, n))

    def qual(self, n=LQ):
        return self.rng.choice([2, 11, 25, 37, 40], n).astype(np.uint8)


def clipped(S, tid, pos, kind, v=0, **kw):
    """a 30-base candidate: '5' / '3' / 'both' emit; 'dup', 'lowq', 'hard', 'xc' give no event in the default run ('lowq' does with -q 0, 'xc'
    with -s); 'xcboth' gives one of its two events (the strand's) without -s.  v in 0 .. 2: another CIGAR for the same key.
    Keys: '5' at pos + 1, '3' at pos + 20, of 'both' at pos + 14"""
    v %= 3
    left = [(10 + v, "S"), (20 - v, "M")]
    right = [(20, "M"), (10, "S")] if v == 0 else [(10, "M"), (v, "I"), (10, "M"), (10 - v, "S")]
    both = [(8 - v, "S"), (14, "M"), (8 + v, "S")]
    ops, extra = {"5": (left, {}), "3": (right, {}), "both": (both, {}), "dup": (left, dict(flag=99 | F_DUP)), "lowq": (right, dict(mapq=0)),
                  "hard": ([(10, "S"), (20, "M"), (3, "H")], {}), "xc": (left, dict(xc=1)), "xcboth": (both, dict(xc=1, flag=99 if v else 99 | F_REV))}[kind]
    extra.update(kw)
    return rec(tid, pos, ops, S.seq(), S.qual(), **extra)


NONE_KINDS = ("dup", "lowq", "hard", "xc")


def batch_of(recs, ends=True, ship_all=False, pad=True):
    """record dicts -> a host batch; bases and qualities only of the records with an S at either end (or of all), `ends`: with the cigar_ends column"""
    n = len(recs)
    b = dict(tid=np.array([r["tid"] for r in recs], np.int32), pos=np.array([r["pos"] for r in recs], np.int32),
             flag=np.array([r["flag"] for r in recs], np.uint16), mapq=np.array([r["mapq"] for r in recs], np.uint8),
             n_cigar=np.array([len(r["ops"]) for r in recs], np.uint16), l_qseq=np.array([r["lq"] for r in recs], np.int32),
             mtid=np.array([r["mtid"] for r in recs], np.int32), mpos=np.array([r["mpos"] for r in recs], np.int32),
             isize=np.array([r["isize"] for r in recs], np.int32), xc=np.array([r["xc"] for r in recs], np.uint8))
    code = np.zeros(256, np.uint8)
    for ch, v in {"=": 0, "A": 1, "C": 2, "G": 4, "T": 8, "N": 15}.items():
        code[ord(ch)] = v
    cig, coff, soff, blob, nbytes = [], np.zeros(n, np.uint32), np.full(n, NO_SEQ, np.uint64), [], 0
    for i, r in enumerate(recs):
        coff[i] = len(cig)
        cig += [(l << 4) | OPS.index(op) for l, op in r["ops"]]
        if ship_all or M.is_candidate(r):
            lq = r["lq"]
            c = code[np.frombuffer(r["seq"].encode(), np.uint8)]
            if lq & 1:
                c = np.concatenate([c, np.zeros(1, np.uint8)])
            soff[i] = nbytes
            blob += [(c[0::2] << 4) | c[1::2], np.asarray(r["qual"], np.uint8)]
            nbytes += (lq + 1) // 2 + lq
    if pad:
        blob.append(np.zeros(16, np.uint8))
    b.update(cigar=np.array(cig, np.uint32), cigar_off=coff, seq_off=soff, seqqual=np.concatenate(blob) if blob else np.zeros(0, np.uint8),
             max_ref_span=max([1] + [r["span"] for r in recs]))
    if ends:
        b["cigar_ends"] = np.array([(OPS.index(r["ops"][0][1]) | OPS.index(r["ops"][-1][1]) << 4) if r["ops"] else 0xff for r in recs], np.uint8)
    return b


def make(name, family, recs, runs=("d", "q0"), kind="getclip", cutsets=(), own=None, initial_last_tid=0, passes=None, n_contigs=None, expect=None, **kw):
    nt = n_contigs or max(r["tid"] for r in recs) + 1
    top = max(r["pos"] + r["span"] for r in recs) + 1000
    assert len(recs) <= MAX_RECORDS
    return dict(name=name, family=family, names=[f"c{i}" for i in range(nt)], lens=[top] * nt, recs=recs, runs=tuple(runs), kind=kind,
                cutsets=[sorted(set(c)) for c in cutsets], own=own, initial_last_tid=initial_last_tid, passes=passes, expect=expect or {}, **kw)


def sorted_positions(n, start=100, step=2):
    return [start + step * i for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------
# ends: every pair of CIGAR end codes in every byte lane of a 16-byte load
# ---------------------------------------------------------------------------------------------------------------------
def ends_input(rot):
    S = Seqs(100 + rot)
    shapes = [[(7, a), (LQ - (7 if a in "MIS=X" else 0) - (6 if b in "MIS=X" else 0), "M"), (6, b)] for a in OPS for b in OPS]
    shapes += [[(LQ, a)] for a in OPS] + [[]]
    recs = [filler(0, 0) for _ in range(rot)]
    for k, ops in enumerate(shapes):
        safe = len(ops) > 0 and ops[0][1] in ("MSH" if len(ops) > 1 else "MS") and ops[-1][1] in "MSH"   # (the restrictions of random_sample(safe=True))
        lq = sum(l for l, op in ops if op in "MIS=X") if ops else LQ
        recs.append(rec(0, 0, ops, S.seq(lq), S.qual(lq), ref=safe))
    for i, p in enumerate(sorted_positions(len(recs), step=40)):
        recs[i]["pos"], recs[i]["mpos"] = p, p + 200
    return make(f"ends-{rot}", "ends", recs, cutsets=[[len(recs) // 2]])


# ---------------------------------------------------------------------------------------------------------------------
# tile_edges
# ---------------------------------------------------------------------------------------------------------------------
def tile_places(n, tiles=None):
    """record 0 and n - 1; in every tile (or in `tiles`): the first and last record of the tile and of its sub-tiles, records 15 and 16 (a lane's
    load), 1023 and 1024 (a wavefront's 64 lanes)"""
    out = {0, n - 1}
    for t in range((n + CC_TILE - 1) // CC_TILE):
        if tiles is None or t in tiles:
            out |= {t * CC_TILE + p for p in TILE_PLACES}
    return sorted(i for i in out if 0 <= i < n)


def tile_input(name, n, places, tail_all=False):
    S = Seqs(n + 7 * tail_all)
    kinds = ("5", "3", "both", "lowq", "3", "5")
    places = set(places)
    if tail_all:
        places |= set(range((n - 1) // CC_TILE * CC_TILE, n))
    recs, c = [], 0
    for i, p in enumerate(sorted_positions(n)):
        if i in places:
            recs.append(clipped(S, 0, p, kinds[c % 6], v=i))
            c += 1
        else:
            recs.append(filler(0, p))
    return make(name, "tile_edges", recs, cutsets=[[(2 * n) // 3 | 1]] if n > 2 else [], scan_variants=True, expect=dict(places=sorted(places)))


def tile_edge_sizes():
    return [k * CC_TILE + d for k in range(3) for d in TILE_DELTAS if k * CC_TILE + d > 0]


# ---------------------------------------------------------------------------------------------------------------------
# candidate_counts
# ---------------------------------------------------------------------------------------------------------------------
PATTERNS = ("both", "none", "3", "5", "alt", "lone0", "lone15", "lone16", "lone63", "gap")


def pattern_kinds(pattern, n):
    """the kinds of n candidates, or None where the pattern needs more of them"""
    none = lambda k: NONE_KINDS[k % 4]
    if pattern in ("both", "3", "5"):
        return [pattern] * n
    if pattern == "none":
        return [none(k) for k in range(n)]
    if pattern == "alt":
        return [(none(k // 5), "5", "3", "both", "xcboth")[k % 5] for k in range(n)]
    if pattern.startswith("lone"):
        p = int(pattern[4:])
        if p >= n:
            return None
        # in the last workgroup of 256 candidates that has such a place; the others dup and hard only, so that it is alone in every run
        base = (n - 1) // BLOCK * BLOCK if base_fits(n, p) else 0
        return [("dup", "hard")[k % 2] if k != base + p else ("5", "3", "both")[p % 3] for k in range(n)]
    if pattern == "gap":
        W = FILTER_WAVE
        return None if n < 3 * W else ["both"] * W + [("dup", "hard")[k % 2] for k in range(W)] + ["both"] * W + [(none(k // 4), "5", "3", "both")[k % 4] for k in range(n - 3 * W)]
    raise KeyError(pattern)


def base_fits(n, p):
    return (n - 1) // BLOCK * BLOCK + p < n


def counts_input(n, pattern):
    kinds = pattern_kinds(pattern, n)
    if kinds is None:
        return None
    S = Seqs(1000 + n)
    recs = []
    for k, kind in enumerate(kinds):   # a filler in front of every candidate but not of each third: the candidates' lines lie at changing distances
        if k % 3:
            recs.append(filler(0, 0))
        recs.append(clipped(S, 0, 0, kind, v=k))
    for i, p in enumerate(sorted_positions(len(recs))):
        recs[i]["pos"], recs[i]["mpos"] = p, p + 200
    n_rec = len(recs)
    return make(f"count-{n}-{pattern}", "candidate_counts", recs, runs=("d", "q0", "s"), cutsets=[[n_rec // 2 + 1]] if n_rec > 2 else [], scan_variants=True,
                expect=dict(n_cand=n, pattern=pattern))


# ---------------------------------------------------------------------------------------------------------------------
# contig_switch
# ---------------------------------------------------------------------------------------------------------------------
def switch_input(gap, flags, initial):
    """contigs t0 .. : [kept] | first (dropped), `gap` unmapped-pair records on another contig, second (kept) | two contigs of one clipped record
    (nothing) | first, gap, second again, and `gap` unmapped-pair records at the very end.  t0 = initial_last_tid: the first record is looked at"""
    S = Seqs(2000 + gap)
    t0 = initial
    recs, cand, runs = [], [], []
    pos = iter(range(100, 10 ** 7, 40))

    def unmapped(k):
        kind = ("5", "3", "both", None)[k % 4]   # some of them soft clipped: candidates of the scan that the flag test sends away
        r = clipped(S, t0 + 9, next(pos), kind, v=k, flag=(99 | flags) & ~2) if kind else filler(t0 + 9, next(pos), flag=(99 | flags) & ~2)
        return r

    recs.append(clipped(S, t0, next(pos), "both"))               # the first record of the input, on the contig the pass starts with: looked at
    recs.append(clipped(S, t0, next(pos), "5", v=1))
    for c, kinds in ((t0 + 1, ("3", "both")), (t0 + 4, ("both", "5"))):
        recs.append(clipped(S, c, next(pos), kinds[0]))          # a contig's first record: dropped
        runs.append((len(recs), len(recs) + gap))
        recs += [unmapped(k) for k in range(gap)]
        cand.append(len(recs))
        recs.append(clipped(S, c, next(pos), kinds[1], v=2))     # its second: kept, whatever lies in between
        recs.append(filler(c, next(pos)))
        if c == t0 + 1:
            recs.append(clipped(S, t0 + 2, next(pos), "both"))   # contigs of one record each
            recs.append(clipped(S, t0 + 3, next(pos), "3"))
    runs.append((len(recs), len(recs) + gap))
    recs += [unmapped(k) for k in range(gap)]
    cutsets = [[cand[0]], [cand[1]]]                             # in front of the candidate: with gap 300 the batch before ends with 300 unmapped-pair records
    if gap >= 1:
        a, b = runs[0]
        cutsets.append([a + gap // 2])                           # inside the run
        cutsets.append([runs[1][0], runs[1][1]])                 # a batch of unmapped-pair records only
        if gap >= 15:
            cutsets.append([a + 1, b - 1, runs[2][0]])
    names = {4: "u", 8: "m", 12: "um"}
    return make(f"switch-{gap}-{names[flags]}-{initial}", "contig_switch", recs, cutsets=cutsets, initial_last_tid=initial, n_contigs=t0 + 10,
                expect=dict(kept=[0, 1] + cand, runs=runs, gap=gap))


# ---------------------------------------------------------------------------------------------------------------------
# ranges_and_ownership
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def range_records():
    """three contigs of 40 records, every fifth a candidate: '5', '3', 'both' in turn; the first record of contigs 1 and 2 is a candidate too"""
    S = Seqs(3000)
    recs = []
    for tid in range(3):
        for k, p in enumerate(sorted_positions(40, start=1000, step=50)):
            recs.append(clipped(S, tid, p, ("5", "3", "both")[(k // 5 + tid) % 3], v=k) if k % 5 == 0 or (k == 1 and tid) else filler(tid, p))
    return recs


def range_inputs():
    recs = range_records()
    n = len(recs)
    out = []
    c = 45                                           # a candidate in the middle of contig 1
    assert M.is_candidate(recs[c]) and M.is_candidate(recs[85]) and recs[39]["tid"] != recs[40]["tid"] and M.is_candidate(recs[40]) and M.is_candidate(recs[41])
    cases = {"r0-on": (c, n), "r0-behind": (c + 1, n), "r1-on": (0, c), "r1-behind": (0, c + 1), "empty": (c, c), "r1-zero": (0, 0),
             "r0-contig-first": (40, n), "r0-contig-second": (41, n)}
    for name, (r0, r1) in cases.items():
        out.append(make(f"range-{name}", "ranges_and_ownership", recs, kind="passes", passes=[dict(initial_last_tid=0, scans=[(0, n, r0, r1)])]))
    # two passes that share the batch at a cut (what Context.getclip does where a contig comes back), the second continuing from the first's state
    out.append(make("range-two-passes", "ranges_and_ownership", recs, kind="passes",
                    passes=[dict(initial_last_tid=0, scans=[(0, n, 0, c)]), dict(initial_last_tid=1, scans=[(0, n, c, n)])]))
    # ranges inside two batches of one pass
    out.append(make("range-two-batches", "ranges_and_ownership", recs, kind="passes", passes=[dict(initial_last_tid=0, scans=[(0, 60, 5, 46), (60, n, 15, n - 60)])]))
    return out


def own_inputs():
    recs = range_records()
    ev, _ = M.clip_events([(recs, None)])
    k5 = next(e for e in ev if e.side == 0 and e.tid == 1 and e.rec > 50)
    k3 = next(e for e in ev if e.side == 1 and e.tid == 1 and e.rec > 50)
    both = next(e for e in ev if e.tid == 1 and e.rec > 50 and len(recs[e.rec]["ops"]) == 3)
    first, last = (0, 0), (3, 0)
    out = []
    for tag, e in (("5", k5), ("3", k3)):
        for d in (-1, 0, 1):
            out.append(make(f"own-lo-{tag}{d:+d}", "ranges_and_ownership", recs, own=((e.tid, e.pos + d), last), cutsets=[[e.rec]], expect=dict(key=e, d=d, edge="lo")))
            out.append(make(f"own-hi-{tag}{d:+d}", "ranges_and_ownership", recs, own=(first, (e.tid, e.pos + d)), cutsets=[[e.rec]], expect=dict(key=e, d=d, edge="hi")))
    p5, p3 = recs[both.rec]["pos"] + 1, recs[both.rec]["pos"] + 14
    out.append(make("own-both-5in", "ranges_and_ownership", recs, own=(first, (1, p5 + 5)), cutsets=[[both.rec]], expect=dict(rec=both.rec, sides=[0])))
    out.append(make("own-both-3in", "ranges_and_ownership", recs, own=((1, p5 + 5), last), cutsets=[[both.rec]], expect=dict(rec=both.rec, sides=[1])))
    out.append(make("own-across", "ranges_and_ownership", recs, own=((0, 2000), (2, 2000)), cutsets=[[60]]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# side_order
# ---------------------------------------------------------------------------------------------------------------------
def far_end(S, tid, pos, reach):
    """a right-clipped read whose deletion carries its end `reach` bases past where its neighbours' lie (pos + 20)"""
    return rec(tid, pos, [(10, "M"), (reach, "D"), (10, "M"), (10, "S")], S.seq(), S.qual())


def inversion_records(S, tid, before, places, behind=40):
    """right-clipped reads two bases apart; the one at list place `before` ends past the ends of the next `places` of them"""
    recs = []
    for i, p in enumerate(sorted_positions(before + 1 + places + behind)):
        recs.append(far_end(S, tid, p, 2 * places + 1) if i == before else clipped(S, tid, p, "3", v=i))
    return recs


def order_inputs():
    out = []
    for where, before in (("start", 10), ("straddle", WS_TILE - 16)):
        for places in (WS_W, WS_W + 1):
            S = Seqs(4000 + places)
            out.append(make(f"order-{where}-{places}", "side_order", inversion_records(S, 0, before, places), cutsets=[[before + 3]],
                            expect=dict(inversion=places, at=before)))
    # equal keys: three reads of different starts and one end ('3'), three of one start ('5'); homopolymers of different bases
    S = Seqs(4100)
    recs = [filler(0, 100)]
    for k, base in enumerate("ACG"):
        recs.append(rec(0, 200 + 2 * k, [(24 - 2 * k, "M"), (6 + 2 * k, "S")], base * LQ, S.qual()))
        recs.append(filler(0, 201 + 2 * k))
    for k, base in enumerate("ACGT"):
        recs.append(rec(0, 300, [(5 + k, "S"), (25 - k, "M")], base * LQ, S.qual()))
    out.append(make("order-equal-keys", "side_order", recs, cutsets=[[3], [9]], expect=dict(bins={(1, 224): 3, (0, 301): 4})))
    # one contig whose positions fall: the '5' keys descend; equal keys on both sides, in BAM order
    S = Seqs(4200)
    recs = []
    for i, p in enumerate(reversed(sorted_positions(120, step=6))):
        kind = ("5", "3", "both", None)[i % 4]
        recs.append(clipped(S, 0, p, kind, v=i) if kind else filler(0, p))
        if i in (40, 41, 42):   # twice the same start: two '5' / two '3' / two of each with one key
            recs[-1]["seq"] = "A" * LQ
            recs.append(dict(clipped(S, 0, p, kind, v=i + 1), seq="C" * LQ))
    out.append(make("order-falling", "side_order", recs, cutsets=[[50]], expect=dict(falling=True)))
    # contig ids far apart, events on few of them
    S = Seqs(4300)
    recs = []
    kinds = {1: ("5", "5"), 2: ("3", "3"), 255: ("both",), 256: ("5", "3"), 257: (), 4096: ("3", "both", "5"), 70000: ("both", "3")}
    for tid in CONTIG_IDS:
        ps = iter(sorted_positions(10, step=30))
        recs.append(clipped(S, tid, next(ps), "both"))   # dropped
        recs += [clipped(S, tid, next(ps), k, v=j) for j, k in enumerate(kinds[tid])]
        recs.append(filler(tid, next(ps)))
    # (not sent to the reference: the BAM writer of the tests puts the header into one BGZF block, and 70,001 contig names do not fit)
    out.append(make("order-contig-ids", "side_order", recs, cutsets=[[7]], n_contigs=CONTIG_IDS[-1] + 1, reference=False, expect=dict(contigs=kinds)))
    # the radix fallback with the width of the keys decided by the '3' list alone: '5' and '3' events on contigs 1 - 3, '3' events only - with an
    # inverted pair WS_W + 1 places apart - on contig 128, whose keys are the first to need a sixth digit of RADIX_BITS bits
    S = Seqs(4400)
    recs = []
    for tid in (1, 2, 3):
        ps = iter(sorted_positions(10, step=30))
        recs.append(filler(tid, next(ps)))
        recs += [clipped(S, tid, next(ps), k, v=j) for j, k in enumerate(("5", "3", "both", "3"))]
    recs.append(filler(KEY_BITS_CONTIG, 50))
    recs += inversion_records(S, KEY_BITS_CONTIG, 5, WS_W + 1, behind=8)
    out.append(make("order-key-bits", "side_order", recs, cutsets=[[20]], expect=dict(inversion=WS_W + 1, key_bits_by_3=True)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------
def long_ops(lq, n_cigar, right):
    """a clipped read of lq bases and n_cigar operations: 20S, then 1M 1D ... (the last of them 1I where it would be an M), then the rest as M"""
    mid = [(1, "MD"[k % 2]) for k in range(n_cigar - 2)]
    if mid[-1][1] == "M":
        mid[-1] = (1, "I")
    used = 20 + sum(l for l, op in mid if op in "MI")
    ops = [(20, "S")] + mid + [(lq - used, "M")]
    return ops[::-1] if right else ops


def gather_input():
    S = Seqs(5000)
    shapes = [(lq, None) for lq in GATHER_LQ if lq < 10] + [(lq, nc) for lq in GATHER_LQ if lq >= 10 for nc in GATHER_NCIG]
    small = {1: [(1, "S")], 2: [(1, "S"), (1, "M")], 3: [(2, "M"), (1, "S")], 5: [(2, "S"), (3, "M")]}
    shift = {0: None, 1: 3, 2: 1, 3: 2}   # bytes to move on -> the length of an unclipped read whose entry has that many mod 4 (5, 2 and 3 bytes)
    recs, entries, nbytes = [], [], 0
    pos = iter(range(100, 10 ** 8, 700))
    order = [(mis, k) for k in range(len(shapes)) for mis in range(4)]
    order.append(order.pop(order.index((3, len(shapes) - 1))))   # the last entry: 600 bases, three bytes off a dword, ends where the blob ends
    for j, (mis, k) in enumerate(order):
        lq, nc = shapes[k]
        d = (mis - nbytes) % 4
        if shift[d]:
            recs.append(rec(0, next(pos), [(shift[d], "M")], S.seq(shift[d]), S.qual(shift[d])))
            nbytes += (shift[d] + 1) // 2 + shift[d]
        ops = small[lq] if nc is None else long_ops(lq, nc, right=(k + mis) % 2 == 1)
        assert nbytes % 4 == mis
        entries.append((len(recs), mis, lq, len(ops)))
        recs.append(rec(0, next(pos), ops, S.seq(lq), S.qual(lq)))
        nbytes += (lq + 1) // 2 + lq
    return make("gather", "gather", recs, cutsets=[[len(recs) // 2]], ship_all=True, pad=False, expect=dict(entries=entries, nbytes=nbytes))


# ---------------------------------------------------------------------------------------------------------------------
# the list
# ---------------------------------------------------------------------------------------------------------------------
def _build():
    out = [ends_input(rot) for rot in range(16)]
    for n in tile_edge_sizes():
        out.append(tile_input(f"tile-{n}", n, tile_places(n)))
        out.append(tile_input(f"tile-{n}-tail", n, tile_places(n), tail_all=True))
    n = 5 * CC_TILE + 1
    out.append(tile_input(f"tile-{n}", n, tile_places(n)))
    out.append(tile_input("tile-empty-middle", 3 * CC_TILE, tile_places(3 * CC_TILE, tiles=(0, 2))))
    out += [x for x in (counts_input(n, p) for n in CAND_COUNTS for p in PATTERNS) if x is not None]
    for gap in GAPS:
        for flags in (F_UNMAP, F_MUNMAP, F_UNMAP | F_MUNMAP) if gap else (F_UNMAP,):
            for initial in (0, 1):
                out.append(switch_input(gap, flags, initial))
    out += range_inputs() + own_inputs() + order_inputs() + [gather_input()]
    assert len({x["name"] for x in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def inputs():
    return {x["name"]: x for x in _build()}


@functools.lru_cache(maxsize=None)
def names(family=None):
    return [k for k, x in inputs().items() if family is None or x["family"] == family]


FAMILIES = ("ends", "tile_edges", "candidate_counts", "contig_switch", "ranges_and_ownership", "side_order", "gather")
FORMS = ("gather", "ends-5", "tile-8193", "count-65-alt", "switch-16-um-0", "own-across", "order-key-bits")   # the inputs that run in the three batch forms


def batches_of(x, cuts=()):
    """the input's records as host batches cut at `cuts`: [(records, batch)]"""
    edges = [0] + list(cuts) + [len(x["recs"])]
    kw = dict(ship_all=x.get("ship_all", False), pad=x.get("pad", True))
    return [(x["recs"][a:b], batch_of(x["recs"][a:b], **kw)) for a, b in zip(edges, edges[1:])]


@functools.lru_cache(maxsize=16)
def host_batches(name, cuts=(), ends=True):
    """the host batches of batches_of(inputs()[name], cuts), kept for the calls that follow (nobody writes into them); ends: with the cigar_ends column"""
    x = inputs()[name]
    edges = [0] + list(cuts) + [len(x["recs"])]
    return [batch_of(x["recs"][a:b], ends=ends, ship_all=x.get("ship_all", False), pad=x.get("pad", True)) for a, b in zip(edges, edges[1:])]


def passes_of(x):
    """every input as passes: [dict(initial_last_tid, own, scans [(records, (r0, r1) or None)])] - a "getclip" input is one pass over its one batch"""
    if x["kind"] == "getclip":
        return [dict(initial_last_tid=x["initial_last_tid"], own=x["own"], scans=[(x["recs"], None)])]
    return [dict(initial_last_tid=p["initial_last_tid"], own=None, scans=[(x["recs"][lo:hi], (r0, r1)) for lo, hi, r0, r1 in p["scans"]]) for p in x["passes"]]


@functools.lru_cache(maxsize=None)
def modelled(name, tag, ref_only=False):
    """-> (table, [(events, scans)] per pass) of the model for one run; ref_only: over the records that the reference defines"""
    x = inputs()[name]
    kw = RUN_KW[tag]
    tables, per_pass = [], []
    for p in passes_of(x):
        scans = [([r for r in recs if r["ref"]], rng) for recs, rng in p["scans"]] if ref_only else p["scans"]
        assert not ref_only or all(rng is None for _, rng in scans)
        ev, _ = M.clip_events(scans, own=p["own"], initial_last_tid=p["initial_last_tid"], **kw)
        tables.append(M.table(ev, scans))
        per_pass.append((ev, scans))
    return M.concat(tables), per_pass


def report_of(name, tag="d"):
    _, per_pass = modelled(name, tag)
    return [M.report(ev, scans, CC_TILE, SUB_TILE, FILTER_WAVE, FILTER_BLOCK, BLOCK) for ev, scans in per_pass]


def reference_defined(x):
    """the inputs that go to the real reference: whole, no ownership, no ranges, the contig the pass starts with being 0 as in the reference"""
    return x["kind"] == "getclip" and x["own"] is None and x["initial_last_tid"] == 0 and x.get("reference", True)
