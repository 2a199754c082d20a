"""Inputs of tests/test_realign_alts_gpu.py: one reference of a few kilobases with planted elements, and query sets built for one rule of the
alternate loci each.  tests/test_realign_alts_inputs.py runs the model alone over every set and holds each set to the property it
was built for; a set that misses its property is changed here, not excused there.

Every set is (queries, labels).  The reference is reference(); where(name) is the global position of a planted piece.  The set with more than 64
distinct candidates is realign_inputs.sweep_set() (its own reference), the flags set wants the sorted index with the cap FLAGS_CAP."""
import functools

import numpy as np

from realign_inputs import dna, other, revcomp, sub, unlike

CAP = 500        # the sorted index's cap for every set but flags_set
FLAGS_CAP = 3
NAMES = tuple(f"a{i}" for i in range(8))
N_FAMILY = 18    # copies of the family element: the primary and 17 alternate loci, one more than the largest max_alt


class _Ref:
    """contigs put together from random filler (an int: that many bases) and planted pieces (name, string)"""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.contigs, self.at = [], {}

    def contig(self, *pieces):
        base = sum(len(c) for c in self.contigs)
        s = ""
        for p in pieces:
            if isinstance(p, int):
                s += dna(self.rng, p)
            else:
                self.at[p[0]] = base + len(s)
                s += p[1]
        self.contigs.append(s)


def _elements():
    rng = np.random.RandomState(2201)
    return {k: dna(rng, n) for k, n in dict(ratio=60, eq=50, floor=36, order=60, span=60, both=60, t32=32, t33=33, supp=90, family=50, hang=56,
                                            gap=70, long=300, mask=80, pool=60).items()}


@functools.lru_cache(maxsize=None)
def _built():
    E = _elements()
    r = _Ref(2202)
    fam = [E["family"]] + [sub(E["family"], [25], None) for _ in range(N_FAMILY - 1)]   # copy 0 exact, the others with base 25 changed
    # a0: the ratio rule and its equality case (eq39 is the start of a4); the order set's reverse copy: before every forward copy, a smaller diagonal, the other strand
    r.contig(131, ("ratio0", E["ratio"]), 97, ("ratio2", sub(E["ratio"], [25, 50])), 113, ("ratio3", sub(E["ratio"], [24, 49, 54])), 89,
             ("eq0", E["eq"]), 101, ("eq40", sub(E["eq"], [24, 48])), 77, ("order_r", revcomp(sub(E["order"], [28]))), 58)
    # a1: the floor (30 and 29 leading bases of a 36-base element, then bases that match nowhere), the order set's forward copies
    r.contig(59, ("floor0", E["floor"]), 83, ("floor30", E["floor"][:30] + unlike(E["floor"][30:])), 71, ("floor29", E["floor"][:29] + unlike(E["floor"][29:])), 95,
             ("order_f2", sub(E["order"], [26])), 67, ("order0", E["order"]), 103, ("order_f1", sub(E["order"], [30])), 57)
    # a2: an element on both strands; the first 46 bases of `hang`; the contig ends inside a copy of `span` (its first 30 bases)
    r.contig(61, ("both_f", E["both"]), 79, ("both_r", revcomp(E["both"])), 107,
             ("hang46", E["hang"][:46]), 53, ("span_a", E["span"][:30]))
    # a3: ... and a3 begins with the other 30 bases of `span`: one diagonal, two contigs; the primary of that query holds its first 36 bases
    r.contig(("span_b", E["span"][30:]), 73, ("span36", E["span"][:36] + unlike(E["span"][36:])), 87, ("hang0", E["hang"]), 99,
             ("t32", E["t32"] * 2), 3, 81, ("t33", E["t33"] * 2), 64)
    # a4: starts with eq's bases 1..49 carrying two substitutions: 49 bases inside the contig, no extension over the contig's start: 47 - 8 = 39
    r.contig(("eq39", sub(E["eq"], [24, 48])[1:]), 93, ("supp0", E["supp"][:48] + unlike(E["supp"][48:])), 85,
             ("supp_del", E["supp"][:43] + E["supp"][48:]), 102)   # a 5-base deletion: two diagonals of one locus, 43 and 42 bases
    # a5: the family
    pieces = [47]
    for i, f in enumerate(fam):
        pieces += [(f"family{i}", f), 9 + (i * 7) % 13]
    r.contig(*pieces)
    # a6: the gapped set and the flags set
    g = E["gap"]
    r.contig(66, ("gap_locus", g[:35] + g[37:]), 90, ("gap32", g[:32] + unlike(g[32:52])), 75, ("long0", E["long"]), 44, ("long1", E["long"]), 48, ("long2", E["long"]), 60)
    m = E["mask"]
    r.contig(52, ("mask0", m), 36, ("mask1", m), 28, *sum(([(f"mask_head{i}", m[:40]), 24] for i in range(4)), []), ("pool", E["pool"]), 40, ("pool_b", sub(E["pool"], [27])), 33)
    assert len(r.contigs) == len(NAMES)
    return tuple(r.contigs), dict(r.at), E


def reference():
    return _built()[0]


def where(name):
    return _built()[1][name]


def element(name):
    return _built()[2][name]


class _Set:
    def __init__(self):
        self.q, self.lab = [], []

    def add(self, label, s, both=True):
        self.q.append(s)
        self.lab.append(label + "/fwd")
        if both:
            self.q.append(revcomp(s))
            self.lab.append(label + "/rev")

    def done(self):
        assert len(set(self.lab)) == len(self.lab)
        return tuple(self.q), tuple(self.lab)


@functools.lru_cache(maxsize=None)
def ratio_set():
    """60 exact bases; a copy with 2 substitutions scores 50 (250 >= 240: in), one with 3 scores 45 (out).  The equality case: 50 exact bases, a copy
    with two substitutions scores 40 (200 >= 200: in), the same copy short of its first base at a contig's start 39 (out)"""
    s = _Set()
    s.add("ratio", element("ratio"))
    s.add("equality", element("eq"))
    return s.done()


@functools.lru_cache(maxsize=None)
def floor_set():
    """best 36, so the ratio asks for 29: a locus with 30 leading bases is in, one with 29 passes the ratio but is not scored (below 30)"""
    s = _Set()
    s.add("floor", element("floor"))
    return s.done()


@functools.lru_cache(maxsize=None)
def order_set():
    """three loci at 55 behind an exact primary: forward ones by diagonal, the reverse one last although its diagonal is the smallest.  And one diagonal in two
    contigs: a 60-base sequence whose halves end a2 and begin a3 (30 and 30) behind a primary of 36: the smaller contig id first; both alternates hang over a contig's end"""
    s = _Set()
    s.add("order", element("order"), both=False)
    s.add("contig", element("span"), both=False)
    return s.done()


@functools.lru_cache(maxsize=None)
def strand_set():
    """an element present forward and reverse-complemented: either query finds the other copy on the other strand with the same score"""
    s = _Set()
    s.add("both", element("both"))
    return s.done()


@functools.lru_cache(maxsize=None)
def tandem_set():
    """a unit of 32 bases twice in a row: the second copy is the primary's locus (no alternate, and no `second`); a unit of 33: two loci"""
    s = _Set()
    s.add("tandem32", element("t32") + element("t32")[:8])
    s.add("tandem33", element("t33") + element("t33")[:8])
    return s.done()


@functools.lru_cache(maxsize=None)
def suppress_set():
    """90 bases: the primary holds the first 48; another locus holds them around a 5-base deletion - two diagonals 5 apart, 43 and 42 bases, both qualify, neither
    is the primary's locus: the first is an alternate, the second is suppressed by THAT alternate, and nothing is cut at max_alt 1"""
    s = _Set()
    s.add("suppress", element("supp"))
    return s.done()


@functools.lru_cache(maxsize=None)
def family_set():
    """an element in 18 copies: 17 alternate loci at 45 behind the exact primary, by diagonal; max_alt 1, 2 and 16 all cut"""
    s = _Set()
    s.add("family", element("family"))
    return s.done()


@functools.lru_cache(maxsize=None)
def hang_set():
    """a locus that holds the first 46 of 56 bases (230 >= 224): an alternate with a clipped end.  (Alternates that hang over a contig's end: order_set's "contig")"""
    s = _Set()
    s.add("hang", element("hang"))
    return s.done()


@functools.lru_cache(maxsize=None)
def gapped_set():
    """gapped mode.  "gain": 70 bases whose primary locus lacks two bases in the middle (first stage 35, 60 with the two inserted bases) and another locus with the first 32
    bases: an alternate at 32 >= 0.8 x 35, its `second` the first stage's 35.  "late": 30 matching bases and a mismatch on the last one, cheaper to take than to
    clip (26): the floor lets it through, the refinement leaves it unaligned, no alternates.  "rescue" / "stays": 25 | 25 around a 1-base gap, and 25 alone"""
    ref, at = reference(), where
    text = "".join(ref)
    s = _Set()
    s.add("gain", element("gap"))
    p = at("ratio0")
    s.add("late", text[p:p + 30] + other(text[p + 30]))
    p = at("hang0")
    s.add("rescue", text[p:p + 25] + text[p + 26:p + 51])
    s.add("stays", text[p:p + 25] + unlike(text[p + 25:p + 50]))
    return s.done()


@functools.lru_cache(maxsize=None)
def flags_set():
    """the sorted index with the cap FLAGS_CAP.  "overflow": 300 bases at three loci, 210 seeds: OVERFLOW, two alternates.  "masked": 80 bases at two loci whose
    first 40 occur four more times: their 20-mers give no seed (MASKED), the rest finds both loci.  "family": every 20-mer masked or not, as the model has it"""
    s = _Set()
    s.add("overflow", element("long"))
    s.add("masked", element("mask"))
    s.add("family", element("family"))
    return s.done()


N_MIX = 2055   # more than one tile of the scan (2048), no multiple of the four wavefronts of a workgroup


@functools.lru_cache(maxsize=None)
def mix_set():
    """2055 queries: with alternates (the sets above), unique substrings with 0-2 substitutions, random sequence, 19 and 1025 bases, in a fixed shuffle"""
    rng = np.random.RandomState(2203)
    ref = reference()
    plain = [c for i, c in enumerate(ref) if i not in (5, 6)]   # substrings of one contig, and not of the family's or the 300-base copies': at most 192 seeds
    with_alts = [q for fn in (ratio_set, floor_set, order_set, strand_set, tandem_set, suppress_set, family_set, hang_set) for q in fn()[0]]
    q, lab = [], []
    for i in range(N_MIX):
        kind = i % 7
        if kind in (0, 4):
            q.append(with_alts[int(rng.randint(len(with_alts)))] if i < 2048 else element("family")); lab.append(f"mix{i}-planted")   # (behind the scan's first tile: one that has alternates)
        elif kind == 5 and i % 3 == 0:
            q.append(dna(rng, int(rng.randint(30, 90)))); lab.append(f"mix{i}-random")
        elif kind == 6 and i % 5 == 0:
            n = 19 if i % 2 else 1025
            text = plain[int(rng.randint(len(plain)))] if n == 19 else "".join(ref)
            p = int(rng.randint(0, len(text) - n))
            q.append(text[p:p + n]); lab.append(f"mix{i}-len{n}")
        else:
            n = int(rng.randint(35, 110))
            text = plain[int(rng.randint(len(plain)))]
            p = int(rng.randint(0, len(text) - n))
            x = sub(text[p:p + n], sorted(set(int(v) for v in rng.randint(0, n, int(rng.randint(3))))), rng)
            q.append(x if i % 2 else revcomp(x)); lab.append(f"mix{i}-sub")
    assert len(q) == N_MIX and N_MIX > 2048 and N_MIX % 4
    return tuple(q), tuple(lab)


SETS = dict(ratio=ratio_set, floor=floor_set, order=order_set, strand=strand_set, tandem=tandem_set, suppress=suppress_set, family=family_set, hang=hang_set,
            gapped=gapped_set)


@functools.lru_cache(maxsize=None)
def all_queries():
    """every set of SETS, one after the other, then the mix -> (queries, labels with the set's name in front)"""
    q, lab = [], []
    for name, fn in list(SETS.items()) + [("mix", mix_set)]:
        a, b = fn()
        q.extend(a)
        lab.extend(f"{name}:{x}" for x in b)
    return tuple(q), tuple(lab)


@functools.lru_cache(maxsize=None)
def cli_set():
    """`seeksv realign -S`: the queries of SETS and the first 200 of the mix that fit a read name (254 characters), each once -> [(sequence, quality)]"""
    rng = np.random.RandomState(2204)
    seen, out = set(), []
    for q in [x for fn in SETS.values() for x in fn()[0]] + list(mix_set()[0][:200]):
        if 0 < len(q) <= 254 and q not in seen:
            seen.add(q)
            out.append((q, "".join(chr(33 + int(x)) for x in rng.randint(2, 41, len(q)))))
    return tuple(out)


# ---- end to end through getsv: a breakpoint whose far side lies in copy 3 of a 5-copy element ----
E2E_NAMES, E2E_LENS = ("tA", "tB"), (2003, 2102)
E2E_ELEMENT, E2E_COPIES = 80, (300, 620, 910, 1230, 1540)   # tB: where the copies begin
E2E_A = 1000                       # 0-based: the last base of tA before the breakpoint
E2E_B = E2E_COPIES[2] + 10         # the first base of tB behind it: 10 bases into copy 3
E2E_CLIP = 60                      # the clip ends 10 bases before the copy does: every base of it is the element's
E2E_SV_OPTS = []                   # getsv's defaults


@functools.lru_cache(maxsize=None)
def e2e_sample():
    """-> (contigs, records for bamio.write_bam, coordinate-sorted).  Background: proper pairs of 100-base reads over both contigs.  The junction: ten
    reads that end at tA's base E2E_A and go on with 60 bases of tB from E2E_B on as a soft clip; their mates lie on tB behind copy 3, reverse, in
    unique sequence.  The reads of the other side begin inside the element: their aligner gave them MAPQ 0, and getclip drops them.  The clip's 60
    bases occur five times: an aligner that writes one record puts them at copy 1."""
    rng = np.random.RandomState(2301)
    a, b = dna(rng, E2E_LENS[0]), list(dna(rng, E2E_LENS[1]))
    el = dna(rng, E2E_ELEMENT)
    for p in E2E_COPIES:
        b[p:p + E2E_ELEMENT] = el
    b = "".join(b)
    recs = []
    qual = lambda n: "".join(chr(33 + 30 + int(x)) for x in rng.randint(0, 10, n))  # noqa: E731
    for tid, c in enumerate((a, b)):
        for i, p in enumerate(range(5, len(c) - 320, 13)):
            name = f"bg{tid}_{i}"
            recs.append(dict(qname=name, flag=99, tid=tid, pos=p, mapq=60, cigar="100M", mtid=tid, mpos=p + 200, isize=300, seq=c[p:p + 100], qual=qual(100)))
            recs.append(dict(qname=name, flag=147, tid=tid, pos=p + 200, mapq=60, cigar="100M", mtid=tid, mpos=p, isize=-300, seq=c[p + 200:p + 300], qual=qual(100)))
    for i in range(10):
        m = 36 + 3 * i   # aligned bases on tA
        p = E2E_A + 1 - m
        mp = E2E_B + 150 + 7 * i
        seq = a[p:E2E_A + 1] + b[E2E_B:E2E_B + E2E_CLIP]
        recs.append(dict(qname=f"jn{i}", flag=97, tid=0, pos=p, mapq=60, cigar=f"{m}M{E2E_CLIP}S", mtid=1, mpos=mp, isize=0, seq=seq, qual=qual(len(seq))))
        recs.append(dict(qname=f"jn{i}", flag=145, tid=1, pos=mp, mapq=60, cigar="100M", mtid=0, mpos=p, isize=0, seq=b[mp:mp + 100], qual=qual(100)))
    for i in range(5):   # the repeat side's own clipped reads: 40 bases of tA before the breakpoint as a soft clip, 45 + 5 i bases of tB; MAPQ 0
        m = 45 + 5 * i
        seq = a[E2E_A + 1 - 40:E2E_A + 1] + b[E2E_B:E2E_B + m]
        recs.append(dict(qname=f"rp{i}", flag=0, tid=1, pos=E2E_B, mapq=0, cigar=f"40S{m}M", mtid=-1, mpos=-1, isize=0, seq=seq, qual=qual(len(seq))))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return (a, b), tuple(recs)
