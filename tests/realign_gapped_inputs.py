"""Inputs of tests/test_realign_gapped_gpu.py: one reference of random contigs and query sets built for one rule of the gapped re-aligner each
(DESIGN.md 10c).  tests/test_realign_gapped_inputs.py runs the model alone over every set and holds each set to the property it was built for, so
the seeds below were chosen on the CPU; a set that misses its property is changed here, not excused there.

Every set is (queries, labels); every query comes on both strands (label + "/fwd", "/rev").  The reference is reference()."""
import functools

import numpy as np

from realign_inputs import JUNK_BYTES, dna, offsets, other, revcomp, sub

# ten contigs of 1-2 kb; offsets that are no multiples of 4 or 32
LENS = [1531, 1027, 1999, 1205, 1751, 1001, 1337, 1122, 1877, 1409]
NAMES = [f"g{i}" for i in range(len(LENS))]
TANDEM_CONTIG, TANDEM_AT, TANDEM_UNIT, TANDEM_COPIES = 4, 700, "CAG", 6
HOMO_CONTIG, HOMO_AT, HOMO_LEN = 6, 640, 8


@functools.lru_cache(maxsize=None)
def reference():
    """the contigs; contig 4 carries (CAG) x 6 at 700 and contig 6 an A x 8 at 640, both between bases that do not continue them"""
    rng = np.random.RandomState(1301)
    c = [dna(rng, n) for n in LENS]
    assert all(o % 4 and o % 32 for o in offsets(c)[1:-1])

    def plant(t, at, what):
        s = c[t]
        c[t] = s[:at - 1] + other(what[-1]) + what + other(what[0]) + s[at + len(what) + 1:]
    plant(TANDEM_CONTIG, TANDEM_AT, TANDEM_UNIT * TANDEM_COPIES)
    plant(HOMO_CONTIG, HOMO_AT, "A" * HOMO_LEN)
    assert [len(x) for x in c] == LENS
    return tuple(c)


def gapped(c, p, n, kind, L, at, rng):
    """n query bases from contig string c at p with one gap: "D": L reference bases are missing before query base `at`; "I": L bases that do not
    continue the reference are inserted at `at`"""
    if kind == "D":
        return c[p:p + at] + c[p + at + L:p + L + n]
    ins = "".join(other(c[p + at + i], 1 + int(rng.randint(3))) for i in range(L))
    return c[p:p + at] + ins + c[p + at:p + n - L]


class _Set:
    def __init__(self):
        self.q, self.lab = [], []

    def add(self, label, s):
        self.q.extend([s, revcomp(s)])
        self.lab.extend([label + "/fwd", label + "/rev"])

    def done(self):
        assert len(set(self.lab)) == len(self.lab)
        return tuple(self.q), tuple(self.lab)


def _spot(rng, c, n, margin=40):
    return int(rng.randint(margin, len(c) - n - margin))


@functools.lru_cache(maxsize=None)
def length_set():
    """D and I of 1, 2, 16 and 17 bases in the middle of a 100-base query: label "<kind><L>-<copy>"; 17 has to come back without a gap"""
    ref, rng, s = reference(), np.random.RandomState(1), _Set()
    for kind in "DI":
        for L in (1, 2, 16, 17):
            for copy in range(3):
                c = ref[(copy * 3 + L) % len(ref)]
                p = _spot(rng, c, 120)
                s.add(f"{kind}{L}-{copy}", gapped(c, p, 100, kind, L, 50, rng))
    return s.done()


PLACES = ("middle", "22-from-start", "22-from-end", "7-from-start", "8-from-start", "7-from-end", "8-from-end")


@functools.lru_cache(maxsize=None)
def place_set():
    """a 1-base gap in a 60-base query: in the middle; 22 bases from either end (the short side alone has no 23 bases that guarantee a seed); 7 and 8
    bases from either end, the two sides of the break-even (7 matches pay for the gap exactly: no gap; 8 win a point).  label "<kind>-<place>-<copy>".
    The base next to the gap on the short side is made to mismatch along the long side's diagonal, so that the ungapped alignment does not win a
    point there by chance."""
    ref, rng, s = reference(), np.random.RandomState(2), _Set()
    n = 60
    for kind in "DI":
        for place in PLACES:
            for copy in range(3):
                c = ref[(copy * 2 + len(place)) % len(ref)]
                short = int(place.split("-")[0]) if place != "middle" else 30
                left_short = place.endswith("start") or place == "middle"
                at = short if left_short else n - short - (1 if kind == "I" else 0)   # I: the inserted base is query base `at`, the short side follows it
                for _ in range(200):
                    p = _spot(rng, c, n + 2)
                    q = gapped(c, p, n, kind, 1, at, rng)
                    # the neighbour of the gap on the short side, placed on the long side's diagonal
                    if left_short:   # long side = right piece, diagonal p + g: query base at - 1 lies on reference p + g + at - 1
                        g = 1 if kind == "D" else -1
                        ok = q[at - 1] != c[p + g + at - 1] and (kind == "D" or q[at] != c[p + g + at])   # (and the inserted base)
                    else:            # long side = left piece, diagonal p: query base j = at (D) / at + 1 (I) lies on reference p + j
                        j = at + (1 if kind == "I" else 0)
                        ok = q[j] != c[p + j]
                    if ok:
                        break
                s.add(f"{kind}-{place}-{copy}", q)
    return s.done()


@functools.lru_cache(maxsize=None)
def side_set():
    """which piece the winner becomes: a 2-base gap at 60 of 100 (the winner is the left piece) and at 40 of 100 (the right piece)"""
    ref, rng, s = reference(), np.random.RandomState(3), _Set()
    for kind in "DI":
        for at, side in ((60, "left"), (40, "right")):
            for copy in range(3):
                c = ref[(copy + at) % len(ref)]
                s.add(f"{kind}-winner-{side}-{copy}", gapped(c, _spot(rng, c, 120), 100, kind, 2, at, rng))
    return s.done()


@functools.lru_cache(maxsize=None)
def rescue_set():
    """below 30 on either side of the gap: 25 | 25 around a gap of 1 or 2 bases ("rescue-..."; unaligned without the gap, aligned with it), and 25
    matching bases with a random remainder ("stays-...": unaligned either way)"""
    ref, rng, s = reference(), np.random.RandomState(4), _Set()
    for kind in "DI":
        for L in (1, 2):
            for copy in range(3):
                c = ref[(copy * 3 + L + (kind == "I")) % len(ref)]
                s.add(f"rescue-{kind}{L}-{copy}", gapped(c, _spot(rng, c, 60), 50 + (L if kind == "I" else 0), kind, L, 25, rng))
    for copy in range(4):
        c = ref[copy + 2]
        p = _spot(rng, c, 60)
        tail = dna(rng, 25)
        s.add(f"stays-head25-{copy}", other(c[p - 1]) + c[p:p + 25] + other(c[p + 25]) + tail)
        s.add(f"stays-tail25-{copy}", tail + other(c[p - 1]) + c[p:p + 25] + other(c[p + 25]))
    return s.done()


@functools.lru_cache(maxsize=None)
def edge_set():
    """a right piece that runs over its contig's end into the next contig's bases, and a left piece that begins before its contig's start: the piece
    is cut at the contig's edge.  label "over-end<t>-..." / "before-start<t>-..." """
    ref, rng, s = reference(), np.random.RandomState(5), _Set()
    text, off = "".join(ref), offsets(ref)
    for t in (1, 3, 6, 8):
        lo, hi = off[t], off[t + 1]
        for kind in "DI":
            for over in (1, 9):
                # 40 bases, the gap (2), 30 bases of which `over` lie behind the contig's end
                p = hi - 40 - 2 - (30 - over) if kind == "D" else hi - 40 - (30 - over)
                s.add(f"over-end{t}-{kind}-{over}", gapped(text, p, 70 + (2 if kind == "I" else 0), kind, 2, 40, rng))
                # `over` bases before the contig's start + 30 - over, the gap, 40 bases
                p = lo - over
                s.add(f"before-start{t}-{kind}-{over}", gapped(text, p, 70 + (2 if kind == "I" else 0), kind, 2, 30, rng))
    return s.done()


@functools.lru_cache(maxsize=None)
def repeat_set():
    """the gap inside a tandem repeat and inside a homopolymer: one unit more / fewer than the reference has; the gap has to come back at the
    repeat's first base (the smallest k)"""
    ref, s = reference(), _Set()
    c = ref[TANDEM_CONTIG]
    a, b = TANDEM_AT, TANDEM_AT + len(TANDEM_UNIT) * TANDEM_COPIES
    for left in (30, 41):
        s.add(f"tandem-unit-less-{left}", c[a - left:a] + TANDEM_UNIT * (TANDEM_COPIES - 1) + c[b:b + 71 - left])
        s.add(f"tandem-unit-more-{left}", c[a - left:a] + TANDEM_UNIT * (TANDEM_COPIES + 1) + c[b:b + 71 - left])
    c = ref[HOMO_CONTIG]
    a, b = HOMO_AT, HOMO_AT + HOMO_LEN
    for left in (28, 40):
        s.add(f"homopolymer-2-less-{left}", c[a - left:a] + "A" * (HOMO_LEN - 2) + c[b:b + 66 - left])
        s.add(f"homopolymer-1-more-{left}", c[a - left:a] + "A" * (HOMO_LEN + 1) + c[b:b + 66 - left])
    return s.done()


@functools.lru_cache(maxsize=None)
def substitution_set():
    """substitutions only, 1-4 of them anywhere in 80-150 bases: no gap, and the hit of the ungapped aligner"""
    ref, rng, s = reference(), np.random.RandomState(7), _Set()
    for copy in range(16):
        c = ref[copy % len(ref)]
        n = int(rng.randint(80, 151))
        p = _spot(rng, c, n)
        s.add(f"sub-{copy}", sub(c[p:p + n], sorted(set(int(x) for x in rng.randint(0, n, 1 + copy % 4))), rng))
    return s.done()


@functools.lru_cache(maxsize=None)
def limit_set():
    """the shortest and the longest query: 20 exact bases (below 30: unaligned), 1,024 bases with a 1-base gap 19 bases from an end (the 19 bases
    hold no seed: more than 192 seeds, but all on one diagonal), 1,024 exact bases, 1,025 bases"""
    ref, rng, s = reference(), np.random.RandomState(8), _Set()
    c = ref[2]
    s.add("exact-20", c[300:320])
    s.add("exact-1024", c[401:1425])
    s.add("long-1025", c[401:1426])
    for kind in "DI":
        s.add(f"long-{kind}-19-from-end", gapped(c, 333, 1024, kind, 1, 1024 - 19 - (kind == "I"), rng))
        s.add(f"long-{kind}-19-from-start", gapped(ref[8], 222, 1024, kind, 1, 19, rng))
    return s.done()


@functools.lru_cache(maxsize=None)
def junk_set():
    """bytes that are no bases next to the gap: on the last base before it, on the first behind it, on both; and in place of the inserted bases"""
    ref, rng, s = reference(), np.random.RandomState(9), _Set()
    for kind in "DI":
        for where in ("before", "behind", "both", "inserted"):
            if where == "inserted" and kind == "D":
                continue
            for copy in range(2):
                c = ref[(copy * 5 + len(where)) % len(ref)]
                q = list(gapped(c, _spot(rng, c, 100), 80, kind, 3, 40, rng))
                j = 40 + (3 if kind == "I" else 0)
                spots = dict(before=[39], behind=[j], both=[39, j], inserted=[40, 41, 42])[where]
                for at in spots:
                    q[at] = JUNK_BYTES[int(rng.randint(len(JUNK_BYTES)))]
                s.add(f"junk-{kind}-{where}-{copy}", "".join(q))
    return s.done()


N_MANY = 151   # x 2 strands = 302 queries: more than 256, and no multiple of the four wavefronts of a workgroup


@functools.lru_cache(maxsize=None)
def many_set():
    """302 queries of 40-120 bases: a gap of 1-16 bases anywhere at least 12 bases from the ends, 0-2 substitutions, now and then a lower-case run
    or an unrelated tail"""
    ref, rng, s = reference(), np.random.RandomState(10), _Set()
    for k in range(N_MANY):
        c = ref[int(rng.randint(len(ref)))]
        n = int(rng.randint(40, 121))
        kind, L = "DI"[int(rng.randint(2))], int(rng.randint(1, 17))
        if kind == "I" and n - L < 40:
            L = 1
        at = int(rng.randint(12, n - 12 - (L if kind == "I" else 0) + 1))
        q = gapped(c, _spot(rng, c, n + 20), n, kind, L, at, rng)
        q = sub(q, sorted(set(int(x) for x in rng.randint(0, n, int(rng.randint(3))))), rng)
        if k % 5 == 1:
            a = int(rng.randint(0, n))
            q = q[:a] + q[a:a + 20].lower() + q[a + 20:]
        if k % 7 == 3:
            q = q + dna(rng, int(rng.randint(1, 25)))
        s.add(f"many-{k}-{kind}{L}@{at}/{n}", q)
    assert len(s.q) > 256 and len(s.q) % 4
    return s.done()


SETS = dict(length=length_set, place=place_set, side=side_set, rescue=rescue_set, edge=edge_set, repeat=repeat_set, substitution=substitution_set,
            limit=limit_set, junk=junk_set, many=many_set)


@functools.lru_cache(maxsize=None)
def all_queries():
    """every set, one after the other -> (queries, labels with the set's name in front)"""
    q, lab = [], []
    for name, fn in SETS.items():
        a, b = fn()
        q.extend(a)
        lab.extend(f"{name}:{x}" for x in b)
    return tuple(q), tuple(lab)


@functools.lru_cache(maxsize=None)
def cli_set():
    """`seeksv realign -g` end to end: the queries of every set that fit a read name (254 characters), each once, with distinct qualities
    -> [(sequence, quality)]"""
    rng = np.random.RandomState(11)
    seen, out = set(), []
    for q in all_queries()[0]:
        if 0 < len(q) <= 254 and q not in seen:
            seen.add(q)
            out.append((q, "".join(chr(33 + int(x)) for x in rng.randint(2, 41, len(q)))))
    return tuple(out)


# ---- end to end through getsv: one inter-contig breakpoint whose partner side carries a small deletion ----
E2E_NAMES, E2E_LENS = ("tA", "tB"), (2003, 1802)
E2E_A, E2E_B = 1000, 700          # 0-based: the last base of tA before the breakpoint, the first base of tB behind it
E2E_DEL_AT, E2E_DEL = 26, 3       # the sample lacks tB[E2E_B + 26 : E2E_B + 29]
E2E_CLIP = 60
E2E_SV_OPTS = ["-f", "0", "-d", "0"]


@functools.lru_cache(maxsize=None)
def e2e_sample():
    """-> (contigs, records for bamio.write_bam, coordinate-sorted).  Background: proper pairs of 100-base reads over both contigs.  The junction:
    ten reads that end at tA's base E2E_A and go on with 60 bases of tB from E2E_B on - without the three bases at E2E_B + 26 - as a soft clip; their
    mates lie on tB, reverse.  Without a gap the clip aligns only behind the deletion (26S34M): the junction lands 29 bases off or is lost."""
    rng = np.random.RandomState(1401)
    a, b = dna(rng, E2E_LENS[0]), dna(rng, E2E_LENS[1])
    # the deletion cannot slide, and the first base behind it does not continue the clip's first 26 bases
    b = list(b)
    d0 = E2E_B + E2E_DEL_AT
    b[d0 - 1], b[d0], b[d0 + 1], b[d0 + 2], b[d0 + 3] = "A", "C", "G", "T", "G"
    b = "".join(b)
    partner = b[E2E_B:d0] + b[d0 + E2E_DEL:]   # what follows the breakpoint in the sample
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
        seq = a[p:E2E_A + 1] + partner[:E2E_CLIP]
        recs.append(dict(qname=f"jn{i}", flag=97, tid=0, pos=p, mapq=60, cigar=f"{m}M{E2E_CLIP}S", mtid=1, mpos=mp, isize=0, seq=seq, qual=qual(len(seq))))
        recs.append(dict(qname=f"jn{i}", flag=145, tid=1, pos=mp, mapq=60, cigar="100M", mtid=0, mpos=p, isize=0, seq=b[mp:mp + 100], qual=qual(100)))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return (a, b), tuple(recs)
