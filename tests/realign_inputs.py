"""Inputs of tests/test_realign_differential_gpu.py: small references of random bases and query sets built for one rule of the re-aligner each.
tests/test_realign_model.py runs the model alone over every set and holds the conditions the GPU comparison needs (no `overflow`, no `tie`
outside the overflow set, the edges really hit), so the seeds below were chosen on the CPU.

Every set is (contigs, queries): contigs are ACGT strings, queries are ASCII strings as ssv_realign_query takes them."""
import functools

import numpy as np

COMP = str.maketrans("ACGTacgt", "TGCAtgca")
JUNK_BYTES = "NnRy-*.XU"


def revcomp(s):
    return s.translate(COMP)[::-1]


def dna(rng, n):
    return "".join("ACGT"[x] for x in rng.randint(0, 4, n))


def other(ch, k=1):
    """another base than ch (k = 1..3)"""
    return "ACGT"[("ACGT".index(ch.upper()) + k) % 4]


def sub(s, positions, rng=None):
    s = list(s)
    for at in positions:
        s[at] = other(s[at], 1 if rng is None else 1 + int(rng.randint(3)))
    return "".join(s)


def unlike(s, rng=None):
    """a sequence of the same length that differs from s in every base: matches nowhere along s's diagonal"""
    return sub(s, range(len(s)), rng)


# Contig lengths: offsets that are no multiples of 4 or 32, a contig shorter than a seed (17) whose neighbours' last 20-mers would run into it,
# contigs of exactly one seed (20) and one base less (19).  SHAPES["even"]: the total is a multiple of 32 and the last contig ends on it (the
# last word is full, the slack word is the one behind it); SHAPES["odd"]: total = 1 mod 32 (one base in the last word).
SHAPES = {"even": [3001, 17, 2229, 2047, 20, 1533, 23, 2600, 19, 1055], "odd": [2047, 3001, 19, 1211, 17, 2229, 20, 1750, 33, 1162]}
assert sum(SHAPES["even"]) % 32 == 0 and sum(SHAPES["odd"]) % 32 == 1


def offsets(contigs):
    off = [0]
    for c in contigs:
        off.append(off[-1] + len(c))
    return off


@functools.lru_cache(maxsize=None)
def shape_reference(shape):
    rng = np.random.RandomState({"even": 101, "odd": 202}[shape])
    return tuple(dna(rng, n) for n in SHAPES[shape])


@functools.lru_cache(maxsize=None)
def random_set(shape):
    """~600 queries: substrings of 20..400 bases on both strands with 0-6 substitutions anywhere (the ends included), lower-case runs, N and other
    bytes, unrelated heads and tails of 1-40 bases; queries over every contig boundary; the lengths at the limits"""
    contigs = shape_reference(shape)
    text, off = "".join(contigs), offsets(contigs)
    rng = np.random.RandomState({"even": 11, "odd": 12}[shape])
    long_ones = [i for i, c in enumerate(contigs) if len(c) >= 400]
    queries = []
    for k in range(520):
        tid = long_ones[int(rng.randint(len(long_ones)))]
        n = int(rng.randint(20, 401))
        p = int(rng.randint(0, len(contigs[tid]) - n + 1))
        s = contigs[tid][p:p + n]
        n_sub = int(rng.randint(0, 7))
        where = set(int(x) for x in rng.randint(0, n, n_sub))
        if k % 7 == 0 and n_sub:
            where |= {0, n - 1}
        s = sub(s, sorted(where), rng)
        if k % 3 == 1:   # lower-case runs
            a = int(rng.randint(0, n))
            b = min(n, a + int(rng.randint(1, 60)))
            s = s[:a] + s[a:b].lower() + s[b:]
        if k % 5 == 2:   # bytes that are no bases
            s = list(s)
            for at in rng.randint(0, n, int(rng.randint(1, 4))):
                s[int(at)] = JUNK_BYTES[int(rng.randint(len(JUNK_BYTES)))]
            s = "".join(s)
        if k % 4 == 3:   # unrelated head and / or tail
            head = dna(rng, int(rng.randint(0, 41)))
            tail = dna(rng, int(rng.randint(1, 41)))
            s = head + s + tail
        queries.append(revcomp(s) if rng.randint(2) else s)
    for b in off[1:-1]:   # over every boundary, unequal parts, both strands
        for left, right in ((37, 52), (61, 24), (25, 25 + 17 + 30), (3, 40), (40, 3)):
            if b - left >= 0 and b + right <= len(text):
                s = text[b - left:b + right]
                queries.append(s)
                queries.append(revcomp(s))
    big = max(range(len(contigs)), key=lambda i: len(contigs[i]))
    for n in (0, 19, 20, 49, 50, 1024, 1025):
        p = int(rng.randint(0, len(contigs[big]) - n + 1))
        queries.append(contigs[big][p:p + n])
        queries.append(revcomp(contigs[big][p:p + n]))
    queries += [dna(rng, 60) for _ in range(20)] + ["N" * 40, "acgt" * 10]
    return contigs, tuple(queries)


@functools.lru_cache(maxsize=None)
def threshold_set(shape):
    """one rule each, both sides of its edge; every query on both strands.  -> (contigs, queries, labels)"""
    contigs = shape_reference(shape)
    rng = np.random.RandomState(31)
    c = contigs[SHAPES[shape].index(2229)]
    q, lab = [], []

    def add(label, s):
        q.extend([s, revcomp(s)])
        lab.extend([label + "/fwd", label + "/rev"])

    def core(n):
        p = int(rng.randint(100, len(c) - n - 100))
        return p, c[p:p + n]
    # the 30-point floor: exact substrings; one mismatch (n - 5); a matching stretch inside unlike flanks
    for n in (29, 30, 31):
        add(f"exact{n}", core(n)[1])
    for n in (34, 35):   # 5 - 4 + (n - 6)
        add(f"mismatch-at-5-of-{n}", sub(core(n)[1], [5]))
    for n in (29, 30):
        p, s = core(n)
        add(f"flanked{n}", unlike(c[p - 10:p]) + s + unlike(c[p + n:p + n + 10]))
    # the end sums: X = mismatch, M = match; the part of the pattern next to the core comes first
    for pat in ("X", "XX", "MX", "XXMMM", "XXMMMM", "XMXMM", "XMXMMM", "XMMMMX", "XMMMMMX"):
        k = len(pat)
        p, s = core(60 + k)
        bad = [i for i, ch in enumerate(pat) if ch == "X"]
        add("tail-" + pat, sub(s, [60 + i for i in bad]))
        add("head-" + pat, sub(s, [k - 1 - i for i in bad]))
    # an end outside the contig: the bases over the edge continue into the neighbour along the same diagonal
    text, off = "".join(contigs), offsets(contigs)
    for t in [i for i, x in enumerate(contigs) if len(x) >= 1000][:4]:
        lo, hi = off[t], off[t + 1]
        for over in (1, 3, 4, 19):
            if hi + over <= len(text):
                add(f"over-end{t}+{over}", text[hi - 45:hi + over])
            if lo - over >= 0:
                add(f"over-start{t}+{over}", text[lo - over:lo + 45])
        add(f"at-end{t}-X", sub(text[hi - 45:hi], [44]))         # the last base of the contig mismatches: -4, extended
        add(f"at-end{t}-XX", sub(text[hi - 45:hi], [43, 44]))    # -8: clipped
    return contigs, tuple(q), tuple(lab)


def _assemble(rng, pieces):
    """pieces: list of contigs, each a list of strings or ints (int = that many random bases)"""
    return tuple("".join(x if isinstance(x, str) else dna(rng, x) for x in ctg) for ctg in pieces)


@functools.lru_cache(maxsize=None)
def two_locus_set():
    """a sequence X present at two loci: copies with 0..3 mismatches (gaps 0, 5, 10, 15), partial copies at a contig's end (gaps 1..9), on the same and
    on the opposite strand, in another contig and in the same; a sequence cut in two by an insertion / a deletion of 4..64 bases (two diagonals of
    one contig and strand, inside and outside the same-locus window).  -> (contigs, queries, labels)"""
    rng = np.random.RandomState(41)
    L = 120
    pieces, q, lab = [], [], []

    def add(label, s):
        q.extend([s, revcomp(s)])
        lab.extend([label + "/fwd", label + "/rev"])
    for m in range(4):
        for opposite in (False, True):
            x = dna(rng, L)
            y = sub(x, [30, 60, 90][:m])
            y = revcomp(y) if opposite else y
            pieces.append([int(rng.randint(50, 90)), x, int(rng.randint(300, 400))])          # other contig
            pieces.append([int(rng.randint(200, 300)), y, int(rng.randint(50, 90))])
            add(f"copy-m{m}-{'opp' if opposite else 'same'}-other-contig", x)
            x2 = dna(rng, L)
            y2 = sub(x2, [25, 70, 100][:m])
            y2 = revcomp(y2) if opposite else y2
            pieces.append([int(rng.randint(50, 90)), x2, int(rng.randint(33, 200)), y2, int(rng.randint(50, 90))])  # same contig
            add(f"copy-m{m}-{'opp' if opposite else 'same'}-same-contig", x2)
    for g in range(1, 10):
        for opposite in (False, True):
            x = dna(rng, L)
            pieces.append([int(rng.randint(50, 90)), x, int(rng.randint(60, 90))])
            if opposite:   # revcomp(x) without its first g bases, at the start of a contig: the copy of x[:L - g] on the other strand
                pieces.append([revcomp(x[:L - g]), int(rng.randint(60, 90))])
            else:
                pieces.append([int(rng.randint(60, 90)), x[:L - g]])
            add(f"partial-gap{g}-{'opp' if opposite else 'same'}", x)
    for delta in (4, 8, 31, 32, 33, 34, 64):
        for a in (64, 70):
            x = dna(rng, L)
            pieces.append([int(rng.randint(50, 90)), x[:a], delta, x[a:], int(rng.randint(50, 90))])   # insertion in the reference
            add(f"ins{delta}-{a}/{L - a}", x)
            x = dna(rng, L + delta)
            pieces.append([int(rng.randint(50, 90)), x[:a], x[a + delta:], int(rng.randint(50, 90))])                    # deletion in the reference
            add(f"del{delta}-{a}/{L - a}", x)
    return _assemble(rng, pieces), tuple(q), tuple(lab)


SWEEP = range(255, 301)


@functools.lru_cache(maxsize=None)
def sweep_set():
    """X forward at locus A (global offset = 0 mod 4) and reverse-complemented at locus B, exact or with one mismatch; queries X[:n] for n = 255..300.
    All strand-0 seeds are found before any strand-1 seed, n = 272..275 gives exactly 64 of them: the two loci are then first seen at candidate
    indices 0 and 64.  -> (contigs, queries, labels)"""
    rng = np.random.RandomState(51)
    x0, x1 = dna(rng, 300), dna(rng, 300)
    contigs = _assemble(rng, [[400, x0, 300, x1, 177], [251, revcomp(x0), 333], [90, revcomp(sub(x1, [150])), 61]])
    q = [x0[:n] for n in SWEEP] + [x1[:n] for n in SWEEP]
    lab = [f"exact-{n}" for n in SWEEP] + [f"one-mismatch-{n}" for n in SWEEP]
    return contigs, tuple(q), tuple(lab)


UNIT, N_UNITS, N_UNITS_2 = 36, 80, 10


@functools.lru_cache(maxsize=None)
def tandem_set():
    """more distinct diagonals than lanes: a tandem array of a 36-base unit x 80 and a second, diverged one (one substitution a unit) x 10 in another
    contig.  The unit is a multiple of the sampling step, so a query 20-mer finds either every copy or none; of the short queries tried here only
    those with at most 192 seeds are kept (counted with the model's seeds(): 2 sampled offsets x 80 copies fit, 3 do not).
    -> (contigs, queries, labels)"""
    import realign_model as M
    rng = np.random.RandomState(61)
    u = dna(rng, UNIT)
    u2 = sub(u, [5])
    a0, b0 = 403, 222
    contigs = _assemble(rng, [[a0, u * N_UNITS, 350], [b0, u2 * N_UNITS_2, 301]])
    a, b = u * N_UNITS, u2 * N_UNITS_2
    q, lab = [], []
    for n in (30, 31, 32, 33):
        for ph in range(UNIT):
            q.append(a[UNIT + ph:UNIT + ph + n]); lab.append(f"first-array-{n}@{ph}")
    for n in (36, 38, 40):
        for ph in range(UNIT):
            q.append(b[UNIT + ph:UNIT + ph + n]); lab.append(f"second-array-{n}@{ph}")
    for flank in (3, 5, 8, 12, 30):   # the array's first bases behind / its last bases in front of unique sequence
        for n in (30, 31, 32, 33):
            q.append(contigs[0][a0 - flank:a0 + n]); lab.append(f"into-array-{flank}+{n}")
            q.append(contigs[0][a0 + UNIT * N_UNITS - n:a0 + UNIT * N_UNITS + flank]); lab.append(f"out-of-array-{n}+{flank}")
    q += [revcomp(s) for s in q]
    lab += [x + "/rev" for x in lab]
    ref = M.Reference(contigs)
    keep = [i for i, s in enumerate(q) if len(M.seeds(ref, s)) <= M.MAX_CAND]
    return contigs, tuple(q[i] for i in keep), tuple(lab[i] for i in keep)


@functools.lru_cache(maxsize=None)
def overflow_set():
    """more than 192 seeds: a 1024-base unique match has 251 on one diagonal and is still exact; long queries out of the tandem array are not"""
    contigs, _, _ = tandem_set()
    rng = np.random.RandomState(71)
    big = dna(rng, 1500)
    contigs = contigs + (big,)
    a0 = 403
    q = [big[100:1124], revcomp(big[8:1032]), sub(big[301:1325], [0, 500, 1023])]
    lab = ["unique-1024", "unique-1024/rev", "unique-1024-3mm"]
    for n in (60, 100, 300):
        q += [contigs[0][a0 + 40:a0 + 40 + n], revcomp(contigs[0][a0 + 77:a0 + 77 + n]), contigs[0][a0 - 50:a0 + n]]
        lab += [f"array-{n}", f"array-{n}/rev", f"into-array-50+{n}"]
    return contigs, tuple(q), tuple(lab)


POLY_A = 6000


@functools.lru_cache(maxsize=None)
def low_complexity_set():
    """a 6 kb poly-A contig among random ones.  -> (contigs, queries, expect): expect[i] = (tid, pos, reverse) for the queries of >= 60 bases cut from
    the random contigs, None for the others (poly-A, the contig's edges)"""
    rng = np.random.RandomState(81)
    contigs = (dna(rng, 3001), "A" * POLY_A, dna(rng, 2530), dna(rng, 777))
    q, expect = [], []
    for k in range(120):
        tid = (0, 2, 3)[k % 3]
        n = int(rng.randint(60, 200))
        p = int(rng.randint(0, len(contigs[tid]) - n + 1))
        s = contigs[tid][p:p + n]
        if k % 4 == 1:
            s = sub(s, [n // 2])
        rev = bool(k & 1)
        q.append(revcomp(s) if rev else s)
        expect.append((tid, p, int(rev)))
    for s in ("A" * 50, "T" * 64, "a" * 20, "A" * 1024, contigs[0][-30:] + "A" * 30, "A" * 25 + contigs[2][:40], revcomp(contigs[0][-40:] + "A" * 40), "A" * 30 + "C" + "A" * 30):
        q.append(s)
        expect.append(None)
    return contigs, tuple(q), tuple(expect)


def poly_a_sampled(contigs):
    """the indexed positions of low_complexity_set's poly-A contig"""
    off = offsets(contigs)
    return sum(1 for p in range(off[1], off[2] - 19) if p % 4 == 0)


N_MANY, MANY_LEN = 66500, 40
MANY_QUERY_CONTIGS = (10, 65535, 65536, 66000)


@functools.lru_cache(maxsize=None)
def many_contigs_set():
    """more contigs than 16 bits count: 66,500 of 40 bases; queries = whole contigs below, at and above 65,536, both strands"""
    rng = np.random.RandomState(91)
    codes = rng.randint(0, 4, N_MANY * MANY_LEN).astype(np.uint8)
    text = np.frombuffer(b"ACGT", np.uint8)[codes].tobytes().decode()
    contigs = tuple(text[i * MANY_LEN:(i + 1) * MANY_LEN] for i in range(N_MANY))
    q = []
    for t in MANY_QUERY_CONTIGS:
        q += [contigs[t], revcomp(contigs[t]), contigs[t][3:38]]
    return contigs, tuple(q)


@functools.lru_cache(maxsize=None)
def cli_set():
    """`seeksv realign` end to end: a mixed-case FASTA of four contigs and ~60 clipped sequences with distinct qualities.
    -> (names, contigs as written (mixed case), [(sequence, quality)])"""
    rng = np.random.RandomState(95)
    contigs = []
    for n in (1203, 37, 990, 1500):
        s = list(dna(rng, n))
        for _ in range(n // 100 + 1):
            a = int(rng.randint(0, n))
            for i in range(a, min(n, a + int(rng.randint(1, 50)))):
                s[i] = s[i].lower()
        contigs.append("".join(s))
    contigs[3] += contigs[0][100:180] + dna(rng, 55)   # a stretch present twice
    names = ["ctgA", "short", "ctgC", "ctgD"]
    seqs = []
    for k in range(52):
        tid = (0, 2, 3)[k % 3]
        n = int(rng.randint(25, 200))
        p = int(rng.randint(0, len(contigs[tid]) - n + 1))
        s = contigs[tid][p:p + n].upper()
        if k % 4 == 1:
            s = sub(s, [int(x) for x in rng.randint(0, n, 2)], rng)
        if k % 4 == 2:
            s = dna(rng, int(rng.randint(1, 30))) + s
        if k % 4 == 3:
            s = s + dna(rng, int(rng.randint(1, 30)))
        if k % 5 == 0:
            s = s[:n // 3] + s[n // 3:n // 2].lower() + s[n // 2:]
        if k % 6 in (1, 4):
            s = s[:5] + "N" + s[6:n // 2] + "r" + s[n // 2 + 1:]
        seqs.append(revcomp(s) if k & 1 else s)
    for k in range(4):   # unrelated head and tail: S, M, S
        core = contigs[2][200 + 100 * k:260 + 100 * k].upper()
        s = dna(rng, 7 + k) + core + dna(rng, 11 + k)
        seqs.append(revcomp(s) if k & 1 else s)
    seqs += [contigs[0][100:180].upper(), revcomp(contigs[0][110:170].upper()), contigs[0][90:180].upper()]
    seqs += [dna(rng, 70), dna(rng, 19), "N" * 30, "acgtn" * 8, contigs[0][-30:].upper() + contigs[1].upper() + contigs[2][:45].upper(), revcomp(contigs[3][-50:].upper()),
             contigs[0][:29].upper(), contigs[0][:30].upper()]
    assert len(set(seqs)) == len(seqs)
    out = [(s, "".join(chr(33 + int(x)) for x in rng.randint(2, 41, len(s)))) for s in seqs]
    return names, tuple(contigs), tuple(out)
