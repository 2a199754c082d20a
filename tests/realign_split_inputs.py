"""Inputs of tests/test_realign_split_gpu.py: references of a few kilobases built AROUND reads of two loci, and query sets built for one rule of the
two-piece split alignments each.  tests/test_realign_split_inputs.py runs the model alone over every set and holds each set to the
property it was built for; a set that misses its property is changed here, not excused there.

A read is drawn first; the reference then gets, for every piece [b, e) of it (the READ's coordinates) on a strand, the piece's bases between FLANK
bases on either side that differ from the read's in every base: no segment runs on by chance, a piece's q_beg / q_end are the planted ones.
Every set is (queries, labels) on reference() unless it says otherwise; where(label) is the global position of a planted piece's first base."""
import functools

import numpy as np

from realign_inputs import dna, other, revcomp, sub, unlike

CAP = 500        # the sorted index's cap for every set but flags_set
FLAGS_CAP = 3
FLANK = 8
NAMES = tuple(f"s{i}" for i in range(8))


def planted(read, b, e, st, mm=()):
    """(left flank, bases, right flank) of the reference text that holds the read's bases [b, e) on strand st; mm: read positions whose base the
    reference's copy does not share"""
    n = len(read)
    s = sub(read, mm)
    if st:
        s, b, e = revcomp(s), n - e, n - b
    r = revcomp(read) if st else read
    return unlike(r[max(b - FLANK, 0):b]), s[b:e], unlike(r[e:e + FLANK])


# name -> (read length, [(label, b, e, strand, contig, mismatching read positions)]): the hand-worked cases of tests/test_realign_split_model.py
CASES = {
    "ff": (100, [("A", 0, 60, 0, 0, ()), ("B", 60, 100, 0, 1, ())]),
    "fr": (100, [("A", 0, 60, 0, 0, ()), ("B", 60, 100, 1, 1, ())]),
    "rf": (100, [("A", 0, 60, 1, 0, ()), ("B", 60, 100, 0, 1, ())]),
    "rr": (100, [("A", 0, 60, 1, 0, ()), ("B", 60, 100, 1, 1, ())]),
    "overlap5": (100, [("A", 0, 60, 0, 0, ()), ("B", 55, 100, 0, 2, ())]),
    "gap10": (100, [("A", 0, 55, 0, 1, ()), ("B", 65, 100, 0, 2, ())]),
    "contained": (100, [("A", 0, 100, 0, 2, ()), ("B", 30, 70, 0, 3, ())]),
    "own20": (100, [("A", 0, 70, 0, 0, ()), ("B", 40, 90, 0, 3, ())]),
    "own19": (100, [("A", 0, 70, 0, 0, ()), ("B", 40, 89, 0, 3, ())]),
    "own20-tie": (100, [("A", 0, 60, 0, 1, ()), ("B", 20, 80, 0, 4, ())]),
    "own19-tie": (100, [("A", 0, 60, 0, 1, ()), ("B", 19, 79, 0, 4, ())]),
    "score30": (100, [("A", 0, 60, 0, 2, ()), ("B", 65, 100, 0, 4, (96,))]),   # 31 bases, a mismatch, 3 bases: cheaper to take than to clip: 34 - 4
    "score29": (100, [("A", 0, 60, 0, 2, ()), ("B", 66, 100, 0, 4, (96,))]),   # 30 bases, a mismatch, 3 bases: a scored candidate at 29
    "comp20": (100, [("A", 0, 60, 0, 0, ()), ("B", 62, 100, 0, 3, ()), ("K", 52, 82, 0, 4, ())]),
    "comp19": (100, [("A", 0, 60, 0, 0, ()), ("B", 62, 100, 0, 3, ()), ("K", 51, 81, 0, 4, ())]),
    "mapq5050": (100, [("A", 0, 50, 0, 1, ()), ("B", 50, 100, 0, 4, ())]),
    "p-twocopy": (100, [("A", 0, 60, 0, 0, ()), ("A2", 0, 60, 0, 3, ()), ("B", 60, 100, 0, 5, ())]),
    "m-twocopy": (100, [("A", 0, 60, 0, 2, ()), ("B2", 60, 100, 1, 1, ()), ("B", 60, 100, 0, 5, ())]),   # the reverse copy lies first; the forward one is the mate
    # reads of 40 (one piece: two would score 20 each), 64, 65, 250 and 1024 bases (400 | 324 bases of nothing | 300: 167 seeds, fewer than slots)
    "len40": (40, [("A", 0, 40, 0, 5, ())]),
    "len40-34": (40, [("A", 0, 34, 0, 5, ())]),
    "len64": (64, [("A", 0, 33, 0, 5, ()), ("B", 33, 64, 1, 3, ())]),
    "len65": (65, [("A", 0, 33, 1, 5, ()), ("B", 33, 65, 0, 4, ())]),
    "len250": (250, [("A", 0, 150, 0, 5, ()), ("B", 150, 250, 1, 6, ())]),
    "len1024": (1024, [("A", 0, 400, 1, 6, ()), ("B", 724, 1024, 0, 6, ())]),
    # the flags set (sorted index, cap FLAGS_CAP): 500 + 400 bases have 217 seeds; 60 bases whose first 30 stand at five places, + 40
    "overflow": (900, [("A", 0, 500, 0, 7, ()), ("B", 500, 900, 0, 7, ())]),
    "masked": (100, [("A", 0, 60, 0, 7, ()), ("h0", 0, 30, 0, 7, ()), ("h1", 0, 30, 0, 7, ()), ("h2", 0, 30, 0, 7, ()), ("h3", 0, 30, 0, 7, ()), ("B", 60, 100, 0, 6, ())]),
}
DEL20 = 20   # "del20": 60 bases, 20 reference bases that the read lacks, 40 bases, on one contig: two diagonals 20 apart, inside the locus window


@functools.lru_cache(maxsize=None)
def _built():
    rng = np.random.RandomState(2401)
    reads = {name: dna(rng, n) for name, (n, _) in CASES.items()}
    reads["del20"] = dna(rng, 100)
    per = [[] for _ in NAMES]   # per contig: strings and (label, string)
    for name, (_, loci) in CASES.items():
        for label, b, e, st, ctg, mm in loci:
            left, body, right = planted(reads[name], b, e, st, mm)
            per[ctg] += [dna(rng, int(rng.randint(41, 97))), left, (f"{name}:{label}", body), right]
    r = reads["del20"]
    per[3] += [dna(rng, 77), unlike(r[:0]), ("del20:A", r[:60]), unlike(r[60:68]) + dna(rng, DEL20 - 2 * FLANK) + unlike(r[52:60]), ("del20:B", r[60:]), dna(rng, 5)]
    contigs, at, base = [], {}, 0
    for pieces in per:
        s = ""
        for p in pieces + [dna(rng, int(rng.randint(50, 90)))]:
            if isinstance(p, tuple):
                if p[0].startswith("masked:") and not p[0].endswith(":B"):   # the five copies at one offset mod 4 (they begin the read: no flank in front): one 20-mer, five indexed positions
                    s += dna(rng, -(base + len(s)) % 4)
                at[p[0]] = base + len(s)
                p = p[1]
            s += p
        contigs.append(s)
        base += len(s)
    return tuple(contigs), at, reads


def reference():
    return _built()[0]


def where(label):
    return _built()[1][label]


def read(name):
    return _built()[2][name]


def offsets():
    off = [0]
    for c in reference():
        off.append(off[-1] + len(c))
    return off


def _both(names):
    q, lab = [], []
    for name in names:
        q += [read(name), revcomp(read(name))]
        lab += [name + "/fwd", name + "/rev"]
    return tuple(q), tuple(lab)


GEOMETRY = ("ff", "fr", "rf", "rr", "overlap5", "gap10", "contained", "del20")
BOUNDARIES = ("own20", "own19", "own20-tie", "own19-tie", "score30", "score29", "comp20", "comp19")
MAPQ = ("mapq5050", "p-twocopy", "m-twocopy")
LENGTHS = ("len40", "len40-34", "len64", "len65", "len250", "len1024")
FLAGS = ("overflow", "masked")


def geometry_set():
    return _both(GEOMETRY)


def boundary_set():
    return _both(BOUNDARIES)


def mapq_set():
    return _both(MAPQ)


def length_set():
    return _both(LENGTHS)


def flags_set():
    """the sorted index with the cap FLAGS_CAP: SSV_RA_F_OVERFLOW (217 seeds; the mate is among the 192 that are followed) and SSV_RA_F_MASKED (the
    20-mers of the first 30 bases stand at five places and give no seed) on a primary that has a mate"""
    return _both(FLAGS)


SWEEP_1, SWEEP_2 = range(266, 282), range(522, 538)


@functools.lru_cache(maxsize=None)
def sweep_set():
    """the mate one and two rounds behind the winner, in the winner's lane: X[:n] forward (X at a global offset = 0 mod 4) + one other base + 50 bases that stand
    reverse-complemented in another contig.  Every strand-0 seed is found before any strand-1 seed and lies on X's diagonal: n = 272..275 gives
    exactly 64 of them and n = 528..531 exactly 128, the mate's first seed then takes candidate slot 64 / 128: lane 0, like slot 0.
    -> (contigs, queries, labels)"""
    rng = np.random.RandomState(2402)
    x, y = dna(rng, 540), dna(rng, 50)
    contigs = (dna(rng, 400) + x + dna(rng, 120), dna(rng, 151) + revcomp(y) + dna(rng, 99))
    q = [x[:n] + other(x[n]) + y for n in list(SWEEP_1) + list(SWEEP_2)]   # (one base that is not X's next: no seed runs over X[:n]'s end)
    return contigs, tuple(q), tuple(f"sweep-{n}+1+50" for n in list(SWEEP_1) + list(SWEEP_2))


UNIT, N_UNITS = 36, 90


@functools.lru_cache(maxsize=None)
def tandem_set():
    """more than 64 candidate diagonals: 36 unique bases + 30 bases out of a tandem array of a 36-base unit x 90 (a multiple of the sampling step: a
    20-mer finds every copy or none; of the 30 bases' 11 it is 2 or 3, by the phase).  The array's copies are 90 candidates 36 apart, one locus each; the mate is the one with the smallest diagonal that
    holds all of the bases, its MAPQ 0 (the other copies compete for its bases), and the primary's 60 (the plain call's: 30 or 36): no copy shares a base of the read with it.  Kept: the queries with at most 192 seeds, i.e. the phases with 2.
    -> (contigs, queries, labels)"""
    import realign_model as M
    rng = np.random.RandomState(2403)
    u, a = dna(rng, UNIT), dna(rng, 36)
    arr = u * N_UNITS
    contigs = (dna(rng, 301) + arr + dna(rng, 222), dna(rng, 133) + a + dna(rng, 90))
    q, lab = [], []
    for n in (30,):
        for ph in range(UNIT):
            t = arr[UNIT + ph:UNIT + ph + n]
            q += [a + t, t + a, revcomp(a + t)]
            lab += [f"unique+array-{n}@{ph}", f"array-{n}@{ph}+unique", f"unique+array-{n}@{ph}/rev"]
    ref = M.Reference(contigs)
    keep = [i for i, s in enumerate(q) if len(M.seeds(ref, s)) <= M.MAX_CAND]
    return contigs, tuple(q[i] for i in keep), tuple(lab[i] for i in keep)


N_MIX = 2003   # no multiple of the four wavefronts of a workgroup


@functools.lru_cache(maxsize=None)
def mix_set():
    """about 2000 queries where split reads (two stretches of two places of the reference, and the planted reads), unsplit ones (one stretch with 0-2
    substitutions), random sequence, 19 and 1025 bases take turns: early returns beside live wavefronts in one workgroup"""
    rng = np.random.RandomState(2404)
    ref = reference()
    plain = [c for i, c in enumerate(ref) if i != 7]   # (not the contig with the five copies of 30 bases)
    cases = [s for fn in (geometry_set, boundary_set, mapq_set) for s in fn()[0]]

    def stretch(n):
        text = plain[int(rng.randint(len(plain)))]
        p = int(rng.randint(0, len(text) - n))
        s = text[p:p + n]
        return s if rng.randint(2) else revcomp(s)
    q, lab = [], []
    for i in range(N_MIX):
        kind = i % 5
        if kind == 0:
            q.append(stretch(int(rng.randint(30, 80))) + stretch(int(rng.randint(30, 80)))); lab.append(f"mix{i}-split")
        elif kind == 1:
            n = int(rng.randint(35, 110))
            x = stretch(n)
            q.append(sub(x, sorted(set(int(v) for v in rng.randint(0, n, int(rng.randint(3))))), rng)); lab.append(f"mix{i}-unsplit")
        elif kind == 2:
            q.append(cases[int(rng.randint(len(cases)))] if i % 2 else dna(rng, int(rng.randint(30, 90)))); lab.append(f"mix{i}-" + ("planted" if i % 2 else "random"))
        elif kind == 3:
            q.append(stretch(19) if i % 2 else "".join(ref)[i:i + 1025]); lab.append(f"mix{i}-len{19 if i % 2 else 1025}")
        else:
            q.append(stretch(int(rng.randint(20, 45))) + dna(rng, int(rng.randint(0, 12))) + stretch(int(rng.randint(30, 60)))); lab.append(f"mix{i}-split-gap")
    assert len(q) == N_MIX and N_MIX % 4
    return tuple(q), tuple(lab)


SETS = dict(geometry=geometry_set, boundary=boundary_set, mapq=mapq_set, length=length_set)


@functools.lru_cache(maxsize=None)
def all_queries():
    """every set of SETS, one after the other, then the mix -> (queries, labels with the set's name in front); all on reference(), either index"""
    q, lab = [], []
    for name, fn in list(SETS.items()) + [("mix", mix_set)]:
        a, b = fn()
        q.extend(a)
        lab.extend(f"{name}:{x}" for x in b)
    return tuple(q), tuple(lab)


@functools.lru_cache(maxsize=None)
def cli_set():
    """`seeksv realign -P`: the queries of SETS and the first 150 of the mix -> [(name line behind '@', sequence, quality)]; names with "/1", "/2" and
    with a comment behind white space, which is not part of the name"""
    rng = np.random.RandomState(2405)
    out = []
    for i, s in enumerate([x for fn in SETS.values() for x in fn()[0]] + list(mix_set()[0][:150])):
        if not s:
            continue
        name = f"read{i}/{1 + i % 2}"
        out.append((name + ("" if i % 3 else " 1:N:0 x") + ("\tmore" if i % 7 == 0 else ""), s, "".join(chr(33 + int(x)) for x in rng.randint(2, 41, len(s)))))
    return tuple(out)


def cli_name(line):
    return line.split()[0]


# ---- end to end through getsv -F: reads that cross an inter-contig junction and were left unmapped ----
E2E_NAMES, E2E_LENS = ("tA", "tB"), (2003, 2102)
E2E_A = 1000          # 0-based: the last base of tA before the breakpoint
E2E_B = 900           # the first base of tB behind it
E2E_READS = 10
E2E_SV_OPTS = []      # getsv's defaults


@functools.lru_cache(maxsize=None)
def e2e_sample():
    """-> (contigs, records for bamio.write_bam, coordinate-sorted).  Background: proper pairs of 100-base reads over both contigs, none clipped.  The
    junction: ten pairs whose first read lies on tA in front of the breakpoint, and whose second read - 35 + 3 i bases of tA up to E2E_A, then tB from
    E2E_B on, every other one reverse-complemented - the first aligner left unmapped (flag 4 at its mate's place, as aligners write it).  No read is
    soft-clipped there: without the unmapped reads nothing in the file knows of the junction.  The split points differ from read to read."""
    rng = np.random.RandomState(2406)
    a, b = dna(rng, E2E_LENS[0]), dna(rng, E2E_LENS[1])
    recs = []
    qual = lambda n: "".join(chr(33 + 30 + int(x)) for x in rng.randint(0, 10, n))  # noqa: E731
    for tid, c in enumerate((a, b)):
        for i, p in enumerate(range(5, len(c) - 320, 13)):
            name = f"bg{tid}_{i}"
            recs.append(dict(qname=name, flag=99, tid=tid, pos=p, mapq=60, cigar="100M", mtid=tid, mpos=p + 200, isize=300, seq=c[p:p + 100], qual=qual(100)))
            recs.append(dict(qname=name, flag=147, tid=tid, pos=p + 200, mapq=60, cigar="100M", mtid=tid, mpos=p, isize=-300, seq=c[p + 200:p + 300], qual=qual(100)))
    for i in range(E2E_READS):
        m = 35 + 3 * i
        p = E2E_A - 260 - 7 * i
        seq = a[E2E_A + 1 - m:E2E_A + 1] + b[E2E_B:E2E_B + 100 - m]
        recs.append(dict(qname=f"jn{i}", flag=73, tid=0, pos=p, mapq=60, cigar="100M", mtid=0, mpos=p, isize=0, seq=a[p:p + 100], qual=qual(100)))
        recs.append(dict(qname=f"jn{i}", flag=133, tid=0, pos=p, mapq=0, cigar="", mtid=0, mpos=p, isize=0, seq=revcomp(seq) if i % 2 else seq, qual=qual(100)))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))   # (stable: a pair's mapped read stays in front of its unmapped one)
    return (a, b), tuple(recs)


def e2e_names_both_ends(text):
    """does a line of `text` name both ends of the planted junction: tA at E2E_A + 1 and tB at E2E_B + 1 (1-based)?"""
    x, y = ("tA", str(E2E_A + 1)), ("tB", str(E2E_B + 1))
    for line in text.splitlines():
        f = line.split("\t")
        pairs = set(zip(f, f[1:]))
        if x in pairs and y in pairs:
            return True
    return False
