"""Hand-made record sets for the duplicate-marking rule of `seeksv run -D` (include/seeksv_hip.h, ssv_pairdup_mark), each with the answer written beside it:
`dup` lists the records (by index in the set's coordinate order) that the rule marks, worked out by hand from the rule's text, not by running
tests/pairdup_model.py.  The model is held to these (tests/test_pairdup_inputs.py), the kernels to the model (tests/test_pairdup_gpu.py).  `claim` states what
a set is about; tests/test_pairdup_inputs.py asserts it.  One rule applies per set.

Records are dicts as tests/bamio.py's encode_record takes them.  `records` is the set in coordinate order; orders(s) gives it in four orders."""
import random
import re

from markdup_inputs import in_order, sam_text  # noqa: F401  (sam_text: the records as SAM lines, for the decoders)

TARGETS = ["c0", "c1", "c2", "c3"]
TARGET_LENS = [100000] * 4
BIG_TARGETS = [f"c{k}" for k in range(70000)]     # contig ids up to 69,999 (beyond 16 bits)


def qlen(cigar):
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X")


def read(qname, flag, tid, pos, cigar, mtid, mpos, q=30):
    """one record; q: one quality for every base, or the quality bytes, or None (0xff)"""
    n = qlen(cigar) if cigar else 20
    qual = bytes([q] * n) if isinstance(q, int) else q
    return dict(qname=qname, flag=flag, tid=tid, pos=pos, mapq=60, cigar=cigar or "", mtid=mtid, mpos=mpos, isize=0, seq=("ACGT" * ((n + 3) // 4))[:n], qual=qual)


def pair(qname, a, b, q=30, q2=None):
    """(read 1, read 2) of one pair; a, b = (tid, pos, cigar, reverse) of read 1 and read 2, mate fields and flags as an aligner writes them"""
    (t1, p1, c1, r1), (t2, p2, c2, r2) = a, b
    f1 = 0x1 | 0x40 | (0x10 if r1 else 0) | (0x20 if r2 else 0)
    f2 = 0x1 | 0x80 | (0x10 if r2 else 0) | (0x20 if r1 else 0)
    return read(qname, f1, t1, p1, c1, t2, p2, q), read(qname, f2, t2, p2, c2, t1, p1, q if q2 is None else q2)


FWD100 = (0, 100, "20M", False)       # u = 100
REV300 = (0, 300, "20M", True)        # u = 319

SETS = []


def add(name, records, dup, targets=TARGETS, **claim):
    """records: in any order; dup: indices into that list.  Stored in coordinate order, dup with it."""
    recs, at = in_order(records)
    SETS.append(dict(name=name, records=recs, dup=sorted(at[i] for i in dup), targets=targets, claim=claim))


# ---- the two clipping forms: 20M at 100 and 5S15M at 105 are one 5' end.  -M's rule (aligned positions) finds nothing ----
_k, _d = pair("k", FWD100, REV300), pair("d", (0, 105, "5S15M", False), REV300, q=20)
add("clip_forms", [_k[0], _k[1], _d[0], _d[1]], [2, 3], markdup_misses=True)

# ---- reverse-strand ends: the trailing run of S / H is added, D and N lie inside the span, I does not.  Every copy's read 2 ends at 319 ----
_copies = [("t", "15M5S", 30), ("h", "13M4S3H", 29), ("dd", "10M2D8M", 28), ("n", "5M10N5M", 27), ("i", "10M3I10M", 26)]
_recs = list(pair("k", FWD100, REV300, q=40))
for _name, _cig, _q in _copies:
    _recs += list(pair(_name, FWD100, (0, 300, _cig, True), q=_q))
add("reverse_ends", _recs, list(range(2, 12)), u_b=319, cigars=[c for _, c, _ in _copies])

# ---- seven operations, two more than a record line holds: the leading run on a forward read, the trailing run on a reverse read ----
_k, _d = pair("k", FWD100, REV300), pair("d", (0, 105, "2H3S5M1I5M1D4M", False), (0, 300, "4M1D5M1I5M3S2H", True), q=20)
add("cigar7", [_k[0], _k[1], _d[0], _d[1]], [2, 3], n_cigar=7, u=(100, 319))

# ---- u < 0: 5S15M at 2 and 3S17M at 0 both start at -3 ----
_k, _d = pair("k", (0, 2, "5S15M", False), (0, 200, "20M", True)), pair("d", (0, 0, "3S17M", False), (0, 200, "20M", True), q=20)
add("u_negative", [_k[0], _k[1], _d[0], _d[1]], [2, 3], u_a=-3)

# ---- each of the six key fields differing alone: base and copy are one group, the variant is not in it.  base key = (1, 100, 0, 2, 319, 1) ----
_A, _B = (1, 100, "20M", False), (2, 300, "20M", True)
_VARIANTS = [("tid_a", 0, (0, 100, "20M", False), _B), ("u_a", 1, (1, 101, "20M", False), _B), ("rev_a", 2, (1, 81, "20M", True), _B),
             ("tid_b", 3, _A, (3, 300, "20M", True)), ("u_b", 4, _A, (2, 301, "20M", True)), ("rev_b", 5, _A, (2, 319, "20M", False))]
for _field, _at, _va, _vb in _VARIANTS:
    add(f"key_{_field}", list(pair("base", _A, _B)) + list(pair("copy", _A, _B, q=20)) + list(pair("var", _va, _vb, q=20)), [2, 3], differs_in=_at)

# ---- a pair that wins on the sum but loses on read 1: x = 800 + 300, y = 600 + 600.  y stays (-M's rule, the head alone, would keep x) ----
_x, _y = pair("x", FWD100, REV300, q=40, q2=15), pair("y", FWD100, REV300, q=30)
add("sum_not_read1", [_x[0], _y[0], _x[1], _y[1]], [0, 2], read1=(800, 600), sums=(1100, 1200))

# ---- equal scores: the pair whose smaller g is smallest stays (the one set whose answer depends on the order) ----
_p = [pair(f"p{k}", FWD100, REV300) for k in range(3)]
add("equal_scores", [_p[0][0], _p[1][0], _p[2][0], _p[0][1], _p[1][1], _p[2][1]], [1, 2, 4, 5], ties=True)

# ---- a mate that arrives with 0x400: it keeps the flag and takes no part, so its mate is a name group of one.  e, a real copy, is marked ----
_k, _d, _e = pair("k", FWD100, REV300), pair("d", FWD100, REV300, q=20), pair("e", FWD100, REV300, q=16)
_d[1]["flag"] |= 0x400
add("preset_0x400", [_k[0], _d[0], _e[0], _k[1], _d[1], _e[1]], [2, 5], preset=[4], alone=[1])

# ---- name groups of one record: l's mate is not in the input.  l scores highest and takes no part in the group ----
_k, _d = pair("k", FWD100, REV300), pair("d", FWD100, REV300, q=20)
add("group_of_one", [_k[0], pair("l", FWD100, REV300, q=40)[0], _d[0], _k[1], _d[1]], [2, 4], unpaired=1)

# ---- name groups of three records: t's read 2 comes twice.  t would be a copy of k; it is left alone ----
_k, _t = pair("k", FWD100, REV300), pair("t", FWD100, REV300, q=20)
add("group_of_three", [_k[0], _t[0], _k[1], _t[1], dict(_t[1])], [], unpaired=3)

# ---- name groups of two first-of-pair records ----
_k, _f = pair("k", FWD100, REV300), pair("f", FWD100, REV300, q=20)
_f[1]["flag"] = (_f[1]["flag"] & ~0x80) | 0x40
add("two_first_of_pair", [_k[0], _f[0], _k[1], _f[1]], [], unpaired=2)

# ---- mates whose mate fields disagree: m's read 2 names another mate position; s's read 1 says its mate is forward ----
_k, _m, _s = pair("k", FWD100, REV300), pair("m", FWD100, REV300, q=20), pair("s", FWD100, REV300, q=20)
_m[1]["mpos"] = 101
_s[0]["flag"] &= ~0x20
add("mate_fields_disagree", [_k[0], _m[0], _s[0], _k[1], _m[1], _s[1]], [], unpaired=4)

# ---- mates on two contigs ----
_k, _d = pair("k", (0, 100, "20M", False), (2, 300, "20M", True)), pair("d", (0, 100, "20M", False), (2, 300, "20M", True), q=20)
add("two_contigs", [_k[0], _k[1], _d[0], _d[1]], [2, 3], contigs=(0, 2))

# ---- contig ids up to 69,999: 69998 = 0x1116e and 4462 = 0x116e differ in bit 16 alone ----
_k = pair("k", (69998, 100, "20M", False), (69999, 300, "20M", True))
_d = pair("d", (69998, 100, "20M", False), (69999, 300, "20M", True), q=20)
_v = pair("v", (4462, 100, "20M", False), (69999, 300, "20M", True), q=20)
add("contig_ids", [_k[0], _k[1], _d[0], _d[1], _v[0], _v[1]], [2, 3], targets=BIG_TARGETS, max_tid=69999)

# ---- unmapped and unplaced records in between (in coordinate order the unplaced ones come last; in the other orders they lie between the mates) ----
_k, _d = pair("k", FWD100, REV300), pair("d", FWD100, REV300, q=20)
_half = [read("h", 0x1 | 0x8 | 0x40, 0, 100, "20M", 0, 100, 40), read("h", 0x1 | 0x4 | 0x80, 0, 100, None, 0, 100, 40)]
_un = [read("z", 0x4d, -1, -1, None, -1, -1), read("z", 0x8d, -1, -1, None, -1, -1), read("y", 0x4d, -1, -1, None, -1, -1), read("y", 0x8d, -1, -1, None, -1, -1)]
add("unmapped_between", [_k[0], _half[0], _half[1], _d[0], _un[0], _k[1], _un[1], _d[1], _un[2], _un[3]], [3, 7], no_part=6)


# ---- groups of n pairs with one key, all scores distinct: pair k scores 1200 + (11 k mod n) (11 is coprime to every n here), the best stays ----
def _group(n):
    recs, best = [], None
    for k in range(n):
        v = (11 * k) % n
        a, b = v % 21, v // 21
        r1, r2 = pair(f"r{k}", FWD100, REV300)
        r1["qual"] = bytes([31] * a + [30] * (20 - a))
        r2["qual"] = bytes([51] * b + [30] * (20 - b))
        recs.append((r1, r2))
        if v == n - 1:
            best = k
    order = [p[0] for p in recs] + [p[1] for p in recs]
    add(f"group_{n}", order, [k for k in range(n) if k != best] + [n + k for k in range(n) if k != best], pairs=n, best=best)


for _n in (2, 63, 64, 65, 130):
    _group(_n)

# ---- 300 pairs with distinct keys: nothing is marked; with the name hash cut to 4 bits or to 1 bit the names collide and no name group is a pair ----
_recs = []
for _k in range(300):
    _recs += list(pair(f"q{_k}", (0, 1000 + 3 * _k, "20M", False), (0, 5000 + 3 * _k, "20M", True)))
add("collide_300", _recs, [], pairs=300)

BY_NAME = {s["name"]: s for s in SETS}
SMALL = [s for s in SETS if len(s["records"]) <= 12]


def orders(s, seed=20):
    """the set in four orders -> [(order name, records, where: where[i] = the index in s["records"] of the record at i)]"""
    recs = s["records"]
    n = len(recs)
    by_name = sorted(range(n), key=lambda i: recs[i]["qname"])
    shuffled = list(range(n))
    random.Random(seed).shuffle(shuffled)
    out = []
    for name, where in (("coordinate", list(range(n))), ("read_name", by_name), ("reversed", list(range(n - 1, -1, -1))), ("shuffle", shuffled)):
        out.append((name, [recs[i] for i in where], where))
    return out
