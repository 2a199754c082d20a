"""Named inputs for the read cap of the reference's pileup (libbam 0.1.16, bam_plp_push: at most ~8000 reads alive), one rule each, plus
seeded random ones.  Every case is (contigs, records in file order, junction rows); the junctions come with planted discordant pairs so that
the reference's -B harness reports depths inside and just behind every stack.  What the REAL reference wrote for each case is committed in
tests/golden/pileup_cap/reference.json (tests/golden/make_pileup_cap_reference.py); the tests regenerate the inputs from here.

Only random.Random(seed) is used; nothing depends on hash order."""
import functools
import random

import bamio

# "notid", records with tid == -1 between mapped ones, is not pinned by the reference: libbam's bam_index_build refuses such a file ("reads
# without coordinates prior to reads with coordinates"), so the reference cannot be run on it.  The case is held against the model and the
# oracle only (UNPINNED).
FILTERS = ("dup", "secondary", "qcfail", "mapq", "notid")
RANDOM_POOL = ("100M", "100S", "40S60I", "100=", "50M50S", "10M", "30M10D60M", "40M20N40M")
RANDOM_SEEDS = tuple(range(8))
TILE, CHUNK = 4096, 64    # records per tile / per wavefront chunk of the kernels that replay the cap (getsv_kernels.h)


def ref_span(cigar):
    """bam_calend of libbam 0.1.16: only M, D, N advance the reference"""
    return sum(l for l, op in bamio.parse_cigar(cigar) if op in (0, 2, 3))


class Case:
    def __init__(self, names=("chrA",), lens=(30000,)):
        self.names, self.lens = list(names), list(lens)
        self.recs, self.junctions, self.stacks = [], [], []

    def add(self, tid, pos, cigar="100M", n=1, flag=99, mapq=60, mtid=None, mpos=None, isize=None, tag=None):
        lq = sum(l for l, op in bamio.parse_cigar(cigar) if op in (0, 1, 4, 7, 8))
        r = dict(qname="r", flag=flag, tid=tid, pos=pos, mapq=mapq, cigar=cigar, mtid=tid if mtid is None else mtid,
                 mpos=pos + 200 if mpos is None else mpos, isize=(280 + pos % 41) if isize is None else isize, seq="A" * lq, qual=b"\x1e" * lq)
        if tag is not None:
            r = dict(r, tag=tag)
        for _ in range(n):
            self.recs.append(r)
        return r

    def filtered(self, kind, tid, pos, cigar="100M", tag=None):
        """a record that the depth pass does not take: read_bam's MAPQ cut and BAM_DEF_MASK, or a record without a contig"""
        if kind == "notid":
            r = self.add(-1, -1, cigar, flag=99 | 4, tag=tag)
            r["place"] = (tid, pos)      # (where finish() sorts it)
            return r
        flag = 99 | {"dup": 1024, "secondary": 256, "qcfail": 512, "mapq": 0}[kind]
        return self.add(tid, pos, cigar, flag=flag, mapq=5 if kind == "mapq" else 60, tag=tag)

    def background(self, tid, lo, hi, step=5, n=1):
        for p in range(lo, hi, step):
            self.add(tid, p, n=n)

    def stack(self, tid, pos, n, cigar="100M", junctions=True):
        """n reads at one start, and four junctions inside and just behind the columns they cover"""
        self.add(tid, pos, cigar, n=n)
        self.stacks.append((tid, pos))
        if junctions:
            k = len(self.stacks)
            far = self.lens[tid] - 2500 + 40 * k
            for d in (12, 50, 99, 101):
                self.junction(tid, pos + d, tid, far + d)

    def junction(self, ta, up, tb, down):
        """a junction and four discordant pairs that support it (as tests/golden/make_golden.py:deep_case plants them)"""
        us = "+" if up >= 400 else "-"   # (near a contig's start the supporting reads lie behind the junction)
        self.junctions.append((self.names[ta], up, us, self.names[tb], down, "+"))
        for r in range(4):
            if us == "+":
                pos, mpos, flag = up - 130 - 9 * r, down + 60 + r, 97      # (insert sizes near the background's mean: counted as support)
            else:
                pos, mpos, flag = up + 10 + 7 * r, down + 180 + r, 113
            self.add(ta, pos, flag=flag, mtid=tb, mpos=mpos, isize=0 if ta != tb else mpos - pos)

    def finish(self):
        order = sorted(range(len(self.recs)), key=lambda i: self.recs[i].get("place", (self.recs[i]["tid"], self.recs[i]["pos"])))   # stable: equal starts keep their creation order
        self.recs = [self.recs[i] for i in order]
        self.junctions.sort(key=lambda j: (j[0], j[3], j[2], j[5], j[1], j[4]))   # Junction::operator<
        self.rows = [j + (0,) for j in self.junctions]
        return self

    def first_index(self, tid, pos):
        return next(i for i, r in enumerate(self.recs) if r["tid"] == tid and r["pos"] == pos)


def _plain(n_stack=8100, s=5000):
    c = Case()
    c.background(0, 200, 29000)
    c.stack(0, s, n_stack)
    return c, s


# ---- spanless first reads: a read without any M / D / N operation as the first read at a new start while the cap binds ----

def _j4():
    c, s = _plain()
    c.add(0, s + 1, n=11)
    return c


def _j1(spanless="100S", n_stack=8100):
    c, s = _plain(n_stack)
    c.add(0, s + 1, spanless)
    c.add(0, s + 1, n=10)
    return c


def _j2():
    c, s = _plain()
    c.add(0, s + 2, "30S70I")
    c.add(0, s + 2, "100S")
    c.add(0, s + 2, "90M10S", n=10)
    return c


def _j3():
    c, s = _plain()
    c.add(0, s + 1)
    c.add(0, s + 1, "100S")
    c.add(0, s + 1, n=10)
    return c


def _j5():
    c, s = _plain()
    c.add(0, s + 1, "100S")
    c.add(0, s + 2, n=10)
    return c


def _ten_starts():
    """a spanless first read at ten starts in a row"""
    c, s = _plain()
    for k in range(1, 11):
        c.add(0, s + k, ("100S", "100=", "40S60I")[k % 3])
        c.add(0, s + k, n=3)
    return c


def _origin():
    """the file's first read, at column 0 of the first contig, is spanless: libbam's iterator starts at (tid 0, pos 0), so this one first read
    at a new start has end > iter->pos false and tid > iter->tid false"""
    c = Case()
    c.add(0, 0, "100S")
    c.stack(0, 0, 8100, junctions=False)
    c.add(0, 1, n=10)
    c.background(0, 5, 29000)
    for d in (12, 50, 99, 101):
        c.junction(0, d, 0, 27000 + d)
    return c


# ---- other spanless shapes ----

def _new_contig():
    """a spanless read is the first read of a contig whose first start is deep (kept: tid > iter->tid)"""
    c = Case(("chrA", "chrB"), (12000, 30000))
    c.background(0, 200, 11000)
    c.add(1, 100, "100S")
    c.stack(1, 100, 8100)
    c.add(1, 101, n=10)
    c.background(1, 105, 29000)
    return c


def _inside():
    """spanless reads inside a full stack, none of them first at its start"""
    c = Case()
    c.background(0, 200, 29000)
    s = 5000
    for k in range(8100):
        c.add(0, s, "100S" if k in (100, 4000, 7960, 7975, 7990, 8050) else "100M")
    c.stacks.append((0, s))
    for d in (12, 50, 99, 101):
        c.junction(0, s + d, 0, 27600 + d)
    c.add(0, s + 1, n=10)
    return c


def _group64():
    """130 reads at one start, one of them spanless, across a 64-record chunk of the sweep, while the cap fills up"""
    c, s = _plain(7900)
    c.add(0, s + 1, n=70)
    c.add(0, s + 1, "100S")
    c.add(0, s + 1, n=59)
    c.add(0, s + 2, n=5)
    return c


# ---- fill levels ----

def _fill(target):
    """the stack fills the pileup to exactly `target` live reads before the next start"""
    c = Case()
    c.background(0, 200, 29000)
    s = 5000
    for d in (12, 50, 99, 101):
        c.junction(0, s + d, 0, 27600 + d)
    alive = sum(1 for r in c.recs if r["pos"] <= s and r["pos"] + ref_span(r["cigar"]) >= s)
    c.stack(0, s, target - alive, junctions=False)
    c.add(0, s + 1, n=20)
    c.add(0, s + 2, n=20)
    return c


def _ends_at_start():
    """reads whose end equals the next start stay alive there; reads that end one column earlier do not"""
    c, s = _plain(7000)
    c.add(0, s + 50, "50M", n=600)
    c.add(0, s + 50, "49M", n=600)
    c.add(0, s + 100, n=500)
    return c


def _jump():
    """more than 8192 columns without a passing read right behind a stack, then a second stack: the ring is cleared inside a running sweep"""
    c = Case()
    c.background(0, 200, 5000)
    c.stack(0, 5000, 8100)
    c.add(0, 5001, n=10)
    for p in range(5200, 14000, 400):   # filtered reads in the gap: not seen by the pileup
        c.filtered("dup", 0, p)
    c.stack(0, 14300, 8100)
    c.add(0, 14301, n=10)
    c.background(0, 14305, 29000)
    return c


# ---- ring placement ----

def _ring_first():
    """a read with a 20 kb N, alive across the stack, among the file's first records: the ring of ends is larger than 8192 columns from the start"""
    c, s = _plain()
    c.add(0, 1000, "50M20000N50M", tag="long")
    c.add(0, s + 1, n=10)
    return c


def _ring_later():
    """the same read after a first stack, alive across a second one that begins where the first one's reads end"""
    c, s = _plain()
    c.add(0, s + 3, "50M20000N50M", tag="long")
    c.stack(0, s + 101, 8100)
    c.add(0, s + 102, n=10)
    return c


# ---- filtered reads ----

def _filtered(kind):
    """records of one filtered kind as the first record at a start, of a 64-record chunk and of a 4096-record tile"""
    c = Case()
    c.background(0, 200, 29000)
    s = 5000
    for d in (12, 50, 99, 101):
        c.junction(0, s + d, 0, 27600 + d)
    i = sum(1 for r in c.recs if r["pos"] < s) + 2        # the place in the file of the stack's first record: behind the two records below
    c.filtered(kind, 0, s, tag="first_at_start")         # (moved in front of the background's read at s below)
    n = 0
    while n < 8100:
        if i % TILE == 0 or (i % CHUNK == 0 and 7000 <= n < 7400):
            c.filtered(kind, 0, s, tag="tile" if i % TILE == 0 else "chunk")
        else:
            c.add(0, s)
            n += 1
        i += 1
    c.stacks.append((0, s))
    for k in (1, 2, 3, 4, 6):   # (not s + 5: the background has a read there)
        c.filtered(kind, 0, s + k, "100S" if k % 2 else "100M", tag="first_at_start")
        c.add(0, s + k, n=3)
    c = c.finish()
    # the background's read at s was created before the filtered one: put the filtered one in front of it
    i = next(i for i, r in enumerate(c.recs) if r.get("place", (r["tid"], r["pos"])) == (0, s))
    assert "tag" not in c.recs[i] and c.recs[i + 1].get("tag") == "first_at_start"
    c.recs[i], c.recs[i + 1] = c.recs[i + 1], c.recs[i]
    return c


# ---- sweep life cycle ----

def _two_stacks(pad, filler):
    """two stacks with `filler` records between them (and `pad` extra records in front, to place the first stack in its tile)"""
    c = Case()
    c.background(0, 200, 3000)
    c.add(0, 3000, n=pad)
    c.stack(0, 5000, 8100)
    per = -(-filler // 8000)
    left = filler
    for p in range(5200, 13200):
        k = min(per, left)
        if k:
            c.add(0, p, n=k)
        left -= k
    c.stack(0, 14000, 8100)
    c.add(0, 14001, n=10)
    c.background(0, 14005, 29000)
    return c


def _contig_change():
    """a stack on the last start of one contig and on start 0 of the next"""
    c = Case(("chrA", "chrB"), (12000, 30000))
    c.background(0, 200, 11900)
    c.add(0, 11900, n=8100)
    c.stacks.append((0, 11900))
    for d in (12, 50, 99):
        c.junction(0, 11900 + d, 1, 27000 + d)
    c.add(1, 0, "100S")
    c.add(1, 0, n=8100)
    c.stacks.append((1, 0))
    c.add(1, 1, n=10)
    c.background(1, 5, 29000)
    for d in (12, 50, 99, 101):
        c.junction(1, d, 1, 27300 + d)
    return c


def _random(seed):
    """7900 reads at one start, then 60 starts of 1-5 reads each with mixed CIGARs, filter flags and MAPQs"""
    rng = random.Random(seed)
    c, s = _plain(7900)
    c.add(0, s - 3, n=70)      # (with the background the pileup is nearly full behind the stack: the cap binds within the first few starts)
    p = s
    for _ in range(60):
        p += rng.choice((1, 1, 1, 2, 3))
        for _ in range(rng.randint(1, 5)):
            r = rng.random()
            flag = 99 | (1024 if r < 0.06 else 0) | (256 if 0.06 <= r < 0.10 else 0) | (512 if 0.10 <= r < 0.13 else 0)
            c.add(0, p, rng.choice(RANDOM_POOL), flag=flag, mapq=rng.choice((60, 60, 60, 60, 30, 20, 19, 0)))
    return c


# name -> (builder, kind); kind: "control" (the cap never binds), "spanless_first" (the rule of the first read at a start decides), "" otherwise
BUILDERS = {
    "J4_control": (_j4, ""),
    "J1_spanless_first": (_j1, "spanless_first"),
    "J2_two_spanless_first": (_j2, "spanless_first"),
    "EQ_spanless_first": (lambda: _j1("100="), "spanless_first"),
    "J3_spanless_second": (_j3, ""),
    "J5_spanless_alone": (_j5, ""),
    "J6_stack_3000": (lambda: _j1(n_stack=3000), "control"),
    "ten_spanless_firsts": (_ten_starts, "spanless_first"),
    "spanless_at_origin": (_origin, ""),
    "spanless_first_on_new_contig": (_new_contig, "spanless_first"),
    "spanless_inside_stack": (_inside, ""),
    "spanless_in_group_of_130": (_group64, ""),
    "fill_7997": (lambda: _fill(7997), ""),
    "fill_7998": (lambda: _fill(7998), ""),
    "fill_7999": (lambda: _fill(7999), ""),
    "ends_at_start": (_ends_at_start, ""),
    "jump_in_sweep": (_jump, ""),
    "ring_global_first_batch": (_ring_first, ""),
    "ring_regrow_later_batch": (_ring_later, ""),
    "two_stacks_three_tiles": (lambda: _two_stacks(*TWO_STACKS["three_tiles"]), ""),
    "two_stacks_new_sweep": (lambda: _two_stacks(*TWO_STACKS["new_sweep"]), ""),
    "contig_change": (_contig_change, "spanless_first"),
}
BUILDERS.update({"filtered_" + k: ((lambda k=k: _filtered(k)), "") for k in FILTERS})
BUILDERS.update({f"random_{s}": ((lambda s=s: _random(s)), "") for s in RANDOM_SEEDS})
# (extra records in front, records between the stacks): the tile of the first stack's last deep record and of the second stack's first one
# are three apart / six apart (tests/test_pileup_cap_inputs.py checks it)
TWO_STACKS = {"three_tiles": (0, 4000), "new_sweep": (0, 17000)}
UNPINNED = ("filtered_notid",)
CASES = tuple(k for k in BUILDERS if k not in UNPINNED)      # the cases the reference pins (tests/golden/pileup_cap/reference.json)
ALL_CASES = CASES + UNPINNED
KIND = {k: v[1] for k, v in BUILDERS.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name][0]()
    return c if hasattr(c, "rows") else c.finish()


def write_bam(path, c):
    """the case as a BAM file (records that are equal are encoded once)"""
    enc = {}
    out = []
    for r in c.recs:
        b = enc.get(id(r))
        if b is None:
            b = enc[id(r)] = bamio.encode_record({k: v for k, v in r.items() if k not in ("tag", "place")})
        out.append(b)
    bamio.write_bam(path, c.names, c.lens, out)
