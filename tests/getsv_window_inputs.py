"""Designed geometry for the fused getsv pass (ssv_getsv_begin / _scan / _finish, seeksv_amd/csrc/getsv_kernels.h): junction windows, depth windows,
query ranges and query points made BY HAND - plain structured arrays, no host.Plan - at the sizes and places where the kernels change path.  The
planner only ever produces a breakpoint +- a flank, junction windows of one width, and queries inside windows; the C ABI takes anything sorted,
disjoint and non-empty.  tests/test_getsv_window_inputs.py (CPU) holds every family to the edge it is for and pins the oracle's answer with a second
plain model; tests/test_getsv_windows_gpu.py compares the device with the oracle.

Every family returns (names, lens, batch, junctions, windows, ranges, points, mean, sd); case(name) builds it once.  Columns are 1-based and
inclusive (windows, ranges, points), record positions and junction windows 0-based with an exclusive end, as in the ABI."""
import functools

import numpy as np

from seeksv_amd import _abi

# the constants the sizes below are derived from (tests/test_getsv_window_inputs.py holds them against the headers)
TILE = 512            # genome tile of the tile map: 1 << TILE_SHIFT
WAVE = 64             # probes per round of window_at_or_before
PREFIX_ROUND = 256    # columns per round of k_depth_prefix: 4 x WAVE
GC_COLS = 4096        # columns a dense workgroup's difference array covers
GC_WC = 16            # depth windows a dense workgroup keeps in LDS
GC_JC = 32            # junction windows it keeps in LDS
GC_DENSE_MIN = 128    # candidates from which on a scan tile is k_getsv_cand_dense's
CS_TILE = 4096        # records per scan tile

MEAN, SD = 300, 40    # insert-size statistics every family states: pairs count with an insert of 140 .. 460
OPS = "MIDNSHP=X"
FLAGS = (99, 147, 83, 163, 97, 145, 65, 129, 113, 177, 73, 89, 133, 69)
MAPQS = (0, 1, 5, 19, 20, 30, 60, 60, 60)
F_DEPTH_MASK = 4 | 256 | 512 | 1024
KIND_CDF = np.cumsum([0.62, 0.1, 0.1, 0.06, 0.05, 0.04, 0.03])[:-1]

DESIGNED = {}         # case name -> indices of the junctions that were given pairs of their own (each must count at least one)


# ---------------------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------------------
class Rows:
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.rows = []      # (tid, pos, ops, flag, mapq, mtid, mpos, isize)

    @staticmethod
    def cigar(room, long_n, u):
        """the CIGAR mix of dense_sample (tests/test_random_differential_gpu.py) - M, S, D, short and long N, I, more than five operations, H, = - cut to
        the `room` the contig leaves behind the start: a read's last column never lies beyond its contig.  u: five numbers in [0, 1)"""
        pick = lambda seq, x: seq[int(x * len(seq))]
        fits = [l for l in (50, 100, 150) if l + 70 <= room]
        if not fits:
            return [(int(room), "M")]           # ends on the contig's last column
        L = pick(fits, u[0])
        k = int(np.searchsorted(KIND_CDF, u[1], side="right"))
        a = 1 + int(u[2] * (L - 2))
        if k == 1: return [(a, "S"), (L - a, "M")] if u[3] < 0.5 else [(a, "M"), (L - a, "S")]
        if k == 2: return [(a, "M"), (1 + int(u[3] * 59), "D"), (L - a, "M")]
        if k == 3: return [(a, "M"), (pick([n for n in long_n if L + n <= room] or [5], u[3]), "N"), (L - a, "M")]
        if k == 4 and L - a > 1: return [(a, "M"), (1, "I"), (L - a - 1, "M")]
        if k == 5:
            q = L // 8
            return [(q, "M"), (1, "I"), (q, "M"), (3, "D"), (q, "M"), (2, "I"), (q, "=" if u[3] < 0.3 else "M"), (7, "D"), (L - 4 * q - 3, "M")]
        if k == 6: return [(3, "H"), (L, "M")] if u[3] < 0.5 else [(L, "M"), (2, "H")]
        return [(L, "M")]

    def background(self, tid, positions, length, mate_tids, long_n=(5, 300, 3000, 9000)):
        """reads of every kind at the given starts: every flag bit the passes look at, every MAPQ on either side of -q, mates near and on other contigs"""
        n = len(positions)
        u = self.rng.rand(n, 14).tolist()       # (drawn at once: a draw per record and field was most of the time the CPU test took)
        for pos, x in zip(positions.tolist(), u):
            ops = self.cigar(length - pos, long_n, x)
            flag = FLAGS[int(x[5] * len(FLAGS))]
            for bit, pr, y in ((256, 0.03, x[6]), (512, 0.03, x[7]), (1024, 0.06, x[8]), (2048, 0.03, x[9])):
                if y < pr: flag |= bit
            mtid = tid if x[10] < 0.8 else mate_tids[int(x[10] * 1e6) % len(mate_tids)]
            mpos = max(0, pos + int(x[11] * 1400) - 700)
            d = 240 + int(x[12] * 1e6) % 120
            isz = (0, mpos - pos, d, -d)[int(x[12] * 4)]
            self.rows.append((tid, pos, ops, flag, MAPQS[int(x[13] * len(MAPQS))], mtid, mpos, isz))

    def uniform(self, tid, lo, hi, n, length, mate_tids, **kw):
        """n background reads with starts uniform in [lo, hi] (kept on the contig, 30 bases at least)"""
        lo, hi = max(0, int(lo)), min(int(hi), length - 30)
        self.background(tid, np.sort(self.rng.randint(lo, hi + 1, int(n))), length, mate_tids, **kw)

    def pairs(self, j, n=3):
        """n reads that count for junction j (a row of JUNCTION_DTYPE): 100M, MAPQ 60, on j's up contig inside its window, the mate where the strand
        combination wants it (getsv.cpp:1074-1113; with MEAN / SD the insert must come out in 140 .. 460)"""
        rng = self.rng
        up, down, beg, end = int(j["up_pos"]), int(j["down_pos"]), int(j["beg"]), int(j["end"])
        us, ds = chr(j["up_strand"]), chr(j["down_strand"])
        for _ in range(n):
            if us == "+":
                a = int(rng.randint(0, min(100, up - beg - 1) + 1))   # calend = up - a > beg
                pos = up - 100 - a
            else:
                a = int(rng.randint(0, min(100, end - up - 1) + 1))   # pos = up + a < end
                pos = up + a
            assert pos >= 0 and pos < end and pos + 100 > beg
            if (us, ds) == ("+", "+"): flag, mpos = 97, down + int(rng.randint(0, 101))            # insert 201 + a + b
            elif (us, ds) == ("-", "+"): flag, mpos = 113, down + int(rng.randint(40, 151))        # insert 103 + a + b
            else: flag, mpos = 65, down - 100 - int(rng.randint(40, 151))                          # insert 101 + a + b
            assert mpos >= 0
            self.rows.append((int(j["up_tid"]), pos, [(100, "M")], flag, 60, int(j["down_tid"]), mpos, 0))

    def one_long_skip(self, tid, pos, skip=9000):
        """the one read whose reference span is far beyond every other's: the part of the stream that holds it states a longer max_ref_span, and the
        tile map is built again while records are streaming"""
        self.rows.append((tid, int(pos), [(60, "M"), (skip, "N"), (40, "M")], 99, 60, tid, int(pos) + 200, 0))

    def sorted_rows(self):
        order = sorted(range(len(self.rows)), key=lambda i: (self.rows[i][0], self.rows[i][1]))
        return [self.rows[i] for i in order]


def to_batch(rows):
    """rows (in the order given) -> a host batch as the tests pass them to _abi.make_batch; max_ref_span as a reader would state it"""
    n = len(rows)
    cig, coff = [], []
    for r in rows:
        coff.append(len(cig))
        cig += [(l << 4) | OPS.index(op) for l, op in r[2]]
    col = lambda k, dt: np.array([r[k] for r in rows], dt)
    b = dict(tid=col(0, np.int32), pos=col(1, np.int32), flag=col(3, np.uint16), mapq=col(4, np.uint8), n_cigar=np.array([len(r[2]) for r in rows], np.uint16),
             l_qseq=np.array([sum(l for l, op in r[2] if op in "MIS=X") for r in rows], np.int32), mtid=col(5, np.int32), mpos=col(6, np.int32), isize=col(7, np.int32),
             xc=np.zeros(n, np.uint8), cigar=np.array(cig, np.uint32), cigar_off=np.array(coff, np.uint32), seq_off=np.full(n, 0xFFFFFFFFFFFFFFFF, np.uint64),
             seqqual=np.zeros(16, np.uint8))
    b["max_ref_span"] = int(ref_spans(b).max()) if n else 1
    return b


def _per_record(b, ops):
    """sum of the lengths of the CIGAR operations in `ops` per record"""
    n = len(b["tid"])
    nc = b["n_cigar"].astype(np.int64)
    assert np.array_equal(b["cigar_off"].astype(np.int64), np.cumsum(nc) - nc)      # operations lie in record order, no holes
    rec = np.repeat(np.arange(n), nc)
    keep = np.isin(b["cigar"] & 15, [OPS.index(o) for o in ops])
    out = np.zeros(n, np.int64)
    np.add.at(out, rec[keep], (b["cigar"][keep] >> 4).astype(np.int64))
    return out


def ref_spans(b):
    """what max_ref_span bounds (include/seeksv_hip.h): M, D, N, =, X"""
    return _per_record(b, "MDN=X")


def calends(b):
    """bam_calend of libbam 0.1.16 (exclusive, 0-based): only M, D, N advance; no CIGAR: pos + 1"""
    return np.where(b["n_cigar"] == 0, b["pos"].astype(np.int64) + 1, b["pos"].astype(np.int64) + _per_record(b, "MDN"))


def deal_between_filler(R, rows, filler_tid, filler_len, mate_tids, piece=100, filler=3990):
    """The rows' contig comes back: pieces of `piece` records between pieces of `filler` records on a contig without any window (positions inside a
    piece stay in order, as in the odd seeds of dense_sample).  piece < GC_DENSE_MIN and CS_TILE - filler < GC_DENSE_MIN: whichever way the stream is cut
    into batches, no scan tile holds GC_DENSE_MIN candidates - k_getsv_cand (one thread per record) meets the geometry, never k_getsv_cand_dense."""
    assert max(piece, CS_TILE - filler) < GC_DENSE_MIN and CS_TILE - filler <= 2 * piece   # any 4096 records in a row: a piece, or what a whole filler piece leaves
    out = []
    for k in range(0, len(rows), piece):
        out += rows[k:k + piece]
        F = Rows(int(R.rng.randint(1 << 30)))
        F.uniform(filler_tid, 0, filler_len, filler, filler_len, mate_tids, long_n=(5, 300))
        out += F.sorted_rows()
    return out


def junction(up_tid, up_pos, us, down_tid, down_pos, ds, beg, end):
    j = np.zeros(1, _abi.JUNCTION_DTYPE)[0]
    j["up_tid"], j["up_pos"], j["up_strand"], j["down_tid"], j["down_pos"], j["down_strand"], j["beg"], j["end"] = up_tid, up_pos, ord(us), down_tid, down_pos, ord(ds), beg, end
    return j


def intervals(rows):
    a = np.zeros(len(rows), _abi.INTERVAL_DTYPE)
    for k, (t, b, e) in enumerate(rows):
        a[k] = (t, b, e)
    return a


def junctions(rows):
    a = np.zeros(len(rows), _abi.JUNCTION_DTYPE)
    for k, j in enumerate(rows):
        a[k] = j
    return a


STRANDS = (("+", "+"), ("-", "+"), ("+", "-"))   # the three combinations FindDiscordantReadPairs counts ("-", "-" never)


def three_junctions(R, tid, length, lo, hi, width=700):
    """one junction per live strand combination with its up side in [lo, hi] of contig tid and pairs of its own, for families that are about depth windows"""
    js = []
    for k, (us, ds) in enumerate(STRANDS):
        up = lo + (k + 1) * (hi - lo) // 4
        j = junction(tid, up, us, tid, up + 2000 + 300 * k if up + 2600 + 200 < length else max(300, up - 2000 - 300 * k), ds, max(0, up - width // 2), up + width // 2)
        R.pairs(j, 4)
        js.append(j)
    return js


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------
def window_counts(n_win, seed=1):
    """window_at_or_before (k_range_sum) and the binary search of k_point_depth: 64 probes a round - n_win <= 64 one round, <= 64 * 65 = 4160 two, more
    three (never run before); on every side of both edges, and of 64 * 64.  Windows of 1 .. 3 columns with gaps of 0 or 1 column between them ([x, x], [x + 1, x + 1]
    is legal: end < next.beg): also k_depth_prefix on windows of one column, tile_win's start-of-walk value and depth_segment's walk over hundreds of
    windows in one genome tile, and a dense workgroup with far more than GC_WC windows in its range.  Ranges: every window, whole; points: every
    window's first and last column."""
    R = Rows(100 + seed * 7 + n_win)
    rng = R.rng
    wins, col = [], 700
    for _ in range(n_win):
        l = int(rng.randint(1, 4))
        wins.append((0, col, col + l - 1))
        col += l + int(rng.randint(0, 2))
    first, last = wins[0][1], wins[-1][2]
    hi = max(last + 100, first + 3000)
    length = hi + 1000
    n = int(min(20000, max(4300, (hi - first + 300) * 1.5)))
    R.uniform(0, first - 300, hi, n, length, [0], long_n=(5, 300, 3000))
    js = three_junctions(R, 0, length, first, hi)
    ranges = list(wins)
    points = [(0, c, c) for _, b, e in wins for c in sorted({b, e})]
    DESIGNED[f"window_counts_{n_win}"] = list(range(3))
    return ["w"], [length], to_batch(R.sorted_rows()), junctions(js), intervals(wins), intervals(ranges), intervals(points), MEAN, SD


WINDOW_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)


def window_lengths(seed=2):
    """k_depth_prefix: one wavefront per window, rounds of 4 x 64 = 256 columns with a carry from scan to scan and from round to round - a window of
    one column, one short of / exactly / one beyond a wavefront, a round, two rounds and four rounds plus one column.  Each length once from a genome
    tile's first column on and once across a tile boundary (k_tile_mark_windows: t0 .. t1 of one, two and three tiles).  Ranges: the single columns at
    both ends and the whole window (k_range_sum's lane loop of 1, 64, 65 ... columns)."""
    R = Rows(200 + seed)
    wins, t = [], 2
    for l in WINDOW_LENGTHS:
        beg = t * TILE + 1                               # a tile's first column
        wins.append((0, beg, beg + l - 1))
        t = (beg + l - 1) // TILE + 2
        beg = t * TILE + (TILE if l == 1 else TILE + 1 - (l + 1) // 2)   # l == 1: a tile's last column; else the boundary lies inside
        wins.append((0, beg, beg + l - 1))
        t = (beg + l - 1) // TILE + 2
    length = t * TILE + 700
    R.uniform(0, 0, length, 30000, length, [0])
    js = three_junctions(R, 0, length, 3000, length - 4000)
    ranges = sorted(set(r for _, b, e in wins for r in ((0, b, b), (0, e, e), (0, b, e))), key=lambda r: (r[1], r[2]))
    points = [(0, c, c) for _, b, e in wins for c in sorted({b, (b + e) // 2, e})]
    DESIGNED["window_lengths"] = list(range(3))
    return ["w"], [length], to_batch(R.sorted_rows()), junctions(js), intervals(wins), intervals(ranges), intervals(points), MEAN, SD


LONG_LEN = 20000


def long_window(variant, seed=3):
    """k_getsv_cand_dense, the write-out of a workgroup's columns: ONE window [1, len] over a whole 20,000-bp contig.  `dense`: ~200-fold, every
    scan tile holds nothing but candidates, and all but the first and the last workgroup's 4096 columns lie strictly inside the window - wb < C0 (the
    window's first column gets nothing here) and we > C0 + GC_COLS - 1 (no closing slot).  `sparse`: the same contig at ~5-fold, its records dealt
    between pieces of a contig without windows so that no scan tile is dense: the per-record path (k_getsv_cand, depth_segment) meets the same window.
    `seam`: ~90-fold - every scan tile still dense, but its 4096 records start over a little MORE than 4096 columns, so reads cover the last columns of
    a workgroup's range (the clamp at C0 + GC_COLS - 1 then carries depth; at 200-fold a tile's reads end half way) and the ones across its end go the
    per-read way.  `one_long`: dense, no skip beyond 300 but for ONE read with a 9000N behind the middle (the tile map is built again when its part arrives).
    k_depth_prefix: 79 rounds with a carry.  Ranges and points on the columns 0, 1 and 4095 (mod 4096) from the window's first."""
    R = Rows(300 + seed + len(variant))
    names, lens = ["whole", "filler"], [LONG_LEN, 300000]
    long_n = (5, 300) if variant == "one_long" else (5, 300, 3000, 9000)
    if variant == "sparse":
        R.uniform(0, 0, LONG_LEN, 800, LONG_LEN, [0, 1], long_n=long_n)
    else:
        R.uniform(0, 0, LONG_LEN, 18000 if variant == "seam" else 39000, LONG_LEN, [0, 1], long_n=long_n)
    if variant == "one_long":
        R.one_long_skip(0, 10800, 9000)
    js = three_junctions(R, 0, LONG_LEN, 4000, 16000)
    rows = R.sorted_rows()
    if variant == "sparse":
        rows = deal_between_filler(R, rows, 1, lens[1], [0, 1])
    seams = sorted(set(1 + o for k in range(0, LONG_LEN // GC_COLS + 1) for o in (k * GC_COLS - 1, k * GC_COLS, k * GC_COLS + 1) if 0 <= o < LONG_LEN) | {LONG_LEN})
    ranges = [(0, c, c) for c in seams] + [(0, a, b) for a, b in zip(seams, seams[1:])] + [(0, 1, LONG_LEN)]
    ranges.sort(key=lambda r: (r[1], r[2]))
    points = [(0, c, c) for c in seams]
    DESIGNED[f"long_window_{variant}"] = list(range(3))
    return names, lens, to_batch(rows), junctions(js), intervals([(0, 1, LONG_LEN)]), intervals(ranges), intervals(points), MEAN, SD


def contig_edges(seed=4):
    """k_tile_mark_windows / k_tile_mark_junctions at a contig's ends: a window from column 1 (beg - span < 0), windows that end on the contig's last
    column (the last genome tile) and 1000 columns beyond it (t1 >= ntile), a contig of length 0 between two used ones (one tile, no base), a contig
    of exactly 4 x 512 bases and one of a base more (the last read covers the first column of a tile of its own), a window and a junction on contigs
    the header does not have (tid >= n_targets: nothing is marked, queries there give 0), a junction without a down contig (down_tid = -1: reads
    without a mate contig, mtid = -1, must not count for it)."""
    R = Rows(400 + seed)
    names, lens = ["first", "empty", "mult512", "mult512p1"], [3000, 0, 4 * TILE, 4 * TILE + 1]
    R.uniform(0, 0, lens[0], 1600, lens[0], [0, 2, 3], long_n=(5, 300))
    R.uniform(2, 0, lens[2], 1500, lens[2], [0, 2, 3], long_n=(5, 300))
    R.uniform(3, 0, lens[3], 1500, lens[3], [0, 2, 3], long_n=(5, 300))
    for t in (0, 2, 3):                                   # reads that end exactly on the contig's last column, one of a single base on it
        for l in (1, 30, 100):
            R.rows.append((t, lens[t] - l, [(l, "M")], 99, 60, t, max(0, lens[t] - 400), 0))
    wins = [(0, 1, 300), (0, 2700, 3000), (2, 1500, lens[2] + 1000), (3, 1, 1), (3, 1800, lens[3]), (4, 100, 200), (7, 1, 50)]
    js = [junction(0, 40, "-", 2, 900, "+", 10, 400),                 # beg - span < 0
          junction(0, 2950, "+", 3, 500, "-", 2600, 3000),            # ends with its contig
          junction(2, 1900, "+", 0, 1500, "-", 1700, lens[2] + 1000), # ends beyond it
          junction(3, 2000, "+", -1, 700, "+", 1800, 2049),           # no down contig
          junction(5, 500, "+", 0, 700, "+", 300, 900),               # an up contig the header does not have
          junction(3, 300, "-", 3, 1500, "+", 0, 600)]
    for k in (0, 1, 2, 5):
        R.pairs(js[k], 4)
    R.pairs(js[3], 4)                                     # (mtid = -1 like the junction's down_tid: never counted, getsv.cpp:1074)
    ranges = [(0, 1, 1), (0, 1, 300), (0, 2700, 3000), (0, 3000, 3000), (2, 1500, lens[2]), (2, 1500, lens[2] + 1000), (2, lens[2], lens[2] + 1), (3, 1, 1),
              (3, 1800, lens[3]), (3, lens[3], lens[3]), (4, 100, 200), (7, 1, 50)]
    points = [(0, 1, 1), (0, 2, 2), (0, 300, 300), (0, 2700, 2700), (0, 2999, 2999), (0, 3000, 3000), (2, 1500, 1500), (2, lens[2] - 1, lens[2] - 1), (2, lens[2], lens[2]),
              (2, lens[2] + 1, lens[2] + 1), (2, lens[2] + 1000, lens[2] + 1000), (3, 1, 1), (3, 1800, 1800), (3, lens[3] - 1, lens[3] - 1), (3, lens[3], lens[3]), (4, 150, 150), (7, 50, 50)]
    DESIGNED["contig_edges"] = [0, 1, 2, 5]
    return names, lens, to_batch(R.sorted_rows()), junctions(js), intervals(wins), intervals(ranges), intervals(points), MEAN, SD


MIXED_LEN = 130000
MIXED_STRETCH = 20000     # first column of the 4096-column stretch that holds more than GC_JC junction windows


def mixed_junction_widths(variant, seed=5):
    """tile_junc's start-of-walk value, discordant_walk and k_dense_tiles' jlo: "the first junction that begins after tile start - junc_wmax" is only a
    lower bound.  One junction window of 100,000 bp begins before 60 windows of 50 .. 700 bp: 42 of them in one stretch of 4096 columns (more than
    the GC_JC a dense workgroup keeps in LDS: the rest is read from global memory; nested ones among them), 10 elsewhere under the long one, 8 behind
    its end.  junc_wmax is 100,000, so every walk under the long window starts at junction 0 and passes whatever lies between; every junction has
    pairs of its own, all three strand combinations.  Depth: 40 windows of ONE column inside one genome tile (tile_win, depth_segment's walk, more than
    GC_WC in a dense workgroup's range) and a few ordinary ones.  `dense`: 30,000 records around the stretch (k_getsv_cand_dense); `spread`: 3,300
    records over the whole contig in order (dense workgroups whose records lie further apart than their nine genome tiles); `sparse`: those dealt between
    a contig without windows (k_getsv_cand); `one_long`: dense, with ONE 9000N read behind the first third."""
    R = Rows(500 + seed + len(variant))
    rng = R.rng
    names, lens = ["mixed", "filler"], [MIXED_LEN, 300000]
    specs = [(1000, 101000)]
    S = MIXED_STRETCH
    for k in range(42):
        if k % 6 == 5:                                     # nested in the one before: the same middle, a third of its width
            b, e = specs[-1]
            specs.append((b + (e - b) // 3, e - (e - b) // 3))
        else:
            w = int(rng.randint(150 if k % 6 == 4 else 50, 701))
            b = int(rng.randint(S, S + GC_COLS - w))
            specs.append((b, b + w))
    for k in range(10):
        w = int(rng.randint(50, 701)); b = int(rng.randint(30000, 99000)); specs.append((b, b + w))
    for k in range(8):
        w = int(rng.randint(50, 701)); b = int(rng.randint(101000, 125000)); specs.append((b, b + w) if k else (100800, 101300))   # (the first: across the long one's end)
    js = []
    for k, (b, e) in enumerate(specs):
        us, ds = STRANDS[k % 3]
        up = (b + e) // 2 if k else S + 2000              # (the long one: 21,000 bp behind its window's start, in the stretch - a walk that starts later misses it)
        js.append(junction(0, up, us, 0 if k % 4 else 1, 110000 + 37 * k if k % 4 else 5000 + 100 * k, ds, b, e))
    one_col = [(0, S + TILE * 4 + 10 + 2 * k, S + TILE * 4 + 10 + 2 * k) for k in range(40)]          # one genome tile: 22058 .. 22136
    wins = [(0, 2500, 3400), (0, S - 400, S + 300)] + one_col + [(0, S + 3000, S + 5000), (0, 60000, 60300), (0, 100900, 101100), (0, 124000, 124500)]
    wins.sort()
    long_n = (5, 300) if variant == "one_long" else (5, 300, 3000, 9000)
    if variant in ("dense", "one_long"):
        R.uniform(0, S - 1500, S + GC_COLS + 1500, 30000, MIXED_LEN, [0, 1], long_n=long_n)
        R.uniform(0, 0, MIXED_LEN, 3000, MIXED_LEN, [0, 1], long_n=long_n)
    else:
        few = variant == "sparse"                          # (dealt between filler records: 40,000 records in all)
        R.uniform(0, 0, MIXED_LEN, 450 if few else 2500, MIXED_LEN, [0, 1], long_n=long_n)
        R.uniform(0, S - 500, S + GC_COLS + 500, 250 if few else 600, MIXED_LEN, [0, 1], long_n=long_n)
    if variant == "one_long":
        R.one_long_skip(0, S + 2500, 9000)
    for j in js:
        R.pairs(j, 3)
    rows = R.sorted_rows()
    if variant == "sparse":
        rows = deal_between_filler(R, rows, 1, lens[1], [0, 1])
    ranges = [(0, b, e) for _, b, e in wins] + [(0, S + 3000, S + 3000), (0, S + 4095, S + 4097)]
    ranges.sort(key=lambda r: (r[1], r[2]))
    points = [(0, c, c) for _, b, e in wins for c in sorted({b, (b + e) // 2, e})]
    DESIGNED[f"mixed_junction_widths_{variant}"] = list(range(len(js)))
    return names, lens, to_batch(rows), junctions(js), intervals(wins), intervals(ranges), intervals(points), MEAN, SD


def outside_queries(seed=6):
    """k_point_depth and k_range_sum asked about places without a window: a point before the first window of the first contig (lo == 0), in a gap of one
    column between two windows, one column behind a window, on a contig that has records but no window, on contigs the header does not have; ranges
    that end exactly on their window's last column, start exactly on its first, hold one column, and reach past their window's end into a gap where no
    other window lies (only the part inside counts - on both sides).  No range reaches a second window: the ABI excludes that."""
    R = Rows(600 + seed)
    names, lens = ["gaps", "nowindow", "last"], [6000, 5000, 4000]
    for t in range(3):
        R.uniform(t, 0, lens[t], 1700, lens[t], [0, 1, 2], long_n=(5, 300))
    wins = [(0, 500, 700), (0, 702, 900), (0, 2000, 2100), (2, 100, 400)]
    js = three_junctions(R, 1, lens[1], 500, 4000)       # on the contig without depth windows
    ranges = [(0, 500, 700), (0, 650, 700), (0, 690, 701), (0, 702, 750), (0, 702, 702), (0, 880, 1500), (0, 900, 901), (0, 2050, 2050), (0, 2050, 2300), (0, 2100, 5999),
              (2, 100, 100), (2, 400, 400), (2, 399, 4000)]
    points = {(t, c) for t, b, e in wins for c in (b - 1, b, (b + e) // 2, e, e + 1)} | {(0, 1), (0, 10), (1, 1), (1, 1000), (3, 50), (9, 300)}
    points = [(t, c, c) for t, c in sorted(points)]
    DESIGNED["outside_queries"] = list(range(3))
    return names, lens, to_batch(R.sorted_rows()), junctions(js), intervals(wins), intervals(ranges), intervals(points), MEAN, SD


GENOME_CONTIGS = 3366
GENOME_BIG = 1700         # the contig of 2^29 - 1 bases


def genome_scale(seed=7):
    """Coordinates: ctg_tile_off[tid] + (pos >> 9) with 3,366 contigs and more than two million genome tiles, col + len - 1 and (int)(t << 9) + 1 just
    below 2^29.  A header like a full hg38 index: contig 0 of 248,956,422 bases, one contig of 2^29 - 1 (the last position a BAM index addresses), the
    rest short, every 97th of length 0.  Records, depth windows and junction windows in the last 6,000 bases of contig 0, of the 2^29 - 1 contig and of
    the last contig - the last window of each ends on the contig's last column - and junctions between the three."""
    R = Rows(700 + seed)
    rng = R.rng
    lens = [int(x) for x in rng.randint(1000, 200000, GENOME_CONTIGS)]
    for t in range(5, GENOME_CONTIGS - 1, 97):
        lens[t] = 0
    lens[0], lens[GENOME_BIG], lens[-1] = 248956422, (1 << 29) - 1, 50000
    names = [f"g{t}" for t in range(GENOME_CONTIGS)]
    used = (0, GENOME_BIG, GENOME_CONTIGS - 1)
    wins, js = [], []
    for k, t in enumerate(used):
        L = lens[t]
        R.uniform(t, L - 6000, L, 4500, L, list(used), long_n=(5, 300, 3000))
        for l in (1, 100):
            R.rows.append((t, L - l, [(l, "M")], 99, 60, t, L - 500, 0))
        wins += [(t, L - 5800, L - 5300), (t, L - 4000, L - 3999), (t, L - 3997, L - 2500), (t, L - 600, L)]
        o = used[(k + 1) % 3]
        for m, (us, ds) in enumerate(STRANDS):
            up = L - 5000 + 1500 * m
            js.append(junction(t, up, us, o, lens[o] - 3000 - 500 * m, ds, up - 300 - 100 * m, up + 350))
    for j in js:
        R.pairs(j, 3)
    ranges = [(t, b, e) for t, b, e in wins] + [(t, e, e) for t, b, e in wins]
    ranges.sort()
    points = [(t, c, c) for t, b, e in wins for c in sorted({b, (b + e) // 2, e})]
    DESIGNED["genome_scale"] = list(range(len(js)))
    return names, lens, to_batch(R.sorted_rows()), junctions(js), intervals(wins), intervals(ranges), intervals(points), MEAN, SD


def nothing_to_do(what, seed=8):
    """n_windows = 0 with junctions (no depth pass: no cap flag, k_depth_prefix never launched, every query answers 0), n_junctions = 0 with windows, and
    neither (no tile is marked, no record staged): what comes back is the oracle's, zeros where nothing was asked - max_depth too."""
    R = Rows(800 + seed)
    names, lens = ["n0", "n1"], [9000, 7000]
    R.uniform(0, 0, lens[0], 2600, lens[0], [0, 1], long_n=(5, 300, 3000))
    R.uniform(1, 0, lens[1], 1900, lens[1], [0, 1], long_n=(5, 300, 3000))
    js = three_junctions(R, 0, lens[0], 1000, 6000)
    wins = [(0, 1000, 1400), (0, 5000, 5600), (1, 1, 700)]
    ranges = [(0, 1000, 1400), (0, 5100, 5100), (1, 1, 700)]
    points = [(0, 1000, 1000), (0, 1200, 1200), (0, 5600, 5600), (1, 1, 1), (1, 350, 350)]
    if what in ("no_windows", "neither"): wins = []
    if what in ("no_junctions", "neither"): js = []
    DESIGNED[f"nothing_to_do_{what}"] = list(range(len(js)))
    return names, lens, to_batch(R.sorted_rows()), junctions(js), intervals(wins), intervals(ranges), intervals(points), MEAN, SD


# window_at_or_before: a round of WAVE probes `step` apart leaves step - 1 windows, so one round settles WAVE windows, two settle WAVE * (WAVE + 1) = 4160,
# and the third runs from 4161 on - not from WAVE * WAVE + 1 (tests/test_getsv_window_inputs.py replays the loop); both pairs of edges are cases
SEARCH_TWO_ROUNDS = WAVE * (WAVE + 1)
WINDOW_COUNTS = (1, WAVE - 1, WAVE, WAVE + 1, WAVE * WAVE - 1, WAVE * WAVE, WAVE * WAVE + 1, SEARCH_TWO_ROUNDS, SEARCH_TWO_ROUNDS + 1)
BUILDERS = {}
for _n in WINDOW_COUNTS:
    BUILDERS[f"window_counts_{_n}"] = functools.partial(window_counts, _n)
BUILDERS["window_lengths"] = window_lengths
for _v in ("dense", "seam", "sparse", "one_long"):
    BUILDERS[f"long_window_{_v}"] = functools.partial(long_window, _v)
BUILDERS["contig_edges"] = contig_edges
for _v in ("dense", "spread", "sparse", "one_long"):
    BUILDERS[f"mixed_junction_widths_{_v}"] = functools.partial(mixed_junction_widths, _v)
BUILDERS["outside_queries"] = outside_queries
BUILDERS["genome_scale"] = genome_scale
for _v in ("no_windows", "no_junctions", "neither"):
    BUILDERS[f"nothing_to_do_{_v}"] = functools.partial(nothing_to_do, _v)
CASES = tuple(BUILDERS)
ONE_LONG = tuple(n for n in CASES if n.endswith("one_long"))     # cases whose stream states a short span first and a long one later


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (names, lens, batch, junctions, windows, ranges, points, mean, sd); built once, shared: callers leave it unchanged"""
    return BUILDERS[name]()


def marked_starts(lens, span, windows, juncs):
    """the tile-marking rule of k_tile_mark_windows / k_tile_mark_junctions, plainly: per contig a flag per 512-bp tile that can hold the start (0-based
    pos) of a record overlapping a depth window (pos + 1 <= end, pos + span >= beg) or being a candidate of a junction window (pos < end,
    pos + span > beg - the kernels use >=: one position more, never fewer)"""
    marks = [np.zeros((max(0, l) >> 9) + 1, bool) for l in lens]
    spans = [(int(w["tid"]), int(w["beg"]) - span, int(w["end"]) - 1) for w in windows] + [(int(j["up_tid"]), int(j["beg"]) - span, int(j["end"]) - 1) for j in juncs]
    for t, p0, p1 in spans:
        if 0 <= t < len(lens) and p1 >= 0:
            marks[t][max(0, p0) >> 9:(p1 >> 9) + 1] = True
    return marks


def candidate_flags(lens, b, windows, juncs):
    """per record: does it start in a marked genome tile (is it staged by the scan), at the span the batch states"""
    marks = marked_starts(lens, int(b["max_ref_span"]), windows, juncs)
    return np.array([0 <= t < len(lens) and p >= 0 and (p >> 9) < len(marks[t]) and bool(marks[t][p >> 9]) for t, p in zip(b["tid"].tolist(), b["pos"].tolist())], bool)
