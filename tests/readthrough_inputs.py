"""Seeded inputs of the `getsv -F` tests (tests/test_readthrough_gpu.py) and of tests/golden/make_readthrough_reference.py, which records
what the real reference writes for them (tests/golden/readthrough/).  Plain Python: the tests rebuild the BAMs from here instead of reading
committed ones.

The -F file holds split alignments in the form `bwa bwasw` writes them: one record per part of a read, records of one name anywhere in the file.
The contigs are those of tests/golden/getsv/pairs1.bam (chrA, chrB, HBV): their byte-wise name order (HBV < chrA < chrB) is not their tid order."""
import os

import numpy as np

import bamio

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BG = os.path.join(GOLDEN, "getsv", "pairs1.bam")
NAMES = ["chrA", "chrB", "HBV"]
LENS = [40000, 15000, 3215]
OPS = "MIDNSHP=X"
QUERY_OPS = "MIS=X"

# getsv flag sets: the reference's defaults, and a loose set that lets junctions with little support through (not -d 0: the reference divides by zero
# for a junction whose two sides are one base apart)
LOOSE = ["-f", "0", "-b", "0", "-T", "100000", "-m", "0"]
SMALL_RUNS = (("loose", LOOSE), ("loose_w0", LOOSE + ["-w", "0"]), ("loose_w20", LOOSE + ["-w", "20"]), ("default", []),
              ("loose_B", LOOSE + ["-B", "@B"]), ("loose_B_w0", LOOSE + ["-B", "@B", "-w", "0"]))
RANDOM_RUNS = (("loose", LOOSE), ("default", []), ("loose_w0", LOOSE + ["-w", "0"]))
RANDOM_SEEDS = tuple(range(8))
# a file of ~130 k records in read order: > 65536 contig changes in one 64 MB chunk of the device decoder, many host batches / 1 MB chunks otherwise
LARGE_SEED, LARGE_NAMES = 100, 60000


def _qlen(cigar):
    return sum(l for l, op in bamio.parse_cigar(cigar) if OPS[op] in QUERY_OPS)


def _seq(rng, n, iupac=False):
    alpha = "ACGTN" + ("RYKMSWBDHV=" if iupac else "")
    p = None if not iupac else np.r_[np.full(5, 0.15), np.full(11, 0.25 / 11)]
    return "".join(rng.choice(list(alpha), n, p=p))


def rec(rng, qname, tid, pos0, cigar, flag=0, mapq=60, iupac=False):
    return dict(qname=qname, flag=flag, tid=tid, pos=pos0, mapq=mapq, cigar=cigar, mtid=-1, mpos=-1, isize=0,
                seq=_seq(rng, _qlen(cigar), iupac), qual=None)


def small_records():
    """hand-made cases (names tell which), in one file order"""
    rng = np.random.RandomState(7)
    A, B, H = 0, 1, 2
    R = lambda *a, **k: rec(rng, *a, **k)  # noqa: E731
    out = [
        # same strand: up is the 3'-clipped record; with and without microhomology, on both strands
        R("ss_mh", A, 1000, "70M30S"), R("ss_mh", A, 5000, "40S60M"),
        R("ss_nomh", A, 2000, "30M70S"), R("ss_nomh", B, 3000, "60S40M"),
        R("ss_mh0", A, 2500, "40M3I7M2D50S"), R("ss_mh0", A, 8000, "50S50M"),   # microhomology 0: MinusCigarRight(.., 0) drops the trailing 2D
        R("ss_rev", B, 4000, "35S65M", flag=16), R("ss_rev", B, 9000, "80M20S", flag=16, iupac=True),
        R("ss_rev_nomh", B, 4500, "60S40M", flag=16), R("ss_rev_nomh", A, 9100, "30M70S", flag=16),
        # opposite strands, 5' sides: up / down by (contig NAME, pos); microhomology moves the down position and grows its CIGAR on the left
        R("os5_mh", B, 500, "30S5I65M"), R("os5_mh", A, 600, "60S40M", flag=16, iupac=True),
        R("os5_mh2", A, 10500, "30S70M", flag=16), R("os5_mh2", H, 600, "45S55M", iupac=True),
        R("os5_nomh", A, 700, "80S20M", flag=16), R("os5_nomh", A, 900, "50S50M"),
        # opposite strands, 3' sides; a tie on (contig, pos): the new record is up
        R("os3_mh", H, 100, "60M40S"), R("os3_mh", A, 100, "70M30S", flag=16, iupac=True),
        R("os3_tie", A, 2980, "20M80S", flag=16), R("os3_tie", A, 2990, "10M90S"),
        R("os3_mh_rev", B, 7000, "65M35S", flag=16, iupac=True), R("os3_mh_rev", B, 6000, "80M20S"),
        # a name three times: hold, drop (same strand, same side), pair; four times: pair, hold anew, pair
        R("three", A, 4000, "30S70M"), R("three", A, 4100, "40S60M"), R("lonely", B, 100, "50M50S"), R("three", A, 4200, "70M30S"),
        R("four", B, 11000, "55M45S"), R("four", B, 12000, "45S55M"), R("four", B, 11000, "55M45S", flag=16), R("four", A, 300, "75M25S"),
        # no pair: opposite strands, different sides
        R("opp_diff", A, 15000, "50M50S"), R("opp_diff", A, 16000, "50S50M", flag=16),
        # 3' branch without S: the last operation's length is the right part; X does not count into the reference length
        R("nos_i", A, 17000, "10I90M"), R("nos_i", A, 18000, "20S80M"),
        R("nos_eq", B, 1200, "100="), R("nos_eq", B, 1500, "30S70M", flag=16),
        R("nos_x", A, 19000, "50M50X"), R("nos_x", A, 19500, "50S50M"),
        R("nos_d", A, 21000, "60M3I30M7D"), R("nos_d", A, 21500, "40S53M"),
        R("x_inside", A, 22000, "30M5X65M30S"), R("x_inside", B, 2000, "30S100M"),
        R("eqx_end", H, 1000, "40=2X58=", flag=16), R("eqx_end", H, 2000, "10S90M"),
        # filters (each name's other record is fine): mapq 0 / 10, unmapped, duplicate, hard clip at either end, S..S, M..M
        R("f_mapq0", A, 23000, "60M40S", mapq=0), R("f_mapq0", A, 24000, "40S60M"),
        R("f_mapq10", A, 25000, "60M40S", mapq=10), R("f_mapq10", A, 26000, "40S60M"),
        R("f_mapq25", B, 13000, "60M40S", mapq=25), R("f_mapq25", B, 14000, "40S60M", mapq=25),
        R("f_unmap", A, 27000, "60M40S", flag=4), R("f_unmap", A, 28000, "40S60M"),
        R("f_dup", A, 29000, "60M40S", flag=1024), R("f_dup", A, 29500, "40S60M"),
        R("f_hard", A, 30000, "30H60M40S"), R("f_hard", A, 30500, "40S60M"),
        R("f_hard2", A, 31000, "40S60M10H"), R("f_hard2", A, 31500, "60M40S"),
        R("f_ss", A, 32000, "10S80M10S"), R("f_ss", A, 32500, "40S60M"),
        R("f_mm", A, 33000, "50M2D50M"), R("f_mm", A, 33500, "40S60M"),
        # several pairs on one junction (chrB 6050 + -> chrA 20001 +): equal lengths add nothing, other lengths add one down support
        R("multi1", B, 6000, "50M50S"), R("multi1", A, 20000, "50S50M"),
        R("multi2", B, 6000, "50M50S"), R("multi2", A, 20000, "50S50M"),
        R("multi3", B, 6010, "60M40S"), R("multi3", A, 20000, "40S60M"),
        R("multi4", A, 20000, "50S50M"), R("multi4", B, 6000, "50M50S"),
        # neighbours a few bases apart (MergeJunction) and a pair across contigs on the minus strand
        R("near1", A, 34000, "60M40S"), R("near1", B, 8000, "40S60M"),
        R("near2", A, 34003, "60M40S"), R("near2", B, 8003, "40S60M"),
        R("cross", H, 2500, "45S55M", flag=16), R("cross", B, 10000, "70M30S", flag=16),
    ]
    # interleave: the two records of most names are not neighbours (records of a name can be far apart in a bwasw file)
    order = list(range(0, len(out), 2)) + list(range(1, len(out), 2))
    return [out[i] for i in order]


def b_rows():
    """-B rows: one on the same key as ss_mh (chrA 1040 + -> chrA 5001 +), one on multi's key"""
    row = lambda u, up, us, d, dp, ds: "\t".join(str(x) for x in (u, up, us, 3, d, dp, ds, 2, 0, 0, "NA", 0, 0, 0, 0, 0, 0, 0, 0, "50M", "50M", "ACGT", "ACGT")) + "\n"  # noqa: E731
    return row("chrA", 1040, "+", "chrA", 5001, "+") + row("chrB", 6050, "+", "chrA", 20001, "+")


def random_records(seed, n_names=1500, lens=None):
    """a few thousand split alignments around hot points (shared junctions, neighbours), names 1-4 times, with some records every filter drops
    (lens: the contigs' lengths, those of NAMES by default)"""
    LENS_ = LENS if lens is None else [int(x) for x in lens]
    nt = len(LENS_)
    rng = np.random.RandomState(1000 + seed)
    hot = [(int(rng.randint(0, nt)), 0) for _ in range(40)]
    hot = [(t, int(rng.randint(200, LENS_[t] - 400))) for t, _ in hot]
    recs = []
    for k in range(n_names):
        name = f"rt{seed}_{k}" + ("_" + "x" * int(rng.randint(0, 60)) if rng.rand() < 0.1 else "")
        times = int(rng.choice([1, 2, 2, 2, 2, 3, 4]))
        for _ in range(times):
            t, p = hot[int(rng.randint(0, len(hot)))] if rng.rand() < 0.7 else (int(rng.randint(0, nt)), 0)
            if p == 0:
                p = int(rng.randint(200, LENS_[t] - 400))
            p += int(rng.choice([0, 0, 0, 1, 2, -3, 7]))
            L = int(rng.choice([100, 100, 150, 76]))
            s = int(rng.randint(10, L - 10))
            form = rng.rand()
            if form < 0.42:
                cig = f"{s}S{L - s}M"
            elif form < 0.84:
                cig = f"{L - s}M{s}S"
            elif form < 0.88:
                cig = f"{s}S{L - s - 5}M2D5M"
            elif form < 0.91:
                cig = f"{L - s - 3}M3I{s - 3}M" if s > 6 else f"{L}M"
            elif form < 0.93:
                cig = f"{L}="
            elif form < 0.95:
                cig = f"{L - s}M{s}X"
            elif form < 0.97:
                cig = f"{s}H{L - s}M"
            else:
                cig = f"{s // 2 + 1}S{L - s - 2}M{s - s // 2 + 1}S"
            flag = (16 if rng.rand() < 0.5 else 0) | (1024 if rng.rand() < 0.01 else 0) | (4 if rng.rand() < 0.01 else 0)
            mapq = int(rng.choice([60, 60, 60, 37, 15, 1, 0]))
            recs.append(rec(rng, name, t, p - (L - s if "M" in cig and cig.endswith("S") else 0), cig, flag=flag, mapq=mapq, iupac=rng.rand() < 0.05))
    return [recs[i] for i in rng.permutation(len(recs))]  # (the records of a name anywhere in the file)


def write_f_bam(path, recs, names=None, lens=None):
    names, lens = (NAMES, LENS) if names is None else (list(names), [int(x) for x in lens])
    for r in recs:
        r["pos"] = max(0, min(int(r["pos"]), lens[r["tid"]] - 1))
    bamio.write_bam(path, names, lens, recs)


def empty_clip_inputs(d):
    """an empty clip.bam and clip file: only -F (and -B) junctions"""
    cb, cg = os.path.join(d, "e.clip.bam"), os.path.join(d, "e.clip")
    bamio.write_bam(cb, NAMES, LENS, [])
    open(cg, "w").close()
    return cb, cg


def flags_with(flags, bfile):
    return [bfile if f == "@B" else f for f in flags]


def unpath(line):
    """a stderr line without the place of the original BAM (the reference names it)"""
    return line.replace(BG, "{BG}")


def contig_changes(recs):
    """contig changes among the records that are not UNMAP|MUNMAP (what the device decoder's contig-change list counts)"""
    t = [r["tid"] for r in recs if not (r["flag"] & 12)]
    return sum(1 for a, b in zip(t, t[1:]) if a != b)
