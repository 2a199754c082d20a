"""Hand-made record sets and region lists for `seeksv run -L` / `-X` (the rule: include/seeksv_hip.h, ssv_regions_set; in plain Python: tests/region_model.py).
Every set is about one thing, which `claim` states and tests/test_region_inputs.py asserts; tests/test_region_gpu.py sends the sets through the kernels, each in
both modes.  Where the answer at a boundary matters it is written out by hand (GRID_EXPECT, `kept` / `kept_x`), not taken from the model.

Records are dicts as tests/bamio.py's encode_record takes them.  Read names do not travel with a retained batch, so every record carries its index in the set
as `isize`.  Regions are (tid, s, t) AS GIVEN - unsorted, overlapping, past the contig's end - and region_model.normalise() makes the library's list."""
import re

BASES = "ACGT"
QUERY_OPS = "MIS=X"
CIGAR_RE = re.compile(r"(\d+)([MIDNSHP=X])")
LDS_CAPACITY = 2048      # regions of one contig the selection stages in LDS (ssv_region_lds_capacity)
TILE = 256               # records of one tile of the per-record kernels
BLOCK_RECORDS = 4096     # records of one workgroup of the selection (16 tiles)
GATHER_GROUP = 16        # records of one 256-thread workgroup of the gather (16 lanes a record)


def rec(tid, pos, cigar="10M", flag=0, l=None, mtid=-1, mpos=-1):
    if l is None:
        l = sum(int(n) for n, op in CIGAR_RE.findall(cigar) if op in QUERY_OPS) if cigar != "*" else 10
    seq = "".join(BASES[(k * 7 + pos) % 4] for k in range(l))
    return dict(qname="r", flag=flag, tid=tid, pos=pos, mapq=60, cigar=cigar, mtid=mtid, mpos=mpos, isize=0, seq=seq, qual=bytes([30 + (pos + k) % 8 for k in range(l)]))


SETS = []


def add(name, records, regions, lens, **claim):
    records = [dict(r, isize=i, qname=f"r{i}") for i, r in enumerate(records)]
    SETS.append(dict(name=name, records=records, regions=list(regions), lens=list(lens), targets=[f"c{k}" for k in range(len(lens))], claim=claim))


# ---- the grid: one contig of 64 bases among three, one record at every position for every shape ----
GRID_LENS = [1000, 64, 1000]
GRID_REGIONS = [(1, 40, 41), (1, 20, 25), (1, 60, 70), (1, 10, 20)]      # [10,20) + [20,25) abut: one region [10,25); [60,70) is clipped to [60,64)
GRID_NORMALISED = [(1, 10, 25), (1, 40, 41), (1, 60, 64)]
NINE_OPS = "1M1I1M1D1M1I1M2D1M"      # span 8, and only cigar[] says so: the line holds five operations
GRID_SHAPES = [("10M", 0), ("1M", 0), ("5S5M", 0), ("3M4D3M", 0), ("2M30N2M", 0), (NINE_OPS, 0), ("*", 0), ("*", 4)]
GRID_SPAN = {"10M": 10, "1M": 1, "5S5M": 5, "3M4D3M": 10, "2M30N2M": 34, NINE_OPS: 8, "*": 0}
GRID_POSITIONS = list(range(-1, 64))
add("grid", [rec(1, p, c, flag=f, mtid=1 if f else -1, mpos=p if f else -1) for c, f in GRID_SHAPES for p in GRID_POSITIONS], GRID_REGIONS, GRID_LENS,
    n=len(GRID_SHAPES) * len(GRID_POSITIONS), normalised=GRID_NORMALISED)
# (cigar, flag, pos) -> overlaps, at the boundaries: e == s and pos == t do not overlap; e == s + 1 and pos == t - 1 do
GRID_EXPECT = {
    ("10M", 0, -1): False, ("10M", 0, 0): False, ("10M", 0, 1): True, ("10M", 0, 24): True, ("10M", 0, 25): False, ("10M", 0, 30): False, ("10M", 0, 31): True,
    ("10M", 0, 40): True, ("10M", 0, 41): False, ("10M", 0, 50): False, ("10M", 0, 51): True, ("10M", 0, 63): True,
    ("1M", 0, 9): False, ("1M", 0, 10): True, ("1M", 0, 19): True, ("1M", 0, 20): True, ("1M", 0, 24): True, ("1M", 0, 25): False, ("1M", 0, 39): False, ("1M", 0, 40): True,
    ("1M", 0, 41): False, ("1M", 0, 59): False, ("1M", 0, 60): True, ("1M", 0, 63): True,
    ("5S5M", 0, 5): False, ("5S5M", 0, 6): True, ("5S5M", 0, 35): False, ("5S5M", 0, 36): True,      # the clipped bases do not count
    ("3M4D3M", 0, 0): False, ("3M4D3M", 0, 1): True, ("3M4D3M", 0, 30): False, ("3M4D3M", 0, 31): True,      # the deletion does
    ("2M30N2M", 0, -1): False, ("2M30N2M", 0, 0): True, ("2M30N2M", 0, 25): True, ("2M30N2M", 0, 26): True, ("2M30N2M", 0, 63): True,      # 34 bases reach a region from everywhere
    (NINE_OPS, 0, 2): False, (NINE_OPS, 0, 3): True, (NINE_OPS, 0, 32): False, (NINE_OPS, 0, 33): True, (NINE_OPS, 0, 52): False, (NINE_OPS, 0, 53): True,
    ("*", 0, -1): False, ("*", 0, 9): False, ("*", 0, 10): True, ("*", 0, 24): True, ("*", 0, 25): False, ("*", 0, 40): True, ("*", 0, 41): False,
    ("*", 4, -1): False, ("*", 4, 9): False, ("*", 4, 10): True, ("*", 4, 24): True, ("*", 4, 25): False, ("*", 4, 60): True,      # no flag bit takes part
}
# ---- unplaced records, in both modes ----
add("unplaced", [rec(0, 100), rec(-1, -1, "*", flag=4), rec(0, 300), rec(-1, -1, "*", flag=0x4d), rec(-1, -1, "*", flag=0x45), rec(0, 150)], [(0, 90, 160)], [1000],
    kept=[0, 5], kept_x=[1, 2, 3, 4])

# ---- contigs with and without regions, in front of and behind each other; the last contig ----
add("contig_order", [rec(0, 5), rec(0, 50), rec(1, 5), rec(1, 50), rec(2, 5), rec(2, 50), rec(3, 5), rec(3, 40), rec(3, 989)], [(1, 0, 10), (3, 45, 46), (3, 990, 2000)], [1000] * 4,
    kept=[2, 7, 8], kept_x=[0, 1, 3, 4, 5, 6], without_regions=[0, 2], last_contig=3)

# ---- contig changes that fall on dropped records: the output's change list is not the decoder's ----
add("changes_on_dropped", [rec(0, 10), rec(0, 500), rec(1, 10), rec(1, 500), rec(1, 600, flag=0x49, mtid=1, mpos=600), rec(2, 10), rec(2, 500), rec(0, 700)],
    [(0, 495, 520), (1, 495, 520), (1, 600, 601), (2, 495, 520), (0, 700, 701)], [1000] * 3,
    kept=[1, 3, 4, 6, 7], changes_in=[(2, 1), (5, 2), (7, 0)], changes_out=[(1, 1), (3, 2), (4, 0)],
    kept_x=[0, 2, 5], changes_out_x=[(1, 1), (2, 2)])

# ---- 1, 2 and 3 regions on a contig, and 10,000 one-base regions two bases apart: a list that does not fit LDS ----
MANY = 10000
MANY_AT = 1000
_many = [(3, MANY_AT + 2 * k, MANY_AT + 2 * k + 1) for k in range(MANY)]
_many_recs = []
for _p in (0, MANY_AT - 2, MANY_AT - 1, MANY_AT, MANY_AT + 1, MANY_AT + 2, MANY_AT + 3, MANY_AT + 2 * MANY - 3, MANY_AT + 2 * MANY - 2, MANY_AT + 2 * MANY - 1, MANY_AT + 2 * MANY, MANY_AT + 2 * MANY + 50):
    _many_recs += [rec(3, _p, "1M"), rec(3, _p, "2M"), rec(3, _p, "*", flag=4)]
_many_recs += [rec(3, MANY_AT + 7 * k + 1, "1M") for k in range(300)] + [rec(3, MANY_AT + 7 * k, "1M") for k in range(300)]
add("region_counts", [rec(0, p, "4M") for p in (0, 96, 97, 100, 109, 110)] + [rec(1, p, "4M") for p in (96, 97, 115, 116, 117, 130)] + [rec(2, p, "4M") for p in (96, 97, 110, 150, 196, 197, 310)]
    + _many_recs, [(0, 100, 110), (1, 100, 110), (1, 120, 130), (2, 100, 110), (2, 200, 210), (2, 300, 310)] + _many, [100000] * 4,
    per_contig=[1, 2, 3, MANY], between=True, on=True, straddling=True)

# ---- empty lists, empty batches, one record ----
add("n0_list", [rec(0, 10), rec(-1, -1, "*", flag=4), rec(1, 10)], [], [1000, 1000], kept=[], kept_x=[0, 1, 2])
add("n0_records", [], [(0, 10, 20)], [1000], kept=[], kept_x=[])
add("one_kept", [rec(0, 15)], [(0, 10, 20)], [1000], kept=[0], kept_x=[])
add("one_dropped", [rec(0, 25)], [(0, 10, 20)], [1000], kept=[], kept_x=[0])
add("all_kept", [rec(k % 2, 100 + 3 * k) for k in range(300)], [(0, 0, 1000), (1, 50, 1000)], [1000, 1000], kept=list(range(300)), kept_x=[])
add("none_kept", [rec(k % 2, 100 + 3 * k) for k in range(300)], [(0, 0, 100), (1, 0, 50)], [1000, 1000], kept=[], kept_x=list(range(300)))

# ---- clipped records with bases beside unclipped records without (the BAM decoder ships the bases of clipped records only), kept and dropped ----
_sq = []
for _k in range(40):
    _sq += [rec(0, 100 + 10 * _k, "3S7M"), rec(0, 101 + 10 * _k, "10M"), rec(0, 102 + 10 * _k, "6M5S"), rec(0, 103 + 10 * _k, "7M", l=0)]
add("seq_repack", _sq, [(0, 150, 200), (0, 300, 331)], [1000], clipped=80, odd_and_even_lengths=True)

# ---- more than one workgroup of the selection; tiles that stay on a contig and tiles that a contig change falls into ----
add("blocks", [rec(0, 10 * k) for k in range(5000)] + [rec(1, 10 * k, "2S8M") for k in range(3600)], [(0, 995, 20000), (0, 30001, 30002), (1, 0, 5), (1, 17000, 17001), (1, 35995, 36000)],
    [100000, 100000], n=8600)

BY_NAME = {s["name"]: s for s in SETS}


# ---- the BED of tests/test_region_cli_gpu.py, over the sample of tests/pairdup_cli_inputs.py (two contigs of 60,000 bases) ----
CLI_SEED = 355


def cli_bed(lens=(60000, 60000)):
    """regions AS GIVEN (unsorted, some overlapping): junction A's clipped reads planted, the rest drawn with a fixed seed so that between a third and two thirds of the
    sample's records stay (asserted in tests/test_region_inputs.py)"""
    import random
    rng = random.Random(CLI_SEED)
    out = [(0, 19800, 20300)]      # (the clipped reads of junction A; their mates on the other contig lie outside every region)
    for _ in range(14):
        tid = rng.randrange(len(lens))
        s = rng.randrange(0, lens[tid] - 100)
        out.append((tid, s, s + rng.randrange(300, 10000)))
    rng.shuffle(out)
    return out


def bed_text(regions, names):
    return "".join(f"{names[t]}\t{s}\t{e}\n" for t, s, e in regions)
