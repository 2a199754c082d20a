"""Hand-made record sets for the coordinate sort of `seeksv run -u` (the rule: include/seeksv_hip.h, ssv_batch_sort; in plain Python: tests/coordsort_model.py).
Every set is about one thing, which `claim` states and tests/test_coordsort_inputs.py asserts; tests/test_coordsort_gpu.py sends the sets through the kernels.

Records are dicts as tests/bamio.py's encode_record takes them.  Read names do not travel with a retained batch, so every record carries its index in the set
as `isize`: two records with equal keys can still be told apart, which is what a test of stability needs.  `cuts` (optional): where the set's own input batches
begin - sets without it are cut into equal parts by the tests."""
import functools
import random
import struct

import bamio
import markdup_cli_inputs as CI

TARGETS = ["c0", "c1", "c2"]
MAX_LEN = 2 ** 31 - 1
BIG_N = 70000          # contig ids up to 69,999: every byte of a 17-bit contig rank is exercised
BASES = "ACGT"


def rec(tid, pos, flag=0, cigar="10M", l=10, mtid=-1, mpos=-1, qual=30):
    seq = "".join(BASES[(k * 7 + pos) % 4] for k in range(l))
    return dict(qname="r", flag=flag, tid=tid, pos=pos, mapq=60, cigar=cigar, mtid=mtid, mpos=mpos, isize=0, seq=seq, qual=bytes([qual] * l))


SETS = []


def add(name, records, n_targets=3, cuts=None, **claim):
    records = [dict(r, isize=i, qname=f"r{i}") for i, r in enumerate(records)]
    SETS.append(dict(name=name, records=records, n_targets=n_targets, cuts=cuts, claim=claim))


def targets_of(s):
    """-> (contig names, lengths) of a set's header"""
    n = s["n_targets"]
    return (TARGETS[:n] if n <= 3 else [f"t{i}" for i in range(n)]), [MAX_LEN] * n


def scattered(n, seed, n_pos=40):
    """n records on three contigs and among the unplaced, at few positions: most keys are shared"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        tid = rng.choice([0, 0, 1, 2, -1])
        out.append(rec(tid, rng.randrange(n_pos) * 10 if tid >= 0 else -1, flag=0 if tid >= 0 else 4))
    return out


# ---- record counts ----
add("n0", [], n=0)
add("n1", [rec(1, 100)], n=1)
add("n2", [rec(1, 100), rec(0, 100)], n=2)
add("all_equal", [rec(1, 500) for _ in range(300)], n=300, distinct_keys=1)
for _n in (63, 64, 65, 2047, 2048, 2049):     # a wavefront, and radix_sort.h's tile of 2048 keys
    add(f"n{_n}", scattered(_n, _n), n=_n)

# ---- keys ----
add("pos_extremes", [rec(1, MAX_LEN - 1), rec(1, 0), rec(1, -1, flag=4), rec(0, MAX_LEN - 1), rec(1, 5), rec(0, -1, flag=4), rec(1, MAX_LEN - 1), rec(1, -1, flag=4)],
    positions=[-1, MAX_LEN - 1])
_tids = [0, 255, 256, 65535, 65536, 69999, -1]
_tb = [rec(t, p, flag=0 if t >= 0 else 4) for p in (700, 3, 700) for t in _tids]
random.Random(5).shuffle(_tb)
add("tid_bytes", _tb, n_targets=BIG_N, tids=_tids)
add("one_target", [rec(-1, -1, flag=4), rec(0, 9), rec(-1, -1, flag=4), rec(0, 2), rec(0, 9)], n_targets=1, tids=[0, -1])

# ---- batches and ties ----
# three input batches, each in order by itself; c0:100 lies in all three, c0:300 in the first and the last, c1:50 in the first two: the earlier batch wins a tie
add("three_batches", [rec(0, 100), rec(0, 300), rec(1, 50),
                      rec(0, 100), rec(0, 200), rec(1, 50),
                      rec(0, 50), rec(0, 100), rec(0, 300)], cuts=[3, 6], ties_across={(0, 100): 3, (0, 300): 2, (1, 50): 2})
add("reversed", [rec(t, p) for t in (2, 1, 0) for p in range(990, -10, -15)], strictly_down=True)
_srt = sorted(scattered(200, 77), key=lambda r: (r["tid"] if r["tid"] >= 0 else 3, r["pos"]))
add("sorted", _srt, sorted=True)
add("sorted_but_last", _srt + [rec(0, 0)], sorted_but=1)

# ---- variable parts ----
_ops70 = "1M1I" * 34 + "1M1S"       # 70 operations, 70 bases
_cig = [rec(2, 40, cigar="*", flag=4), rec(2, 30, cigar="10M"), rec(1, 90, cigar="2S2M1I2M1D3M", l=10), rec(1, 80, cigar="2S3M1I2M2S", l=10), rec(0, 500, cigar=_ops70, l=70),
        rec(0, 400, cigar="3S7M"), rec(0, 500, cigar="2S3M1I2M2S", l=10), rec(0, 400, cigar=_ops70, l=70), rec(2, 30, cigar="*", flag=4)]
add("cigar_lengths", _cig, n_ops=[0, 1, 5, 6, 70])
# odd, even and no bases; soft-clipped records (whose bases every decoder ships) beside others (whose bases the BAM decoder leaves out)
_lq = [rec(1, 70, cigar="2S5M", l=7), rec(1, 60, cigar="8M", l=8), rec(1, 50, cigar="7M", l=0), rec(0, 70, cigar="4M4S", l=8), rec(0, 60, cigar="7M", l=7), rec(1, 50, cigar="3S4M", l=7),
       rec(0, 60, cigar="1S7M", l=8), rec(1, 50, cigar="2S6M", l=0)]
add("read_lengths", _lq, l_qseq=[0, 7, 8], clipped=5)
# reads and mates with one unmapped end lie at the mapped end's place: sorted, c1 is seen only in such records until the last one, and c2 before it
_um = [rec(2, 10), rec(1, 30, flag=0x49, mtid=1, mpos=30), rec(0, 20), rec(1, 30, flag=0x85, mtid=1, mpos=30), rec(1, 20, flag=0x89, mtid=1, mpos=20), rec(0, 10),
       rec(1, 20, flag=0x45, mtid=1, mpos=20), rec(-1, -1, flag=0x4d), rec(1, 40)]
add("unmapped_ends", _um, skipped=5, changes=[(6, 1), (7, 2)])

# ---- depth: 10^5 records at one key ----
add("deep_tie", [rec(1, 12345) for _ in range(100000)], n=100000, distinct_keys=1)

BY_NAME = {s["name"]: s for s in SETS}


def write_bam(path, names, lens, records):
    """bamio.write_bam for any number of contigs: the header in BGZF blocks of 0xff00 bytes like the records (70,000 contigs are 1.4 MB of header)"""
    text = sam_header(names, lens).encode()
    stream = b"".join([b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(names))]
                      + [struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l) for n, l in zip(names, lens)]
                      + [bamio.encode_record(r) for r in records])
    with open(path, "wb") as f:
        for at in range(0, len(stream), 0xff00):
            f.write(bamio._bgzf_block(stream[at:at + 0xff00]))
        f.write(bamio.BGZF_EOF)


def batches_of(s, n_batches):
    """the set's records as input batches: its own cuts when it has them, else n_batches parts of equal size"""
    r = s["records"]
    cuts = s["cuts"] if s["cuts"] else [len(r) * k // n_batches for k in range(1, n_batches)]
    b = [0] + list(cuts) + [len(r)]
    return [r[b[k]:b[k + 1]] for k in range(len(b) - 1)]


# ---- the sample of tests/test_coordsort_cli_gpu.py ----
N_HALF_MAPPED = 36


@functools.lru_cache(maxsize=None)
def cli_sample():
    """-> (contigs, records): tests/markdup_cli_inputs.py's sample (40,000 records, a pile of 11,000 at one place) plus N_HALF_MAPPED pairs with one unmapped
    end - the mapped read (0x8 set) and its unmapped mate (0x4 set) both at the mapped read's place, as aligners write them -, coordinate sorted"""
    contigs, recs = CI.sample()
    rng = random.Random(2049)
    extra = []
    for k in range(N_HALF_MAPPED):
        tid = k % 2
        pos = rng.randrange(100, CI.LENS[tid] - 400)
        c = contigs[tid]
        first = k % 3 != 0      # which read of the pair is the mapped one
        other = "".join(rng.choice(BASES) for _ in range(100))
        q = bytes(rng.randrange(20, 40) for _ in range(100))
        extra.append(dict(qname=f"half{k}", flag=0x1 | 0x8 | (0x40 if first else 0x80), tid=tid, pos=pos, mapq=60, cigar="100M", mtid=tid, mpos=pos, isize=0, seq=c[pos:pos + 100], qual=q))
        extra.append(dict(qname=f"half{k}", flag=0x1 | 0x4 | (0x80 if first else 0x40), tid=tid, pos=pos, mapq=0, cigar="*", mtid=tid, mpos=pos, isize=0, seq=other, qual=q[::-1]))
    allr = sorted(list(recs) + extra, key=lambda r: (r["tid"], r["pos"]))
    return contigs, tuple(allr)


def shuffled(recs, seed=7):
    r = list(recs)
    random.Random(seed).shuffle(r)
    return r


def by_name(recs):
    """read-name order, as an aligner writes its pairs: a stable sort by name"""
    return sorted(recs, key=lambda r: r["qname"])


def sam_header(names, lens):
    return "@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(names, lens))
