"""The sample of tests/test_markdup_cli_gpu.py: some 40,000 records (8 MB of BAM records) on two contigs with two planted inter-contig junctions.  Junction A
is supported by two distinct soft-clipped pairs plus three copies of each - eight clipped reads in a file whose duplicates are not marked, two once they
are; junction B by four distinct pairs.  Background: proper pairs of 100-base reads over both contigs, none clipped, no two at one place.

The file is laid out for a reader that takes it in chunks of 1 MB inflated (SSV_CHUNK_INFLATED_MB=1; tests/bamio.py writes the header as a block of its own and
the records as blocks of 0xff00 bytes, so a chunk is 16 record blocks and a seam falls at every multiple of SEAM bytes of the record stream; the record
that straddles a seam belongs to the later batch).  Optional fields of padding (XZ:Z:) on background records move the records so that
  - the first seam falls inside junction A's first run of four heads (an original and its copies),
  - another seam falls right behind the first record of tB: the contig change is the last record of its batch, the one that is held back,
and a pile of PILE single reads at one place of tB - they take no part - is longer than two chunks, so one batch is a single run from end to end."""
import functools

import numpy as np

import bamio
import markdup_model as mm
from realign_inputs import dna

NAMES, LENS = ("tA", "tB"), (60000, 60000)
JUNCTION_A, JUNCTION_B = ((0, 20000), (1, 900)), ((0, 22000), (1, 1800))   # 0-based: the last base of tA before the breakpoint, the first base of tB behind it
COPIES = 3
SEAM = 16 * 0xff00      # bytes of the record stream in a chunk of 1 MB inflated
PILE, PILE_POS = 11000, 40000


def record_ends(recs):
    """where every record ends in the BAM's record stream"""
    out, at = [], 0
    for r in recs:
        at += len(bamio.encode_record(r))
        out.append(at)
    return out


def batch_of(ends):
    """the 1 MB chunk (0-based) whose batch a record comes out in: the one in which it is complete"""
    return [(e - 1) // SEAM for e in ends]


def pad(recs, first, last, n_bytes):
    """n_bytes (>= 8) of optional fields on background records among recs[first:last], at most 250 bytes a record"""
    assert n_bytes >= 8
    for i in range(first, last):
        if n_bytes == 0:
            break
        if not recs[i]["qname"].startswith("bg") or "aux" in recs[i]:
            continue
        take = n_bytes if n_bytes <= 250 else (250 if n_bytes - 250 >= 8 else n_bytes - 8)
        recs[i] = dict(recs[i], aux=b"XZZ" + b"p" * (take - 4) + b"\0")
        n_bytes -= take
    assert n_bytes == 0, "not enough records to pad"


@functools.lru_cache(maxsize=None)
def sample():
    """-> (contigs, records for bamio.write_bam, coordinate sorted, no duplicate flag set)"""
    rng = np.random.RandomState(1024)
    a, b = dna(rng, LENS[0]), dna(rng, LENS[1])
    recs = []
    qual = lambda n, lo=30: bytes((lo + rng.randint(0, 10, n)).tolist())  # noqa: E731
    for tid, c in enumerate((a, b)):
        for i, p in enumerate(range(5, len(c) - 320, 8)):
            name = f"bg{tid}_{i}"
            recs.append(dict(qname=name, flag=99, tid=tid, pos=p, mapq=60, cigar="100M", mtid=tid, mpos=p + 200, isize=300, seq=c[p:p + 100], qual=qual(100)))
            recs.append(dict(qname=name, flag=147, tid=tid, pos=p + 200, mapq=60, cigar="100M", mtid=tid, mpos=p, isize=-300, seq=c[p + 200:p + 300], qual=qual(100)))

    def clipped_pair(name, junction, m, mate_pos, lo):
        """first read: m bases of tA up to the breakpoint, then 100 - m bases of tB behind it (soft-clipped); its mate lies on tB"""
        (_, ja), (_, jb) = junction
        p = ja + 1 - m
        seq = a[p:ja + 1] + b[jb:jb + 100 - m]
        return [dict(qname=name, flag=97, tid=0, pos=p, mapq=60, cigar=f"{m}M{100 - m}S", mtid=1, mpos=mate_pos, isize=0, seq=seq, qual=qual(100, lo)),
                dict(qname=name, flag=145, tid=1, pos=mate_pos, mapq=60, cigar="100M", mtid=0, mpos=p, isize=0, seq=b[mate_pos:mate_pos + 100], qual=qual(100, lo))]

    for j in range(2):
        recs += clipped_pair(f"A{j}", JUNCTION_A, 60 + 5 * j, 1203 + 11 * j, 30)
        for k in range(COPIES):
            recs += clipped_pair(f"A{j}copy{k}", JUNCTION_A, 60 + 5 * j, 1203 + 11 * j, 20)
    for j in range(4):
        recs += clipped_pair(f"B{j}", JUNCTION_B, 50 + 5 * j, 2103 + 11 * j, 30)
    for k in range(PILE):
        recs.append(dict(qname=f"pile{k}", flag=16 * (k % 2), tid=1, pos=PILE_POS, mapq=60, cigar="100M", mtid=-1, mpos=-1, isize=0, seq=b[PILE_POS:PILE_POS + 100], qual=qual(100)))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    # the first seam between the second and the third head of junction A's first run
    run_a = [i for i, r in enumerate(recs) if r["qname"].startswith("A0") and r["tid"] == 0]
    ends = record_ends(recs)
    assert ends[run_a[1]] < SEAM - 300
    pad(recs, 0, run_a[0], SEAM - 60 - ends[run_a[1]])
    # ... and the next seam behind it right behind the first record of tB
    first_b = next(i for i, r in enumerate(recs) if r["tid"] == 1)
    ends = record_ends(recs)
    k = ends[first_b] // SEAM + 1
    pad(recs, run_a[-1] + 1, first_b, k * SEAM - 60 - ends[first_b])
    return (a, b), tuple(recs)


def flagged(recs):
    """the records with the model's duplicate flags set"""
    return tuple(dict(r, flag=f) for r, f in zip(recs, mm.mark(list(recs))))


def names_both_ends(text, junction):
    """does a line of `text` name both ends of the junction (1-based positions)?"""
    (_, ja), (_, jb) = junction
    x, y = ("tA", str(ja + 1)), ("tB", str(jb + 1))
    for line in text.splitlines():
        f = line.split("\t")
        pairs = set(zip(f, f[1:]))
        if x in pairs and y in pairs:
            return True
    return False
