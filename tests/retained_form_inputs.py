"""Record sets for tests/test_retained_form_gpu.py: what the four producers of a retained batch (ssv_batch_retain, ssv_dup_retain, ssv_pairdup_retain,
ssv_batch_sort) are handed, so that the form they write can be compared.  tests/test_retained_form_inputs.py holds the sets to what they are said to be, on the CPU.

Records are dicts as tests/bamio.py's encode_record takes them (tests/pairdup_inputs.py's read and pair)."""
import pairdup_inputs as pi

TARGETS = pi.TARGETS

CIGAR17 = "3M1I3M1D3M1I3M1D3M1I3M1D3M1I3M1D3M"      # 17 operations: the 16 lanes of a record go round twice


def _quals(k, n):
    return bytes(20 + (7 * k + 3 * j) % 20 for j in range(n))


def _form():
    """20 records on two contigs, no two at one place, that neither duplicate rule marks: four proper pairs, a pair with an unmapped mate, nine single reads, one unplaced record"""
    pairs = [(("a", (0, 100, "20M", False), (0, 300, "20M", True))),
             (("b", (0, 150, "15S25M", False), (0, 400, "20M", True))),             # 40 bases, soft-clipped: 60 bytes of bases + qualities
             (("c", (0, 200, CIGAR17, False), (1, 500, "20M", True))),
             (("d", (1, 100, "25M15S", False), (1, 700, "10M2D10M", True)))]
    recs = []
    for name, x, y in pairs:
        recs += list(pi.pair(name, x, y))
    recs += [pi.read("m", 0x1 | 0x8 | 0x40, 1, 800, "20M", 1, 800), pi.read("m", 0x1 | 0x4 | 0x80, 1, 801, None, 1, 800)]     # (no two records at one place: any stable sort gives one order)
    singles = [(0, 50, "10M1I9M", 0), (0, 250, "20M", 0), (0, 260, "5S15M", 16), (0, 900, "6H20M", 0), (1, 50, "20M", 16), (1, 300, "20M", 0), (1, 900, "3S17M", 0),
               (1, 950, "12M4N8M", 16), (1, 990, "20M5S", 0)]
    recs += [pi.read(f"s{k}", flag, tid, pos, cigar, -1, -1) for k, (tid, pos, cigar, flag) in enumerate(singles)]
    recs.append(pi.read("u", 0x4, -1, -1, None, -1, -1))                            # unplaced, no operations: the last record in coordinate order
    for k, r in enumerate(recs):
        r["qual"] = _quals(k, len(r["seq"]))
    return pi.in_order(recs)[0]


FORM = _form()
ONE = [dict(FORM[2])]            # n = 1
NONE = []                        # n = 0

# Records that need sorting and marking across a seam: the twelve records of pairdup_inputs' reverse_ends in descending order - every read 2 (position 300)
# in front of every read 1 (position 100) - cut in the middle, so that every pair has one mate on either side and the sort moves the second half in front.
SEAM = pi.orders(pi.BY_NAME["reverse_ends"])[2][1]
SEAM_CUT = len(SEAM) // 2
