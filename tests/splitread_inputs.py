"""Hand-made inputs for `seeksv run -A` (the split-read rule, tests/splitread_model.py), one rule per set, with the expected pairs WRITTEN OUT: every set is
dict(name, records, rows, counts, ...) where records are the dicts tests/bamio.py writes (qname, flag, tid, pos 0-based, mapq, cigar text, seq; `no_seq`:
the host batch says SSV_NO_SEQ for it although l_qseq is the SEQ's length - a form only a host batch can have) and rows are what the pass must give, in the
order of the completing record: row(key, kind, microhomology, up_seq, down_seq, up_cigar, down_cigar, edits, clipped, records).  The seqs are slices of the
reads below, written as Python slices - nothing here calls the model.

All reads lie on the forward strand of their own bases: a '+' record stores READ, a '-' record stores rc(READ), so that the two records of a split read hold
the same bases and a borrowed seq can be told from a wrong one.  Contigs: tid 0 is "chrB", tid 1 is "chrA" - byte-wise name order is not tid order."""
import numpy as np

import readthrough_model as RM

CONTIGS = ["chrB", "chrA"]
LENS = [20000, 20000]
SUPP, REV, READ1, READ2, SECONDARY, DUP, UNMAP = 2048, 16, 1 | 64, 1 | 128, 256, 1024, 4
COUNT_KEYS = ("candidates", "hard_clipped", "pairs", "pairs_borrowed", "dropped_no_carrier", "dropped_length")


def _bases(n, seed):
    rng = np.random.RandomState(seed)
    return "".join("ACGTN"[k] for k in rng.choice(5, n, p=[0.24, 0.24, 0.24, 0.24, 0.04]))


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


S = _bases(100, 1)          # the read of most sets
RC = rc(S)
S2 = _bases(100, 2)         # read 2 of the paired-end set
LONG = _bases(300, 3)       # the reads of the length set are its prefixes


def rec(qname, flag, pos, cigar, seq, tid=0, mapq=60, **kw):
    return dict(qname=qname, flag=flag, tid=tid, pos=pos, mapq=mapq, cigar=cigar, mtid=-1, mpos=-1, isize=0, seq=seq, qual=None, **kw)


def ops(text):
    return [(l << 4) | "MIDNSHP=X".index(ch) for l, ch in RM.parse_cigar_text(text)]


def row(key, kind, mh, up_seq, down_seq, up_cigar, down_cigar, edits, clipped, records):
    up, down = key[:3], key[3:]
    return dict(key=(CONTIGS[up[0]], up[1], up[2], CONTIGS[down[0]], down[1], down[2]), kind=kind, microhomology=mh, up_seq=up_seq, down_seq=down_seq,
                up_cigar=ops(up_cigar), down_cigar=ops(down_cigar), edits=edits, clipped=clipped, records=records)


def counts(candidates, hard_clipped, pairs, pairs_borrowed, dropped_no_carrier=0, dropped_length=0):
    return dict(candidates=candidates, hard_clipped=hard_clipped, pairs=pairs, pairs_borrowed=pairs_borrowed, dropped_no_carrier=dropped_no_carrier,
                dropped_length=dropped_length)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the two cases worked by hand in the rule's description
# ---------------------------------------------------------------------------------------------------------------------------------------------
def worked():
    records = [rec("w1", 0, 999, "60M40S", S), rec("w1", SUPP, 4999, "60H40M", S[60:]),
               rec("w1b", 0, 999, "62M38S", S), rec("w1b", SUPP, 4999, "60H40M", S[60:]),
               rec("w2", 0, 999, "60M40S", S), rec("w2", SUPP | REV, 4999, "40M60H", RC[:40])]
    rows = [row((0, 1059, "+", 0, 5000, "+"), 0, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0), (0, 1)),
            row((0, 1059, "+", 0, 5000, "+"), 0, 2, S[0:60], S[60:100], "62M", "40M", (1, 0), (0, 0, 0, 0), (2, 3)),      # 1061 - 2; MinusCigarRight makes 60M of it
            row((0, 1059, "+", 0, 5039, "-"), 4, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0), (4, 5))]
    return dict(name="worked", records=records, rows=rows, counts=counts(6, 3, 3, 3))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. all six kinds: the source record of the seqs hard-clipped (borrowed; kinds 0, 1 on the same strand, 2-5 on opposite strands), and both soft-clipped
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _kind_pairs(hard):
    """(records of the six names, rows without their record indices).  hard: the record the case analysis takes the seqs from is hard-clipped"""
    def clip(cigar, stored):
        """the soft-clipped record as it is, or its hard-clipped form: S -> H, and only the aligned bases in SEQ"""
        if not hard:
            return cigar, stored
        (l1, o1), (l2, o2) = RM.parse_cigar_text(cigar)
        return (f"{l1}H{l2}M", stored[l1:]) if o1 == "S" else (f"{l1}M{l2}H", stored[:l1])
    records, rows = [], []
    # kind 0: same strand, up (3' clipped) left 60 >= down (5' clipped) left 60; the seqs are the down record's
    c, s = clip("60S40M", S)
    records += [rec("k0", 0, 999, "60M40S", S), rec("k0", SUPP, 4999, c, s)]
    rows.append(((0, 1059, "+", 0, 5000, "+"), 0, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0)))
    # kind 1: up left 55 < down left 60: the up CIGAR gets 5 right-clipped bases
    records += [rec("k1", 0, 999, "55M45S", S), rec("k1", SUPP, 4999, c, s)]
    rows.append(((0, 1054, "+", 0, 5000, "+"), 1, 0, S[0:60], S[60:100], "55M", "40M", (0, 0), (0, 5, 0, 0)))
    # kind 2: opposite strands, both 5' clipped, up (the lower position) right 60 >= down left 60; the seqs are the up record's, reverse-complemented
    c, s = clip("40S60M", S)
    records += [rec("k2", 0, 1999, c, s), rec("k2", SUPP | REV, 6999, "60S40M", RC)]
    rows.append(((0, 2000, "-", 0, 7000, "+"), 2, 0, rc(S[40:100]), rc(S[0:40]), "60M", "40M", (0, 2), (0, 0, 0, 0)))
    # kind 3: up right 60 < down left 70; the seqs are the down record's as stored
    c, s = clip("70S30M", RC)
    records += [rec("k3", 0, 1999, "40S60M", S), rec("k3", SUPP | REV, 6999, c, s)]
    rows.append(((0, 2000, "-", 0, 7000, "+"), 3, 0, RC[0:70], RC[70:100], "60M", "30M", (0, 0), (0, 10, 0, 0)))
    # kind 4: opposite strands, both 3' clipped, up left 60 >= down right 60; the seqs are the down record's, reverse-complemented
    c, s = clip("40M60S", RC)
    records += [rec("k4", 0, 999, "60M40S", S), rec("k4", SUPP | REV, 4999, c, s)]
    rows.append(((0, 1059, "+", 0, 5039, "-"), 4, 0, rc(RC[40:100]), rc(RC[0:40]), "60M", "40M", (1, 0), (0, 0, 0, 0)))
    # kind 5: up left 50 < down right 60; the seqs are the up record's as stored
    c, s = clip("50M50S", S)
    records += [rec("k5", 0, 999, c, s), rec("k5", SUPP | REV, 4999, "40M60S", RC)]
    rows.append(((0, 1049, "+", 0, 5039, "-"), 5, 0, S[0:50], S[50:100], "50M", "40M", (0, 0), (0, 0, 10, 0)))
    return records, [row(*r, (2 * k, 2 * k + 1)) for k, r in enumerate(rows)]


def kinds_hard():
    records, rows = _kind_pairs(True)
    return dict(name="kinds_hard", records=records, rows=rows, counts=counts(12, 6, 6, 6))


def kinds_soft():
    records, rows = _kind_pairs(False)
    return dict(name="kinds_soft", records=records, rows=rows, counts=counts(12, 0, 6, 0))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. microhomology 1 and 25 in the three >= branches (0 is in set 2), and the three < branches missed by one
# ---------------------------------------------------------------------------------------------------------------------------------------------
def microhomology():
    records, rows = [], []

    def add(name, a, b, r):
        records.extend([a, b])
        rows.append(row(*r, (len(records) - 2, len(records) - 1)))
    for mh in (1, 25):
        L = 60 + mh
        add(f"m0_{mh}", rec(f"m0_{mh}", 0, 999, f"{L}M{100 - L}S", S), rec(f"m0_{mh}", SUPP, 4999, "60S40M", S),
            ((0, 1059, "+", 0, 5000, "+"), 0, mh, S[0:60], S[60:100], f"{L}M", "40M", (1, 0), (0, 0, 0, 0)))           # up pos 999 + L, minus mh
        add(f"m2_{mh}", rec(f"m2_{mh}", 0, 1999, f"{100 - L}S{L}M", S), rec(f"m2_{mh}", SUPP | REV, 6999, "60S40M", RC),
            ((0, 2000, "-", 0, 7000 + mh, "+"), 2, mh, rc(S[100 - L:100]), rc(S[0:100 - L]), f"{L}M", "40M", (0, 2), (0, 0, 0, 0)))
        add(f"m4_{mh}", rec(f"m4_{mh}", 0, 999, f"{L}M{100 - L}S", S), rec(f"m4_{mh}", SUPP | REV, 4999, "40M60S", RC),
            ((0, 1059, "+", 0, 5039, "-"), 4, mh, rc(RC[40:100]), rc(RC[0:40]), f"{L}M", "40M", (1, 0), (0, 0, 0, 0)))
    add("m1", rec("m1", 0, 999, "59M41S", S), rec("m1", SUPP, 4999, "60S40M", S),
        ((0, 1058, "+", 0, 5000, "+"), 1, 0, S[0:60], S[60:100], "59M", "40M", (0, 0), (0, 1, 0, 0)))
    add("m3", rec("m3", 0, 1999, "41S59M", S), rec("m3", SUPP | REV, 6999, "60S40M", RC),
        ((0, 2000, "-", 0, 7000, "+"), 3, 0, RC[0:60], RC[60:100], "59M", "40M", (0, 0), (0, 1, 0, 0)))
    add("m5", rec("m5", 0, 999, "59M41S", S), rec("m5", SUPP | REV, 4999, "40M60S", RC),
        ((0, 1058, "+", 0, 5039, "-"), 5, 0, S[0:59], S[59:100], "59M", "40M", (0, 0), (0, 0, 1, 0)))
    return dict(name="microhomology", records=records, rows=rows, counts=counts(18, 0, 9, 0))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. both records hard-clipped: no pair, the held one stays, a third record pairs with it      5. R_A != R_B: dropped
# ---------------------------------------------------------------------------------------------------------------------------------------------
def both_hard():
    records = [rec("hh", SUPP, 4999, "60H40M", S[60:]), rec("hh", SUPP, 999, "60M40H", S[:60]), rec("hh", 0, 999, "60M40S", S)]
    rows = [row((0, 1059, "+", 0, 5000, "+"), 0, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0), (0, 2))]
    return dict(name="both_hard", records=records, rows=rows, counts=counts(3, 2, 1, 1, dropped_no_carrier=1))


def unequal_lengths():
    records = [rec("ul", 0, 999, "60M40S", S), rec("ul", SUPP, 4999, "50S40M", S[10:])]
    return dict(name="unequal_lengths", records=records, rows=[], counts=counts(2, 0, 0, 0, dropped_length=1))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. one paired-end name, read 1 and read 2 each split, interleaved: two pairs, none across mates (by the name alone the first pair would be read 1's
#    primary with read 2's supplementary)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def mates():
    records = [rec("pe", READ1, 999, "60M40S", S), rec("pe", READ2 | SUPP, 8999, "70H30M", S2[70:]),
               rec("pe", READ1 | SUPP, 4999, "60H40M", S[60:]), rec("pe", READ2, 2999, "70M30S", S2)]
    rows = [row((0, 1059, "+", 0, 5000, "+"), 0, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0), (0, 2)),
            row((0, 3069, "+", 0, 9000, "+"), 0, 0, S2[0:70], S2[70:100], "70M", "30M", (1, 0), (0, 0, 0, 0), (1, 3))]
    by_name_only = [(0, 1), (2, 3)]    # records of the pairs that the name alone gives: read 1's primary with read 2's supplementary, and the other two
    return dict(name="mates", records=records, rows=rows, counts=counts(4, 2, 2, 2), by_name_only=by_name_only)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7. names of 1 and 254 bytes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def name_lengths():
    long_name = ("n254." + "abcdefghij" * 25)[:254]
    assert len(long_name) == 254
    sibling = long_name[:-1] + "X"     # differs in its last byte: another key
    records = [rec("x", 0, 999, "60M40S", S), rec(long_name, 0, 999, "60M40S", S), rec(sibling, 0, 999, "60M40S", S),
               rec(long_name, SUPP, 4999, "60H40M", S[60:]), rec("x", SUPP, 4999, "60H40M", S[60:])]
    r = ((0, 1059, "+", 0, 5000, "+"), 0, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0))
    return dict(name="name_lengths", records=records, rows=[row(*r, (1, 3)), row(*r, (0, 4))], counts=counts(5, 2, 2, 2))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 8. records that take no part: each would complete a pair with the good record of its name
# ---------------------------------------------------------------------------------------------------------------------------------------------
def not_taken():
    bad = [("sec", dict(flag=SUPP | SECONDARY)), ("dup", dict(flag=SUPP | DUP)), ("unm", dict(flag=SUPP | UNMAP)), ("mq0", dict(mapq=0)),
           ("tid", dict(tid=len(CONTIGS), host_only=True)), ("noc", dict(cigar="")), ("ss", dict(cigar="50S40M10S")), ("hs", dict(cigar="50H40M10S", seq=S[50:])),
           ("mm", dict(cigar="100M")), ("im", dict(cigar="10I90M")), ("eq", dict(cigar="100="))]
    records = []
    for name, change in bad:
        records.append(rec(name, 0, 999, "60M40S", S))
        records.append(dict(rec(name, SUPP, 4999, "60S40M", S), **change))
    return dict(name="not_taken", records=records, rows=[], counts=counts(len(bad), 0, 0, 0), file_counts=counts(len(bad) - 1, 0, 0, 0))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 9. 5H10S85M: the clip is the run of S / H, 15
# ---------------------------------------------------------------------------------------------------------------------------------------------
def clip_run():
    records = [rec("run", 0, 999, "85M15S", S), rec("run", SUPP, 4999, "5H10S85M", S[5:]),
               rec("run3", 0, 4999, "15S85M", S), rec("run3", SUPP, 999, "85M10S5H", S[:95])]
    rows = [row((0, 1014, "+", 0, 5000, "+"), 0, 70, S[0:15], S[15:100], "85M", "85M", (1, 0), (0, 0, 0, 0), (0, 1)),     # 999 + 85 - 70
            row((0, 1014, "+", 0, 5000, "+"), 0, 70, S[0:15], S[15:100], "85M", "85M", (1, 0), (0, 0, 0, 0), (2, 3))]     # the same, the 3' run hard-clipped: not borrowed
    return dict(name="clip_run", records=records, rows=rows, counts=counts(4, 2, 2, 1))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 10. R of 1, 2, 63, 64, 65, 129 and 77: kind 2 (both seqs reverse-complemented), the up record's clip odd where R allows, once soft-clipped (read with rc from
#     an odd offset) and once hard-clipped (borrowed: read from the '-' record, the down seq from offset R - a)
# ---------------------------------------------------------------------------------------------------------------------------------------------
LENGTHS = (2, 63, 64, 65, 129, 77)


def read_lengths():
    records, rows = [], []
    for R in LENGTHS:
        read = LONG[:R]
        a = 1 if R < 6 else (R // 3) | 1      # the up record's clip: odd
        b = R - a                             # ... and its aligned part, the microhomology's side
        c = b - 1 if b > 1 else b             # the down record's clip: microhomology 1 (0 for R == 2)
        mh = b - c
        for form in ("s", "h"):
            name = f"len{R}{form}"
            up = rec(name, 0, 1999, f"{a}S{b}M", read) if form == "s" else rec(name, SUPP, 1999, f"{a}H{b}M", read[a:])
            records += [up, rec(name, REV, 6999, f"{c}S{R - c}M", rc(read))]
            rows.append(row((0, 2000, "-", 0, 7000 + mh, "+"), 2, mh, rc(read[a:R]), rc(read[0:a]), f"{b}M", f"{R - c}M", (0, 2), (0, 0, 0, 0),
                            (len(records) - 2, len(records) - 1)))
    # R == 1: a clip of one base and an operation that holds none (1S1D / 1D1S).  Same strand, up left 0 < down left 1: kind 1, an empty down seq
    records += [rec("len1", 0, 999, "1D1S", "G", host_only=True), rec("len1", SUPP, 4999, "1H1D", "", host_only=True)]
    rows.append(row((0, 1000, "+", 0, 5000, "+"), 1, 0, "G", "", "1D", "1D", (0, 0), (0, 1, 0, 0), (len(records) - 2, len(records) - 1)))
    n = len(LENGTHS)
    return dict(name="read_lengths", records=records, rows=rows, counts=counts(4 * n + 2, n + 1, 2 * n + 1, n + 1), file_counts=counts(4 * n, n, 2 * n, n))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 11. forty keys, all primaries first: with the hash cut to 4 bits (SSV_RT_HASH_BITS=4) every run of equal hashes holds several keys
# ---------------------------------------------------------------------------------------------------------------------------------------------
N_COLLIDING = 40


def colliding():
    records = [rec(f"c{k}", 0, 999 + k, "60M40S", S) for k in range(N_COLLIDING)]
    order = [(7 * k) % N_COLLIDING for k in range(N_COLLIDING)]            # the supplementaries in another order
    records += [rec(f"c{k}", SUPP, 4999 + 10 * k, "60H40M", S[60:]) for k in order]
    rows = [row((0, 1059 + k, "+", 0, 5000 + 10 * k, "+"), 0, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0), (k, N_COLLIDING + j)) for j, k in enumerate(order)]
    return dict(name="colliding", records=records, rows=rows, counts=counts(2 * N_COLLIDING, N_COLLIDING, N_COLLIDING, N_COLLIDING))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 12. one key, five candidates: hold, drop (same strand and side), pair, hold anew, pair on opposite strands with the completing record up
# ---------------------------------------------------------------------------------------------------------------------------------------------
def five():
    records = [rec("five", 0, 999, "60M40S", S), rec("five", SUPP, 1999, "70M30S", S), rec("five", SUPP, 4999, "60S40M", S),
               rec("five", SUPP | REV, 6999, "40S60M", RC), rec("five", SUPP, 1999, "50S50M", S)]
    rows = [row((0, 1059, "+", 0, 5000, "+"), 0, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0), (0, 2)),
            row((0, 2000, "-", 0, 7010, "+"), 2, 10, rc(S[50:100]), rc(S[0:50]), "50M", "60M", (0, 2), (0, 0, 0, 0), (3, 4))]
    return dict(name="five", records=records, rows=rows, counts=counts(5, 0, 2, 0))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 13. a soft-clipped record that does not carry the read: no SEQ (l_qseq 0 != R), and - a host batch only - SSV_NO_SEQ with l_qseq == R
# ---------------------------------------------------------------------------------------------------------------------------------------------
def no_bases():
    records = [rec("nb1", SUPP, 4999, "60S40M", ""), rec("nb1", 0, 999, "60M40S", S),          # the source of the seqs has no SEQ: borrowed
               rec("nb2", SUPP, 4999, "60S40M", ""), rec("nb2", 0, 999, "60M40S", ""),         # neither has
               rec("nb3", SUPP, 4999, "60S40M", S, no_seq=True, host_only=True), rec("nb3", 0, 999, "60M40S", S, host_only=True)]
    r = ((0, 1059, "+", 0, 5000, "+"), 0, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0))
    return dict(name="no_bases", records=records, rows=[row(*r, (0, 1)), row(*r, (4, 5))], counts=counts(6, 0, 2, 2, dropped_no_carrier=1),
                file_counts=counts(4, 0, 1, 1, dropped_no_carrier=1))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# two contigs: the up record of an opposite-strand pair is the one on the contig whose NAME is smaller ("chrA", tid 1)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def two_contigs():
    records = [rec("tc", 0, 999, "60M40S", S, tid=0), rec("tc", SUPP | REV, 4999, "40M60H", RC[:40], tid=1)]
    # up: the '-' record on chrA - left 40 < the down record's right 40?  no: 40 >= 40, kind 4, microhomology 0; the seqs are the down record's (chrB, '+'), rc
    rows = [row((1, 5039, "+", 0, 1059, "-"), 4, 0, rc(S[60:100]), rc(S[0:60]), "40M", "60M", (1, 0), (0, 0, 0, 0), (0, 1))]
    return dict(name="two_contigs", records=records, rows=rows, counts=counts(2, 1, 1, 0))


SETS = (worked, kinds_hard, kinds_soft, microhomology, both_hard, unequal_lengths, mates, name_lengths, not_taken, clip_run, read_lengths, colliding, five,
        no_bases, two_contigs)


def all_sets():
    return [f() for f in SETS]


def file_records(s):
    """the records of a set that a BAM or SAM text can hold"""
    return [r for r in s["records"] if not r.get("host_only")]


def file_set(s):
    """the set as a file holds it: (records, rows) with the host-only names gone (every name of a set stands alone) and the rows' record indices moved; its
    counts are s.get("file_counts", s["counts"])"""
    gone = {r["qname"] for r in s["records"] if r.get("host_only")}
    keep = [k for k, r in enumerate(s["records"]) if r["qname"] not in gone]
    at = {k: j for j, k in enumerate(keep)}
    rows = [dict(r, records=(at[r["records"][0]], at[r["records"][1]])) for r in s["rows"] if r["records"][0] in at]
    return [s["records"][k] for k in keep], rows


def batch_of(records):
    """records -> (batch as readthrough_model and Context take it, names): the decoders' default form in outline - every record's bases are there unless it says
    no_seq or has no SEQ"""
    b, names = RM.batch_from_records([dict(r, cigar=r["cigar"] or []) for r in records])
    so = b["seq_off"].copy()
    for k, r in enumerate(records):
        if r.get("no_seq") or not r["seq"]:
            so[k] = RM.NO_SEQ
    b["seq_off"] = so
    return b, names


def combined(file_form=False):
    """all sets in one input, every name prefixed by its set's: (records, rows, counts).  file_form: what a BAM or SAM text can hold of them (file_set)"""
    records, rows, total = [], [], dict.fromkeys(COUNT_KEYS, 0)
    for s in all_sets():
        base = len(records)
        set_records, set_rows = file_set(s) if file_form else (s["records"], s["rows"])
        records += [dict(r, qname=s["name"] + "." + r["qname"] if len(r["qname"]) < 200 else r["qname"]) for r in set_records]  # (the 254-byte names stay)
        rows += [dict(r, records=(r["records"][0] + base, r["records"][1] + base)) for r in set_rows]
        for k in COUNT_KEYS:
            total[k] += (s.get("file_counts", s["counts"]) if file_form else s["counts"])[k]
    rows.sort(key=lambda r: r["records"][1])
    return records, rows, total


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the agreement set: single-end, M I D S only, every record one-side soft-clipped or M..M, no 0x100 - where the rule and FindJunction say the same
# ---------------------------------------------------------------------------------------------------------------------------------------------
def agreement(seed=0, n_names=150):
    rng = np.random.RandomState(4200 + seed)
    records = []
    groups = []
    for k in range(n_names):
        R = int(rng.choice([30, 76, 100, 101, 150]))
        read = _bases(R, 9000 + 100 * seed + k)
        group = []
        for _ in range(int(rng.choice([1, 2, 2, 2, 3, 4]))):
            strand = "-" if rng.rand() < 0.5 else "+"
            stored = rc(read) if strand == "-" else read
            shape = rng.rand()
            if shape < 0.12:
                cigar = f"{R}M"                                               # M..M: neither rule takes it
            else:
                clip = int(rng.randint(1, R - 1))
                body = R - clip
                parts = f"{body}M"
                if body >= 8 and rng.rand() < 0.4:                            # an insertion and a deletion inside
                    x = int(rng.randint(2, body - 4))
                    i = int(rng.randint(1, min(4, body - x - 1) + 1))
                    parts = f"{x}M{i}I{int(rng.randint(1, 9))}D{body - x - i}M"
                cigar = f"{clip}S{parts}" if shape < 0.56 else f"{parts}{clip}S"
            flag = (REV if strand == "-" else 0) | (SUPP if group else 0)
            r = rec(f"ag{k}", flag, int(rng.randint(500, 18000)), cigar, stored, tid=int(rng.randint(0, 2)), mapq=int(rng.choice([60, 60, 60, 30, 1, 0])))
            if rng.rand() < 0.05:
                r["flag"] |= int(rng.choice([UNMAP, DUP]))
            group.append(r)
        groups.append(group)
    # input order: the records of a name keep their order, the names interleave
    keyed = []
    for g in groups:
        t = np.sort(rng.rand(len(g)))
        keyed += list(zip(t.tolist(), g))
    order = sorted(range(len(keyed)), key=lambda j: (keyed[j][0], j))
    records = [keyed[j][1] for j in order]
    return dict(name=f"agreement{seed}", records=records)


def filler(n, seed=0):
    """M..M records of names of their own (no rule takes them): what lies between the split reads of a coordinate-sorted file"""
    rng = np.random.RandomState(4300 + seed)
    return [rec(f"fill{k}", int(rng.choice([0, REV])), int(rng.randint(500, 18000)), "100M", _bases(100, 9500 + k), tid=int(rng.randint(0, 2))) for k in range(n)]


def coordinate_sorted(records):
    """a stable sort by (tid, pos), as a coordinate-sorted file has them"""
    return sorted(records, key=lambda r: (r["tid"], r["pos"]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the sample of the command-line tests: paired-end fragments whose read 1 is split with the source of its seqs hard-clipped (the six kinds in turn, every
# fragment at positions of its own, 150 apart: no two junctions within getsv's merge distance), read 2 an unclipped mate or - every fourth - split as well
# ---------------------------------------------------------------------------------------------------------------------------------------------
N_FRAGMENTS = 36


def cli_sample():
    hard, _ = _kind_pairs(True)
    records = []
    for k in range(N_FRAGMENTS):
        name = f"frag{k}"
        for r in hard[2 * (k % 6):2 * (k % 6) + 2]:
            records.append(dict(r, qname=name, flag=r["flag"] | READ1, pos=r["pos"] + 150 * k))
        if k % 4 == 1:
            j = (k + 3) % 6
            for r in hard[2 * j:2 * j + 2]:
                records.append(dict(r, qname=name, flag=r["flag"] | READ2, pos=r["pos"] + 150 * (k + N_FRAGMENTS)))
        else:
            records.append(rec(name, READ2 | REV, 15000 + 20 * k, "100M", _bases(100, 9700 + k)))
    return records + filler(60, 7)


def shuffled(records, seed=5):
    order = np.random.RandomState(seed).permutation(len(records))
    return [records[k] for k in order]


def reference_fasta(seed=11):
    rng = np.random.RandomState(seed)
    text = ""
    for name, n in zip(CONTIGS, LENS):
        c = "".join("ACGT"[k] for k in rng.randint(0, 4, n))
        text += f">{name}\n" + "\n".join(c[i:i + 70] for i in range(0, n, 70)) + "\n"
    return text
