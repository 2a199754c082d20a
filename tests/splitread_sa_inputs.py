"""Hand-made inputs for `seeksv run -A -S` (tests/splitread_sa_model.py), one rule per set, with the expected pairs and counts WRITTEN OUT: every set is
dict(name, records, rows, counts, sa_counts[, encodings]) in the form of tests/splitread_inputs.py (imported, not edited: its reads, its rec() and the
rows of its six kinds).  A record's optional fields come in both encodings: `aux` (BAM's typed fields, the bytes tests/bamio.py appends to the record) and
`tags` (SAM text fields, which tests/sam_text.py appends to the line); tagged() makes both from one SA value.  A set that is about one walker names it in
`encodings`.  Nothing here calls the model.

Contigs: tid 0 "chrB", tid 1 "chrA" (as in splitread_inputs), tid 2 "chrA_alt" (tid 1's name is its prefix), tid 3 "chr;C:*"."""
import struct

import splitread_inputs as SI

CONTIGS = ["chrB", "chrA", "chrA_alt", "chr;C:*"]
LENS = [20000, 20000, 20000, 20000]
BAM, SAM = 0, 1
S, RC, S2, rc, rec = SI.S, SI.RC, SI.S2, SI.rc, SI.rec
SUPP, REV, READ1, READ2, DUP = SI.SUPP, SI.REV, SI.READ1, SI.READ2, SI.DUP
SA_KEYS = ("sa_tags", "sa_multi", "sa_refused", "virtuals", "sa_redundant", "pairs_from_sa", "sa_dropped_length")


def row(key, kind, mh, up_seq, down_seq, up_cigar, down_cigar, edits, clipped, records):
    up, down = key[:3], key[3:]
    return dict(key=(CONTIGS[up[0]], up[1], up[2], CONTIGS[down[0]], down[1], down[2]), kind=kind, microhomology=mh, up_seq=up_seq, down_seq=down_seq,
                up_cigar=SI.ops(up_cigar), down_cigar=SI.ops(down_cigar), edits=edits, clipped=clipped, records=records)


def sa_counts(sa_tags=0, sa_multi=0, sa_refused=0, virtuals=0, sa_redundant=0, pairs_from_sa=0, sa_dropped_length=0):
    return dict(sa_tags=sa_tags, sa_multi=sa_multi, sa_refused=sa_refused, virtuals=virtuals, sa_redundant=sa_redundant, pairs_from_sa=pairs_from_sa,
                sa_dropped_length=sa_dropped_length)


def tagged(r, sa, nm=0):
    """the record with NM and the SA value `sa` (str) in both encodings"""
    return dict(r, aux=b"NMC" + bytes([nm]) + b"SAZ" + sa.encode() + b"\0", tags=[f"NM:i:{nm}", "SA:Z:" + sa])


def entry_of(r):
    """the SA entry an aligner writes for record r: H becomes S"""
    return f"{CONTIGS[r['tid']]},{r['pos'] + 1},{'-' if r['flag'] & REV else '+'},{r['cigar'].replace('H', 'S')},{r['mapq']},0;"


def bam_area(r):
    return r.get("aux", b"")


def sam_area(r):
    return "\t".join(r.get("tags", [])).encode("latin-1")


def areas(records, enc):
    return [sam_area(r) if enc == SAM else bam_area(r) for r in records]


# the row of the read most sets use: 60M40S at chrB:1000 whose other piece is 60S40M on the same strand at position 5000 of contig `tid`
def _w(tid, at):
    return row((0, 1059, "+", tid, 5000, "+"), 0, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0), (at, at))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. slice: the six kinds of splitread_inputs with the second record of every pair absent and named by the first one's SA; the rows are that file's
# ---------------------------------------------------------------------------------------------------------------------------------------------
def kinds_complete():
    """every primary has its supplementary: phase 1's pairs stand, every virtual candidate is redundant"""
    records, rows = SI._kind_pairs(False)
    for k in range(0, len(records), 2):
        records[k] = tagged(records[k], entry_of(records[k + 1]))
    return dict(name="kinds_complete", records=records, rows=rows, counts=SI.counts(12, 0, 6, 0), sa_counts=sa_counts(sa_tags=6, virtuals=6, sa_redundant=6))


def kinds_slice():
    """the same with the supplementary records removed: the same junctions, from the SA entries; both strands, both sides"""
    full = kinds_complete()
    records = full["records"][0::2]
    rows = [dict(r, records=(k, k)) for k, r in enumerate(full["rows"])]
    # (borrowed: the four kinds whose seqs the case analysis takes from the absent record - 0, 1, 3, 4; kinds 2 and 5 take them from the source)
    return dict(name="kinds_slice", records=records, rows=rows, counts=SI.counts(6, 0, 6, 4), sa_counts=sa_counts(sa_tags=6, virtuals=6, pairs_from_sa=6))


def other_contig():
    """the partner lies on another contig and is absent; read 1 and read 2 of one name each with its own SA; a single-end read"""
    records = [tagged(rec("oc", READ1, 999, "60M40S", S), "chrA_alt,5000,+,60S40M,60,0;"),
               tagged(rec("oc", READ2, 999, "60M40S", S), "chrA,5000,+,60S40M,60,1;"),
               tagged(rec("single", 0, 999, "60M40S", S), "chr;C:*,5000,+,60S40M,60,0;"),
               rec("plain", 0, 999, "60M40S", S)]
    return dict(name="other_contig", records=records, rows=[_w(2, 0), _w(1, 1), _w(3, 2)], counts=SI.counts(4, 0, 3, 3),
                sa_counts=sa_counts(sa_tags=3, virtuals=3, pairs_from_sa=3))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. the real partner wins; a partner that is refused (0x400, MAPQ 0) leaves the SA entry to fill in; a hard-clipped record is no source
# ---------------------------------------------------------------------------------------------------------------------------------------------
def real_partner():
    sa = "chrB,5000,+,60S40M,60,0;"
    records = [tagged(rec("real", 0, 999, "60M40S", S), sa), rec("real", SUPP, 4999, "60H40M", S[60:]),           # pairs in phase 1 (borrowed: the partner has H)
               tagged(rec("late", 0, 999, "60M40S", S), sa),                                                      # its supplementary comes last
               tagged(rec("dup", 0, 999, "60M40S", S), sa), rec("dup", SUPP | DUP, 4999, "60H40M", S[60:]),
               tagged(rec("low", 0, 999, "60M40S", S), sa), rec("low", SUPP, 4999, "60H40M", S[60:], mapq=0),
               tagged(rec("hsrc", SUPP, 4999, "60H40M", S[60:]), "chrB,1000,+,60M40S,60,0;"),                      # hard-clipped: never a source, its fields are not read
               rec("late", SUPP, 4999, "60H40M", S[60:])]
    w = row((0, 1059, "+", 0, 5000, "+"), 0, 0, S[0:60], S[60:100], "60M", "40M", (1, 0), (0, 0, 0, 0), None)
    rows = [dict(w, records=(0, 1)), dict(w, records=(3, 3)), dict(w, records=(5, 5)), dict(w, records=(2, 8))]
    return dict(name="real_partner", records=records, rows=rows, counts=SI.counts(7, 3, 4, 4),
                sa_counts=sa_counts(sa_tags=4, virtuals=4, sa_redundant=2, pairs_from_sa=2))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. the grammar: one source per case
# ---------------------------------------------------------------------------------------------------------------------------------------------
GRAMMAR = [  # (name, SA value, "ok" with the partner's tid | "multi" | "refused" | "length")
    ("two_entries", "chrB,5000,+,60S40M,60,0;chrA,100,+,60S40M,60,0;", "multi"),
    ("trailing_byte", "chrB,5000,+,60S40M,60,0;;", "multi"),
    ("no_semicolon", "chrB,5000,+,60S40M,60,0", 0),
    ("empty", "", "refused"),
    ("missing_field", "chrB,5000,+,60S40M,60;", "refused"),
    ("empty_nm", "chrB,5000,+,60S40M,60,;", "refused"),
    ("pos_0", "chrB,0,+,60S40M,60,0;", "refused"),
    ("pos_2_31", "chrB,2147483648,+,60S40M,60,0;", "refused"),
    ("pos_signed", "chrB,+5000,+,60S40M,60,0;", "refused"),
    ("strand_star", "chrB,5000,*,60S40M,60,0;", "refused"),
    ("bad_letter", "chrB,5000,+,60S40Q,60,0;", "refused"),
    ("no_length", "chrB,5000,+,60SM,60,0;", "refused"),
    ("star_cigar", "chrB,5000,+,*,60,0;", "refused"),
    ("long_op", "chrB,5000,+,268435456S40M,60,0;", "refused"),
    ("both_ends", "chrB,5000,+,30S40M30S,60,0;", "refused"),
    ("no_end", "chrB,5000,+,100M,60,0;", "refused"),
    ("mapq_256", "chrB,5000,+,60S40M,256,0;", "refused"),
    ("mapq_floor", "chrB,5000,+,60S40M,0,0;", "refused"),
    ("unknown_contig", "chrZ,5000,+,60S40M,60,0;", "refused"),
    ("prefix_short", "chrA,5000,+,60S40M,60,0;", 1),
    ("prefix_long", "chrA_alt,5000,+,60S40M,60,0;", 2),
    ("prefix_cut", "chrA_al,5000,+,60S40M,60,0;", "refused"),
    ("semicolon_name", "chr;C:*,5000,+,60S40M,60,0;", 3),
    ("hard_in_sa", "chrB,5000,+,50H10S40M,60,12;", 0),
    ("r_unequal", "chrB,5000,+,50S40M,60,0;", "length"),
]


def grammar():
    records = [tagged(rec(name, 0, 999, "60M40S", S), sa) for name, sa, _ in GRAMMAR]
    rows = [_w(want, k) for k, (_, _, want) in enumerate(GRAMMAR) if isinstance(want, int)]
    return dict(name="grammar", records=records, rows=rows, counts=SI.counts(25, 0, 5, 5),
                sa_counts=sa_counts(sa_tags=25, sa_multi=2, sa_refused=17, virtuals=6, pairs_from_sa=5, sa_dropped_length=1))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. the BAM walk      5. the SAM walk
# ---------------------------------------------------------------------------------------------------------------------------------------------
_SA = b"SAZchrB,5000,+,60S40M,60,0;\0"
_B = lambda sub, fmt, vals: b"XB" + b"B" + sub + struct.pack("<I", len(vals)) + b"".join(struct.pack(fmt, v) for v in vals)  # noqa: E731
BAM_WALK = [  # (name, the optional-field area, found?)
    ("first", _SA + b"NMC\x01", True),
    ("last", b"NMC\x01ASS\x10\x00" + _SA, True),
    ("behind_A", b"XAAq" + _SA, True), ("behind_c", b"Xcc\xff" + _SA, True), ("behind_C", b"XCC\x00" + _SA, True),
    ("behind_s", b"Xss\xff\xff" + _SA, True), ("behind_S", b"XSS\x01\x02" + _SA, True), ("behind_i", b"Xii\x00\x00\x00\x80" + _SA, True),
    ("behind_I", b"XII\xff\xff\xff\xff" + _SA, True), ("behind_f", b"Xff\x00\x00\x80\x3f" + _SA, True), ("behind_d", b"Xdd" + bytes(8) + _SA, True),
    ("behind_Z", b"XZZtext\0" + _SA, True), ("behind_H", b"XHH1AE3\0" + _SA, True),
    ("behind_Bc", _B(b"c", "<b", [1, -2, 3]) + _SA, True), ("behind_BC", _B(b"C", "<B", [1, 2, 3]) + _SA, True),
    ("behind_Bs", _B(b"s", "<h", [1, -2, 3]) + _SA, True), ("behind_BS", _B(b"S", "<H", [1, 2, 3]) + _SA, True),
    ("behind_Bi", _B(b"i", "<i", [1, -2, 3]) + _SA, True), ("behind_BI", _B(b"I", "<I", [1, 2, 3]) + _SA, True),
    ("behind_Bf", _B(b"f", "<f", [1.0, 2.0]) + _SA, True), ("behind_B_empty", _B(b"c", "<b", []) + _SA, True),
    ("type_A_first", b"SAAx" + _SA, True), ("type_i_first", b"SAi\x05\x00\x00\x00" + _SA, True),
    ("bytes_in_Z", b"XZZSAZchrA,1,+,60S40M,60,0;\0" + b"NMC\x00", False),
    ("bytes_in_Z_then_SA", b"XZZSAZchrA,1,+,60S40M,60,0;\0" + _SA, True),
    ("unknown_type", b"XQQ\x00" + _SA, False),
    ("none", b"NMC\x00", False), ("empty_area", b"", False), ("two_bytes", b"SA", False),
    ("truncated_fixed", b"Xii\x00\x00", False),
    ("overlong_B", b"XBBi\xff\xff\xff\x3f" + _SA, False),
    ("huge_B_count", b"XBBi\xff\xff\xff\xff" + _SA, False),
    ("truncated_Z", b"NMC\x00SAZchrB,5000,+,60S40M,60,0;", False),       # (no NUL: the LAST record of the set - and of a BAM file's batch)
]


def bam_walk():
    records = [dict(rec(name, 0, 999, "60M40S", S), aux=aux) for name, aux, _ in BAM_WALK]
    rows = [_w(0, k) for k, (_, _, found) in enumerate(BAM_WALK) if found]
    return dict(name="bam_walk", records=records, rows=rows, counts=SI.counts(33, 0, 24, 24), sa_counts=sa_counts(sa_tags=24, virtuals=24, pairs_from_sa=24),
                encodings=(BAM,))


_T = "SA:Z:chrB,5000,+,60S40M,60,0;"
SAM_WALK = [  # (name, the text from field 12 on as the host descriptor gives it, found?)
    ("field_12", [_T, "NM:i:1"], True),
    ("last_field", ["NM:i:1", "AS:i:77", _T], True),
    ("only_field", [_T], True),
    ("inside_XA", ["XA:Z:chrA,+1,60S40M,0;SA:Z:chrA,1,+,60S40M,60,0;", "NM:i:0"], False),
    ("inside_XA_then_SA", ["XA:Z:SA:Z:chrA,1,+,60S40M,60,0;", _T], True),
    ("SA_i", ["SA:i:5", "NM:i:0"], False),
    ("SA_i_then_Z", ["SA:i:5", _T], True),
    ("lower_case", ["sa:Z:chrB,5000,+,60S40M,60,0;"], False),
    ("short_field", ["SA:Z", "NM:i:0"], False),
    ("eleven_fields", [], False),
]


def sam_walk():
    records = [dict(rec(name, 0, 999, "60M40S", S), tags=tags) for name, tags, _ in SAM_WALK]
    rows = [_w(0, k) for k, (_, _, found) in enumerate(SAM_WALK) if found]
    return dict(name="sam_walk", records=records, rows=rows, counts=SI.counts(10, 0, 5, 5), sa_counts=sa_counts(sa_tags=5, virtuals=5, pairs_from_sa=5),
                encodings=(SAM,))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. the one order-dependent case: an opposite-strand pair at equal (contig, position).  The completing record is up, and the virtual candidate
#    always completes - whatever the order of the two records in a complete file was.  Kept out of the sets that are compared with a complete file.
# ---------------------------------------------------------------------------------------------------------------------------------------------
def equal_position():
    records = [tagged(rec("eq", 0, 999, "60M40S", S), "chrB,1020,-,40M60S,60,0;")]                                 # both 3' clipped, both at 1059
    rows = [row((0, 1059, "+", 0, 1059, "-"), 4, 0, rc(S[60:100]), rc(S[0:60]), "40M", "60M", (1, 0), (0, 0, 0, 0), (0, 0))]
    return dict(name="equal_position", records=records, rows=rows, counts=SI.counts(1, 0, 1, 0), sa_counts=sa_counts(sa_tags=1, virtuals=1, pairs_from_sa=1))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the sample of the tests through the binary: splitread_inputs.cli_sample (paired-end fragments of the six kinds, the seqs' source record hard-clipped)
# as an aligner writes it - the record with H is the supplementary one, the record that carries the read names it in its SA tag
# ---------------------------------------------------------------------------------------------------------------------------------------------
def cli_sample():
    """-> (the complete sample, the same with the supplementary records removed); contigs: splitread_inputs.CONTIGS"""
    records = [dict(r) for r in SI.cli_sample()]
    by_key = {}
    for k, r in enumerate(records):
        if r["qname"].startswith("frag") and r["cigar"] != "100M":
            by_key.setdefault((r["qname"], r["flag"] & 0xC0), []).append(k)
    for a, b in by_key.values():                                                    # (every key of the sample has its two records)
        for src, other in ((a, b), (b, a)):
            if "H" in records[src]["cigar"]:
                records[src]["flag"] |= SUPP
            else:
                records[src] = tagged(dict(records[src], flag=records[src]["flag"] & ~SUPP), entry_of(records[other]))
    return records, [r for r in records if not r["flag"] & SUPP]


SETS = [kinds_complete, kinds_slice, other_contig, real_partner, grammar, bam_walk, sam_walk, equal_position]


def all_sets():
    return [f() for f in SETS]


def batch_of(records):
    return SI.batch_of(records)
