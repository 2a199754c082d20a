#!/usr/bin/env python3
"""Regenerate tests/golden/samdec/: forms.sam, one line per well-formed form of the SAM grammar the device decoder reads (include/seeksv_hip.h,
ssv_samdec_*), and forms.json, those lines as libbam 0.1.16's text reader decodes them (oracle/_ref/sam2bam, built by `make -C oracle ref`).
No '=' / 'X' CIGARs: libbam's text reader aborts on them.  CPU only.

usage: python tests/golden/make_samdec_reference.py"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sam_text as ST  # noqa: E402

SAM2BAM = os.path.join(ROOT, "oracle", "_ref", "sam2bam")
OUT = os.path.join(HERE, "samdec")
NAMES, LENS = ["chrA", "chrB", "HBV"], [40000, 15000, 3215]


def forms():
    """the record lines (bytes, without line ends) and the line end of each"""
    # every byte a SEQ field can hold: libbam splits fields at \t \n \v \f \r, the decoder refuses NUL, and for bytes of 128 and above libbam indexes its
    # base table with a negative number (whatever lies in front of the table: nothing to record)
    seq_bytes = bytes(b for b in range(1, 128) if b not in (9, 10, 11, 12, 13))
    t = lambda *f: "\t".join(str(x) for x in f).encode("latin-1")  # noqa: E731
    L = [
        t("all_seq_bytes", 0, "chrA", 101, 60, "*", "*", 0, 0) + b"\t" + seq_bytes + b"\t*",
        t("all_qual_bytes", 0, "chrA", 201, 60, "94M", "*", 0, 0, "ACGT" * 23 + "AC", "".join(chr(c) for c in range(33, 127))),
        t("stars", 4, "*", 0, 0, "*", "*", 0, 0, "*", "*"),
        t("mate_same", 99, "chrB", 1001, 37, "10M", "=", 1201, 210, "ACGTACGTAC", "IIIIIIIIII"),
        t("mate_same_neg", 147, "chrB", 1201, 37, "10M", "=", 1001, -210, "ACGTACGTAC", "*"),
        t("mate_other", 65, "chrA", 5001, 20, "4S6M", "HBV", 17, 0, "NNNNACGTAC", "#####IIIII"),
        t("unknown_rname", 0, "chrZ", 77, 60, "5M", "*", 0, 0, "ACGTA", "*"),
        t("unknown_rnext", 1, "chrA", 77, 60, "5M", "chrZ", 5, 0, "ACGTA", "*"),
        t("pos_zero", 0, "chrA", 0, 60, "5M", "=", 0, 0, "ACGTA", "*"),
        t("pad_op", 0, "HBV", 11, 255, "10M2P5I10M", "*", 0, 0, "A" * 25, "*"),
        t("all_ops", 16, "chrA", 301, 1, "3H5S10M2I3D4N10M1P6S2H", "*", 0, 0, "C" * 33, "*"),
        t("n" * 254, 0, "chrA", 401, 60, "5M", "*", 0, 0, "ACGTA", "*"),
        t("tags_xc0", 0, "chrA", 501, 60, "5M", "*", 0, 0, "ACGTA", "*", "NM:i:1", "XC:i:0", "MD:Z:5"),
        t("tags_xc7", 0, "chrA", 502, 60, "5M", "*", 0, 0, "ACGTA", "*", "XC:i:7", "AS:i:5"),
        t("tags_not_xc", 0, "chrA", 503, 60, "5M", "*", 0, 0, "ACGTA", "*", "XS:Z:XC:i:9", "XD:i:3"),
        t("hex_flag", "0x10", "chrA", 601, 60, "5M", "*", 0, 0, "ACGTA", "*"),
        t("hex_flag_big", "0xFFFF", "chrA", 602, 60, "5M", "*", 0, 0, "ACGTA", "*"),
        t("lower_dot", 0, "chrA", 701, 60, "12M", "*", 0, 0, "acgtn.ryKMsw", "*"),
        t("iupac", 0, "chrA", 702, 60, "16M", "*", 0, 0, "=ACMGRSVTWYHKDBN", "*"),
        t("digits", 0, "chrA", 703, 60, "5M", "*", 0, 0, "01234", "*"),
        t("odd_len", 0, "chrA", 704, 60, "7M", "*", 0, 0, "ACGTACG", "ABCDEFG"),
        t("seq_no_cigar", 0, "chrA", 705, 60, "*", "*", 0, 0, "ACGT", "IIII"),
        t("cigar_no_seq", 0, "chrA", 706, 60, "5M", "*", 0, 0, "*", "*"),
        t("big_numbers", 65535, "chrA", 2147483647, 255, "268435455M", "=", 2147483647, 2147483647, "*", "*"),
        t("tlen_min", 0, "chrA", 1, 0, "*", "*", 0, -2147483647, "*", "*"),
    ]
    ends = [b"\n"] * len(L)
    L.append(t("crlf", 0, "chrB", 801, 60, "5M", "*", 0, 0, "ACGTA", "IIIII")); ends.append(b"\r\n")
    L.append(t("crlf_tags", 0, "chrB", 802, 60, "5M", "*", 0, 0, "ACGTA", "*", "XC:i:1")); ends.append(b"\r\n")
    L.append(t("last", 0, "HBV", 3000, 60, "5M", "*", 0, 0, "ACGTA", "*")); ends.append(b"\n")
    return L, ends


def main():
    assert os.path.exists(SAM2BAM), "build the reference first: make -C oracle ref"
    os.makedirs(OUT, exist_ok=True)
    L, ends = forms()
    data = ST.header(NAMES, LENS).encode() + b"".join(a + e for a, e in zip(L, ends))
    sam = os.path.join(OUT, "forms.sam")
    with open(sam, "wb") as f:
        f.write(data)
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "forms.bam")
        r = subprocess.run([SAM2BAM, sam, bam], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        names, recs = ST.read_bam_full(bam)
    assert names == NAMES and len(recs) == len(L), (names, len(recs), len(L), r.stderr)
    with open(os.path.join(OUT, "forms.json"), "w") as f:
        json.dump({"names": names, "header_lines": 1 + len(NAMES), "records": recs}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("forms:", len(recs), "records,", os.path.getsize(sam), "+", os.path.getsize(os.path.join(OUT, "forms.json")), "bytes")


if __name__ == "__main__":
    main()
