#!/usr/bin/env python3
"""Regenerate tests/golden/markdup/: what the REAL reference (oracle/_ref/seeksv_ref, built by `make -C oracle ref`) writes for the sample of
tests/markdup_cli_inputs.sample() once its duplicates are marked by the rule's plain model (tests/markdup_model.py): getclip's clip.gz and getsv's table and
stdout (marked.*), with the records of the re-aligner's MODEL (tests/realign_model.py) for the reference getclip's clip.fq.gz as clip.bam - what
`seeksv run -M` on the unmarked BAM has to reproduce (tests/test_markdup_cli_gpu.py) - and the same for the unmarked BAM (plain.*).  CPU only.

The sample exists for one property, asserted here: junction A is in the table of the unmarked BAM and not in the table of the marked one; junction B is in both.

usage: python tests/golden/make_markdup_reference.py
"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bamio  # noqa: E402
import markdup_cli_inputs as CI  # noqa: E402
import realign_model as M  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
BAMIDX = os.path.join(ROOT, "oracle", "_ref", "bamidx")
OUT = os.path.join(HERE, "markdup")
HEADER = "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(CI.NAMES, CI.LENS))
SV_OPTS = ["-b", "3"]


def run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r


def fastq(path):
    lines = gzip.open(path, "rt").read().splitlines()
    return list(zip(lines[0::4], lines[1::4], lines[3::4]))


def main():
    assert os.path.exists(REF), "build the reference first: make -C oracle ref"
    os.makedirs(OUT, exist_ok=True)
    contigs, recs = CI.sample()
    ref = M.Reference(contigs)
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for tag, records in (("marked", CI.flagged(recs)), ("plain", recs)):
            bam = os.path.join(d, tag + ".bam")
            bamio.write_bam(bam, list(CI.NAMES), list(CI.LENS), records)
            run([BAMIDX, bam])
            pre = os.path.join(d, tag)
            run([REF, "getclip", "-o", pre, bam])
            rows = [dict(M.bam_record(s, q, M.align(ref, s)), name=s) for _, s, q in fastq(pre + ".clip.fq.gz")]
            clip = [dict(qname=r["name"], flag=r["flag"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar="".join(f"{n}{op}" for n, op in r["cigar"]), seq=r["seq"], qual=r["qual"]) for r in rows]
            bamio.write_bam(os.path.join(d, tag + ".clip.bam"), list(CI.NAMES), list(CI.LENS), clip, sam_header_text=HEADER)
            r = run([REF, "getsv"] + SV_OPTS + [os.path.join(d, tag + ".clip.bam"), bam, pre + ".clip.gz", pre + ".sv", pre + ".u.fq"])
            text = open(pre + ".sv").read()
            with open(os.path.join(OUT, tag + ".sv"), "w") as f:
                f.write(text)
            with open(os.path.join(OUT, tag + ".stdout"), "w") as f:
                f.write(r.stdout)
            with open(os.path.join(OUT, tag + ".clip.txt"), "w") as f:
                f.write(gzip.open(pre + ".clip.gz", "rt").read())
            found[tag] = (CI.names_both_ends(text, CI.JUNCTION_A), CI.names_both_ends(text, CI.JUNCTION_B))
            print(tag, len(clip), "clip records;", text.count("\n"), "table lines,", r.stdout.count("\n"), "stdout lines")
            print(text)
    print(found)
    assert found["plain"] == (True, True), "unmarked: both junctions are in the table"
    assert found["marked"] == (False, True), "marked: junction A's two reads stay below -b 3, junction B stays"


if __name__ == "__main__":
    main()
