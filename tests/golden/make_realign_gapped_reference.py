#!/usr/bin/env python3
"""Regenerate tests/golden/realign_gapped/e2e.sv and e2e.stdout: what the REAL reference's getsv (oracle/_ref/seeksv_ref, built by `make -C oracle ref`)
prints for the sample of tests/realign_gapped_inputs.e2e_sample() when its clip.bam holds the records of the gapped re-aligner's MODEL
(tests/realign_gapped_model.py) for the clipped sequences the reference's getclip wrote.  `seeksv run -a "-g"` has to reproduce the table
(tests/test_realign_gapped_gpu.py).  CPU only.

usage: python tests/golden/make_realign_gapped_reference.py
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
import realign_gapped_inputs as GI  # noqa: E402
import realign_gapped_model as GM  # noqa: E402
import realign_model as M  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
BAMIDX = os.path.join(ROOT, "oracle", "_ref", "bamidx")
OUT = os.path.join(HERE, "realign_gapped")


def run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r


def model_clip_bam(path, fq_gz, contigs, gapped=True):
    """clip.bam as `seeksv realign [-g]` writes it: one record per FASTQ entry, in order, the read name is the sequence"""
    ref = M.Reference(contigs)
    lines = gzip.open(fq_gz, "rt").read().splitlines()
    recs = []
    for s, q in zip(lines[1::4], lines[3::4]):
        r = GM.bam_record(s, q, GM.align_gapped(ref, s)) if gapped else M.bam_record(s, q, M.align(ref, s))
        recs.append(dict(qname=s, flag=r["flag"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar="".join(f"{n}{op}" for n, op in r["cigar"]), seq=r["seq"], qual=r["qual"]))
    bamio.write_bam(path, list(GI.E2E_NAMES), list(GI.E2E_LENS), recs, sam_header_text="".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(GI.E2E_NAMES, GI.E2E_LENS)))
    return recs


def main():
    assert os.path.exists(REF), "build the reference first: make -C oracle ref"
    os.makedirs(OUT, exist_ok=True)
    contigs, recs = GI.e2e_sample()
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "s.bam")
        bamio.write_bam(bam, list(GI.E2E_NAMES), list(GI.E2E_LENS), recs)
        run([BAMIDX, bam])
        pre = os.path.join(d, "s")
        run([REF, "getclip", "-o", pre, bam])
        for tag, gapped in (("e2e", True), ("e2e.ungapped", False)):
            clip = model_clip_bam(os.path.join(d, tag + ".clip.bam"), pre + ".clip.fq.gz", contigs, gapped)
            r = run([REF, "getsv"] + GI.E2E_SV_OPTS + [os.path.join(d, tag + ".clip.bam"), bam, pre + ".clip.gz", os.path.join(d, tag + ".sv"), os.path.join(d, tag + ".u.fq")])
            text = open(os.path.join(d, tag + ".sv")).read()
            print(tag, len(clip), "clip records,", sum("D" in c["cigar"] or "I" in c["cigar"] for c in clip), "with a gap;", text.count("\n"), "table lines")
            if gapped:
                with open(os.path.join(OUT, "e2e.sv"), "w") as f:
                    f.write(text)
                with open(os.path.join(OUT, "e2e.stdout"), "w") as f:
                    f.write(r.stdout)
            print(text)
            print(r.stdout)


if __name__ == "__main__":
    main()
