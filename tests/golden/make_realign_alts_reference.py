#!/usr/bin/env python3
"""Regenerate tests/golden/realign_alts/: what the REAL reference's getsv (oracle/_ref/seeksv_ref, built by `make -C oracle ref`) prints for the sample of
tests/realign_alts_inputs.e2e_sample() when its clip.bam holds the records of the re-aligner's MODEL (tests/realign_alts_model.py) for the clipped
sequences the reference's getclip wrote - with the alternate loci as secondary records (e2e.sv, e2e.stdout: `seeksv run -a "-c 500 -S 8"` has to
reproduce them) and without (e2e.primary.sv, e2e.primary.stdout: `seeksv run -a "-c 500"`); tests/test_realign_alts_gpu.py.  Also kept: the reference
getclip's e2e.clip.gz and e2e.clip.fq.gz, from which tests/test_realign_alts_join.py drives the host join on the CPU.  CPU only.

The sample exists for one property, asserted here: with the alternates the planted junction's two ends appear in the SV table or among the filtered
junctions on stdout; without them they appear in neither.

usage: python tests/golden/make_realign_alts_reference.py
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
import realign_alts_inputs as AI  # noqa: E402
import realign_alts_model as AM  # noqa: E402
import realign_model as M  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
BAMIDX = os.path.join(ROOT, "oracle", "_ref", "bamidx")
OUT = os.path.join(HERE, "realign_alts")
MAX_ALT = 8


def run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r


def model_clip_bam(path, fq_gz, contigs, max_alt):
    """clip.bam as `seeksv realign -c 500 [-S max_alt]` writes it: per FASTQ entry, in order, the primary's record and its secondary records; the read
    name is the sequence"""
    ref = M.Reference(contigs)
    lines = gzip.open(fq_gz, "rt").read().splitlines()
    recs = []
    for s, q in zip(lines[1::4], lines[3::4]):
        res = AM.align_alts(ref, s, max_alt or 1, AI.CAP)
        if not max_alt:
            res["alts"] = []
        for r in AM.bam_records(s, q, res):
            recs.append(dict(qname=s, flag=r["flag"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar="".join(f"{n}{op}" for n, op in r["cigar"]), seq=r["seq"], qual=r["qual"]))
    bamio.write_bam(path, list(AI.E2E_NAMES), list(AI.E2E_LENS), recs, sam_header_text="".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(AI.E2E_NAMES, AI.E2E_LENS)))
    return recs


def has_junction(text):
    """a line that names both ends of the planted junction: tA at E2E_A + 1 and tB at E2E_B + 1 (1-based)"""
    a, b = ("tA", str(AI.E2E_A + 1)), ("tB", str(AI.E2E_B + 1))
    for line in text.splitlines():
        f = line.split("\t")
        pairs = set(zip(f, f[1:]))
        if a in pairs and b in pairs:
            return True
    return False


def main():
    assert os.path.exists(REF), "build the reference first: make -C oracle ref"
    os.makedirs(OUT, exist_ok=True)
    contigs, recs = AI.e2e_sample()
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "s.bam")
        bamio.write_bam(bam, list(AI.E2E_NAMES), list(AI.E2E_LENS), recs)
        run([BAMIDX, bam])
        pre = os.path.join(d, "s")
        run([REF, "getclip", "-o", pre, bam])
        for ext in ("clip.gz", "clip.fq.gz"):   # the reference's getclip output, for the CPU test of the join (tests/test_realign_alts_join.py)
            with open(pre + "." + ext, "rb") as f, open(os.path.join(OUT, "e2e." + ext), "wb") as g:
                g.write(f.read())
        found = {}
        for tag, max_alt in (("e2e", MAX_ALT), ("e2e.primary", 0)):
            clip = model_clip_bam(os.path.join(d, tag + ".clip.bam"), pre + ".clip.fq.gz", contigs, max_alt)
            r = run([REF, "getsv"] + AI.E2E_SV_OPTS + [os.path.join(d, tag + ".clip.bam"), bam, pre + ".clip.gz", os.path.join(d, tag + ".sv"), os.path.join(d, tag + ".u.fq")])
            text = open(os.path.join(d, tag + ".sv")).read()
            print(tag, len(clip), "clip records,", sum(c["flag"] & 256 != 0 for c in clip), "secondary;", text.count("\n"), "table lines")
            with open(os.path.join(OUT, tag + ".sv"), "w") as f:
                f.write(text)
            with open(os.path.join(OUT, tag + ".stdout"), "w") as f:
                f.write(r.stdout)
            print(text)
            print(r.stdout)
            found[tag] = (has_junction(text), has_junction(r.stdout))
        print(found)
        assert any(found["e2e"]), "with the alternates the planted junction has to appear in the table or among the filtered junctions"
        assert not any(found["e2e.primary"]), "without them it must appear in neither"


if __name__ == "__main__":
    main()
