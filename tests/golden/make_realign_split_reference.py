#!/usr/bin/env python3
"""Regenerate tests/golden/realign_split/: what the REAL reference's getsv (oracle/_ref/seeksv_ref, built by `make -C oracle ref`) prints for the sample
of tests/realign_split_inputs.e2e_sample() - pairs whose unmapped read crosses a planted inter-contig junction - when its -F file holds the records of the
re-aligner's MODEL (tests/realign_split_model.py) for the reads of the reference getclip's prefix.unmapped_2.fq.gz (e2e.F.sv, e2e.F.stdout:
`seeksv getclip` -> `seeksv realign -P` -> `seeksv getsv -F` has to reproduce them) and without -F (e2e.sv, e2e.stdout); tests/test_realign_split_gpu.py.
clip.bam holds the model's records (tests/realign_model.py) for the reference getclip's clip.fq.gz.  CPU only.

The sample exists for one property, asserted here: with -F the planted junction's two ends appear in the SV table or among the filtered junctions on
stdout; without -F they appear in neither.

usage: python tests/golden/make_realign_split_reference.py
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
import realign_model as M  # noqa: E402
import realign_split_inputs as SI  # noqa: E402
import realign_split_model as SM  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
BAMIDX = os.path.join(ROOT, "oracle", "_ref", "bamidx")
OUT = os.path.join(HERE, "realign_split")
HEADER = "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(SI.E2E_NAMES, SI.E2E_LENS))


def run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r


def fastq(path):
    lines = gzip.open(path, "rt").read().splitlines()
    return list(zip(lines[0::4], lines[1::4], lines[3::4]))


def write(path, rows):
    recs = [dict(qname=r["name"], flag=r["flag"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar="".join(f"{n}{op}" for n, op in r["cigar"]), seq=r["seq"], qual=r["qual"]) for r in rows]
    bamio.write_bam(path, list(SI.E2E_NAMES), list(SI.E2E_LENS), recs, sam_header_text=HEADER)
    return recs


def main():
    assert os.path.exists(REF), "build the reference first: make -C oracle ref"
    os.makedirs(OUT, exist_ok=True)
    contigs, recs = SI.e2e_sample()
    ref = M.Reference(contigs)
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "s.bam")
        bamio.write_bam(bam, list(SI.E2E_NAMES), list(SI.E2E_LENS), recs)
        run([BAMIDX, bam])
        pre = os.path.join(d, "s")
        run([REF, "getclip", "-o", pre, bam])
        with open(pre + ".unmapped_2.fq.gz", "rb") as f, open(os.path.join(OUT, "e2e.unmapped_2.fq.gz"), "wb") as g:   # what `seeksv getclip` has to write too
            g.write(f.read())
        clip = write(os.path.join(d, "clip.bam"), [dict(M.bam_record(s, q, M.align(ref, s)), name=s) for _, s, q in fastq(pre + ".clip.fq.gz")])
        reads = fastq(pre + ".unmapped_2.fq.gz")
        rows = [r for name, s, q in reads for r in SM.bam_records(name[1:].split()[0], s, q, SM.align_split(ref, s))]
        conn = write(os.path.join(d, "F.bam"), rows)
        print(len(clip), "clip records;", len(reads), "unmapped reads,", len(conn), "connected records,", sum(c["flag"] & 2048 != 0 for c in conn), "supplementary")
        assert len(reads) == SI.E2E_READS and len(conn) == 2 * SI.E2E_READS
        found = {}
        for tag, extra in (("e2e.F", ["-F", os.path.join(d, "F.bam")]), ("e2e", [])):
            r = run([REF, "getsv"] + SI.E2E_SV_OPTS + extra + [os.path.join(d, "clip.bam"), bam, pre + ".clip.gz", os.path.join(d, tag + ".sv"), os.path.join(d, tag + ".u.fq")])
            text = open(os.path.join(d, tag + ".sv")).read()
            with open(os.path.join(OUT, tag + ".sv"), "w") as f:
                f.write(text)
            with open(os.path.join(OUT, tag + ".stdout"), "w") as f:
                f.write(r.stdout)
            print(tag, text.count("\n"), "table lines,", r.stdout.count("\n"), "stdout lines")
            print(text)
            print(r.stdout)
            found[tag] = (SI.e2e_names_both_ends(text), SI.e2e_names_both_ends(r.stdout))
        print(found)
        assert any(found["e2e.F"]), "with -F the planted junction has to appear in the table or among the filtered junctions"
        assert not any(found["e2e"]), "without -F it must appear in neither"


if __name__ == "__main__":
    main()
