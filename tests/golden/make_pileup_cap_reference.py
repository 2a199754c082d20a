#!/usr/bin/env python3
"""Regenerate tests/golden/pileup_cap/reference.json: what the REAL reference (oracle/_ref/seeksv_ref and oracle/_ref/bamidx, built by
`make oracle-ref`) writes for the inputs of tests/pileup_cap_inputs.py - the .sv table and the stdout of the -B harness, whole, per case,
for -q 20 and -q 0.  The inputs are made by the tests' own generators, so the tests rebuild them and compare against what is stored here.
CPU only.  A case on which the reference exits with a non-zero status stops the run: it does not belong in the list.

usage: python tests/golden/make_pileup_cap_reference.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bamio  # noqa: E402
import pileup_cap_inputs as P  # noqa: E402
from test_random_oracle_vs_reference import write_junctions  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
BAMIDX = os.path.join(ROOT, "oracle", "_ref", "bamidx")
OUT = os.path.join(HERE, "pileup_cap", "reference.json")


def main():
    assert os.path.exists(REF), "build the reference first: make oracle-ref"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name in P.CASES:
            c = P.case(name)
            bam = os.path.join(d, name + ".bam")
            P.write_bam(bam, c)
            subprocess.run([BAMIDX, bam], check=True, capture_output=True)
            jfile = os.path.join(d, name + ".junctions.txt")
            write_junctions(jfile, c.junctions)
            empty_bam, empty_clip = os.path.join(d, name + ".e.clip.bam"), os.path.join(d, "e.clip")
            bamio.write_bam(empty_bam, c.names, c.lens, [])
            open(empty_clip, "w").close()
            e = out[name] = {}
            for q in (20, 0):
                sv = os.path.join(d, f"{name}.q{q}.sv")
                # as tests/golden/make_golden.py:crafted_getsv runs the harness (-d 0 -f 0 -b 0: every junction with a discordant pair
                # reaches the table with all its depth columns)
                r = subprocess.run([REF, "getsv", "-d", "0", "-f", "0", "-b", "0", "-T", "100000", "-q", str(q), "-B", jfile, empty_bam, bam, empty_clip, sv,
                                    os.path.join(d, "x.fq")], capture_output=True, text=True)
                assert r.returncode == 0, (name, q, r.returncode, r.stderr[-400:])
                e[str(q)] = {"sv": open(sv).read(), "stdout": r.stdout}
            print(name, len(c.recs), "records")
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
