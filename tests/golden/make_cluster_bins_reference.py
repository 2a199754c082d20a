#!/usr/bin/env python3
"""Regenerate tests/golden/cluster_bins/reference.json: what the REAL reference (oracle/_ref/seeksv_ref, built by `make -C oracle ref`)
writes for the designed samples of tests/cluster_bins_inputs.py - for each sample its reference-defined records as a BAM, `getclip` with -t
for every run of the sample's family, the sha256 of the clip and clip.fq texts and the number of rows.  The samples are rebuilt by the tests
from the same code, so only the digests are stored.  CPU only.

usage: python tests/golden/make_cluster_bins_reference.py
"""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_bins_inputs as I  # noqa: E402
from test_random_oracle_vs_reference import write_sample  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
OUT = os.path.join(HERE, "cluster_bins")


def gz_text(path):
    with gzip.open(path, "rt") as f:
        return f.read()


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def main():
    assert os.path.exists(REF), "build the reference first: make -C oracle ref"
    os.makedirs(OUT, exist_ok=True)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for family, cls in I.SAMPLE_IDS:
            s = I.sample(family, cls)
            bam = os.path.join(d, s["name"] + ".bam")
            write_sample(bam, s["names"], s["lens"], [r for r in s["recs"] if r["ref"]], index=False)
            e = out[s["name"]] = {}
            for tag, flags, kw in I.runs_of(family):
                pre = os.path.join(d, s["name"] + tag)
                r = subprocess.run([REF, "getclip"] + flags + ["-o", pre, bam], capture_output=True, text=True)
                assert r.returncode == 0, (s["name"], tag, r.stderr[-400:])
                clip = gz_text(pre + ".clip.gz")
                e[tag] = {"clip": sha(clip), "fq": sha(gz_text(pre + ".clip.fq.gz")), "rows": clip.count("\n")}
            os.remove(bam)
    path = os.path.join(OUT, "reference.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
