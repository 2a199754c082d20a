#!/usr/bin/env python3
"""Regenerate tests/golden/clip_events/reference.json: what the REAL reference (oracle/_ref/seeksv_ref, built by `make -C oracle ref`)
writes for the designed inputs of tests/clip_events_inputs.py where it defines the result (whole inputs without ownership or ranges, the
records marked `ref`) - for each input its records as a BAM, `getclip` with the flags of every run of the input, the sha256 of the clip and
clip.fq texts and the number of rows.  The inputs are rebuilt by the tests from the same code, so only the digests are stored.  CPU only.

usage: python tests/golden/make_clip_events_reference.py
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
import clip_events_inputs as I  # noqa: E402
from test_random_oracle_vs_reference import write_sample  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
OUT = os.path.join(HERE, "clip_events")


def gz_text(path):
    with gzip.open(path, "rt") as f:
        return f.read()


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def reference_outputs(x, d):
    """-> {run tag: {clip, fq, rows}} of one input, through files in the directory d"""
    bam = os.path.join(d, x["name"] + ".bam")
    write_sample(bam, x["names"], x["lens"], [r for r in x["recs"] if r["ref"]], index=False)
    e = {}
    for tag in x["runs"]:
        pre = os.path.join(d, x["name"] + "." + tag)
        r = subprocess.run([REF, "getclip"] + I.RUN_FLAGS[tag] + ["-o", pre, bam], capture_output=True, text=True)
        assert r.returncode == 0, (x["name"], tag, r.stderr[-400:])
        clip = gz_text(pre + ".clip.gz")
        e[tag] = {"clip": sha(clip), "fq": sha(gz_text(pre + ".clip.fq.gz")), "rows": clip.count("\n")}
        os.remove(pre + ".clip.gz")
        os.remove(pre + ".clip.fq.gz")
    os.remove(bam)
    return e


def main():
    assert os.path.exists(REF), "build the reference first: make -C oracle ref"
    os.makedirs(OUT, exist_ok=True)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, x in I.inputs().items():
            if I.reference_defined(x):
                out[name] = reference_outputs(x, d)
    path = os.path.join(OUT, "reference.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(out), "inputs")


if __name__ == "__main__":
    main()
