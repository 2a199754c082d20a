"""What the real reference's getclip (oracle/_ref/seeksv_ref) writes for the bundled samples as SAM text (tests/original_sam.py), in the three forms it can be
given: a plain file, a gzip file, standard input.  Shared by tests/test_original_sam_reference.py and tests/golden/make_original_sam_reference.py."""
import gzip
import hashlib
import os
import subprocess

import golden_util as G
import original_sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV_REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
RECORDED = os.path.join(G.GOLDEN, "original_sam", "reference.json")
SAMPLES = ("cancer", "normal")
FORMS = ("plain", "gzip", "stdin")
OUTPUTS = ("clip.gz", "clip.fq.gz", "unmapped_1.fq.gz", "unmapped_2.fq.gz")
GOLDEN_OF = {"clip.gz": "clip.txt", "clip.fq.gz": "clip.fq.txt", "unmapped_1.fq.gz": "unmapped_1.fq.txt", "unmapped_2.fq.gz": "unmapped_2.fq.txt"}


def sha(data):
    return hashlib.sha256(data).hexdigest()


def golden_bytes(sample, ext):
    with open(os.path.join(G.GOLDEN, "example", f"{sample}.{GOLDEN_OF[ext]}"), "rb") as f:
        return f.read()


def reference_getclip(d, sample, form):
    """-> ({output: gunzipped bytes}, stderr, number of contigs)"""
    data, _, names = original_sam.sam_of_bam(os.path.join(G.GOLDEN, "example", sample + ".sort.bam"))
    path = os.path.join(d, sample + (".sam.gz" if form == "gzip" else ".sam"))
    with (gzip.open(path, "wb") if form == "gzip" else open(path, "wb")) as f:
        f.write(data)
    prefix = os.path.join(d, f"{sample}.{form}")
    if form == "stdin":
        with open(path, "rb") as f:
            r = subprocess.run([SEEKSV_REF, "getclip", "-o", prefix, "-"], capture_output=True, text=True, stdin=f)
    else:
        r = subprocess.run([SEEKSV_REF, "getclip", "-o", prefix, path], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-400:]
    out = {}
    for ext in OUTPUTS:
        with gzip.open(f"{prefix}.{ext}", "rb") as f:
            out[ext] = f.read()
    return out, r.stderr, len(names)
