#!/usr/bin/env python3
"""Regenerate tests/golden/original_sam/reference.json: the sha256 of every gunzipped output the REAL reference's getclip (oracle/_ref/seeksv_ref, built by
`make -C oracle ref`) writes for the bundled samples as SAM text (tests/original_sam.py), per form: plain file, gzip file, standard input.  CPU only.

usage: python tests/golden/make_original_sam_reference.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import original_sam_reference as R  # noqa: E402


def main():
    if not os.path.exists(R.SEEKSV_REF):
        sys.exit("the real reference is not built (make -C oracle ref)")
    rec = {}
    with tempfile.TemporaryDirectory() as d:
        for sample in R.SAMPLES:
            rec[sample] = {}
            for form in R.FORMS:
                out, _, _ = R.reference_getclip(d, sample, form)
                rec[sample][form] = {ext: R.sha(out[ext]) for ext in R.OUTPUTS}
    with open(R.RECORDED, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", R.RECORDED)


if __name__ == "__main__":
    main()
