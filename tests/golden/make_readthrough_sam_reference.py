#!/usr/bin/env python3
"""Regenerate tests/golden/readthrough/sam.json: what the REAL reference (oracle/_ref/seeksv_ref, built by `make -C oracle ref`) writes for
`getsv -F` on the SAM TEXT of the seeded inputs of tests/readthrough_inputs.py, without the read names that own an '=' or 'X' CIGAR (libbam 0.1.16's
text reader aborts on those characters).  The small file: the .sv text, stdout and the stderr lines whole, under every RT.SMALL_RUNS; the random seeds:
sha256 digests under RT.RANDOM_RUNS.  CPU only.

usage: python tests/golden/make_readthrough_sam_reference.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_readthrough_reference as MR  # noqa: E402
import readthrough_inputs as RT  # noqa: E402
import sam_text as ST  # noqa: E402
import test_random_cli_vs_reference_gpu as C  # noqa: E402


def small(d):
    recs = ST.without_eq_x(ST.clip_positions(RT.small_records(), RT.LENS))
    fsam = os.path.join(d, "small.sam")
    ST.write(fsam, recs, RT.NAMES, RT.LENS)
    clip_bam, clip = RT.empty_clip_inputs(d)
    bfile = os.path.join(d, "b.txt")
    with open(bfile, "w") as f:
        f.write(RT.b_rows())
    out = {"records": len(recs)}
    for tag, flags in RT.SMALL_RUNS:
        sv = os.path.join(d, f"small.{tag}.sv")
        r = MR.ref(["getsv"] + RT.flags_with(flags, bfile) + ["-F", fsam, clip_bam, RT.BG, clip, sv, os.path.join(d, "x.fq")])
        out[tag] = {"sv": open(sv).read(), "stdout": r.stdout, "stderr_lines": [RT.unpath(l) for l in r.stderr.splitlines()]}
    return out


def random(d):
    out = {}
    for seed in RT.RANDOM_SEEDS:
        sd = os.path.join(d, f"r{seed}")
        os.makedirs(sd)
        bg, clip_bam, clip_gz = C.make_inputs(seed, sd)
        recs = ST.without_eq_x(ST.clip_positions(RT.random_records(seed), RT.LENS))
        fsam = os.path.join(sd, "f.sam")
        ST.write(fsam, recs, RT.NAMES, RT.LENS)
        e = out[str(seed)] = {"records": len(recs)}
        for tag, flags in RT.RANDOM_RUNS:
            sv = os.path.join(sd, f"o.{tag}.sv")
            r = MR.ref(["getsv"] + flags + ["-F", fsam, clip_bam, bg, clip_gz, sv, os.path.join(sd, "x.fq")])
            text = open(sv).read()
            e[tag] = {"sv": MR.sha(text), "stdout": MR.sha(r.stdout), "sv_lines": text.count("\n")}
    return out


def main():
    assert os.path.exists(MR.REF), "build the reference first: make -C oracle ref"
    with tempfile.TemporaryDirectory() as d:
        data = {"small": small(d), "random": random(d)}
    path = os.path.join(MR.OUT, "sam.json")
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("sam", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
