#!/usr/bin/env python3
"""Regenerate tests/golden/readthrough/: what the REAL reference (oracle/_ref/seeksv_ref, built by `make -C oracle ref`) writes for
`getsv -F` on the seeded inputs of tests/readthrough_inputs.py.  The small hand-made file: the .sv text and stdout whole, and the order of
the stderr lines; the random files: sha256 digests.  The tests rebuild the inputs from the seeds.  CPU only.

model_anchor: generated samples of tests/readthrough_model.py, the .sv text and stdout whole (held against the Python model of FindJunction).

usage: python tests/golden/make_readthrough_reference.py [section ...]     (all sections by default)
"""
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
import readthrough_inputs as RT  # noqa: E402
import test_random_cli_vs_reference_gpu as C  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
OUT = os.path.join(HERE, "readthrough")


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def ref(args):
    r = subprocess.run([REF] + args, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r


def small(d):
    fbam = os.path.join(d, "small.bam")
    RT.write_f_bam(fbam, RT.small_records())
    clip_bam, clip = RT.empty_clip_inputs(d)
    bfile = os.path.join(d, "b.txt")
    with open(bfile, "w") as f:
        f.write(RT.b_rows())
    out = {}
    for tag, flags in RT.SMALL_RUNS:
        sv = os.path.join(d, f"small.{tag}.sv")
        r = ref(["getsv"] + RT.flags_with(flags, bfile) + ["-F", fbam, clip_bam, RT.BG, clip, sv, os.path.join(d, "x.fq")])
        out[tag] = {"sv": open(sv).read(), "stdout": r.stdout, "stderr_lines": [RT.unpath(l) for l in r.stderr.splitlines()]}
    return out


def random(d):
    out = {}
    for seed in RT.RANDOM_SEEDS:
        sd = os.path.join(d, f"r{seed}")
        os.makedirs(sd)
        bg, clip_bam, clip_gz = C.make_inputs(seed, sd)
        fbam = os.path.join(sd, "f.bam")
        recs = RT.random_records(seed)
        RT.write_f_bam(fbam, recs)
        e = out[str(seed)] = {"records": len(recs)}
        for tag, flags in RT.RANDOM_RUNS:
            sv = os.path.join(sd, f"o.{tag}.sv")
            r = ref(["getsv"] + flags + ["-F", fbam, clip_bam, bg, clip_gz, sv, os.path.join(sd, "x.fq")])
            text = open(sv).read()
            e[tag] = {"sv": sha(text), "stdout": sha(r.stdout), "sv_lines": text.count("\n")}
    return out


def large(d):
    fbam = os.path.join(d, "large.bam")
    recs = RT.random_records(RT.LARGE_SEED, n_names=RT.LARGE_NAMES)
    RT.write_f_bam(fbam, recs)
    clip_bam, clip = RT.empty_clip_inputs(d)
    sv = os.path.join(d, "large.sv")
    r = ref(["getsv"] + RT.LOOSE + ["-F", fbam, clip_bam, RT.BG, clip, sv, os.path.join(d, "x.fq")])
    text = open(sv).read()
    return {"records": len(recs), "contig_changes": RT.contig_changes(recs), "sv": sha(text), "stdout": sha(r.stdout), "sv_lines": text.count("\n")}


def model_anchor(d):
    """generated samples (tests/readthrough_model.py, safe: only inputs the reference defines) with contigs of their own: the original BAM is a
    few hundred proper pairs on the sample's first contig, indexed through the reference's libbam; the .sv text and stdout whole"""
    import bamio
    import readthrough_model as M
    out = {}
    for seed in M.ANCHOR_SEEDS:
        sd = os.path.join(d, f"a{seed}")
        os.makedirs(sd)
        s = M.anchor_sample(seed)
        fbam, bg = os.path.join(sd, "f.bam"), os.path.join(sd, "bg.bam")
        bamio.write_bam(fbam, s["contigs"], s["lens"], M.sample_records(s))
        pairs = []
        for k in range(300):
            p = 1000 + 20 * k
            pairs.append(dict(qname=f"p{k}", flag=99, tid=0, pos=p, mapq=60, cigar="100M", mtid=0, mpos=p + 200, isize=300, seq="A" * 100, qual="I" * 100))
            pairs.append(dict(qname=f"p{k}", flag=147, tid=0, pos=p + 200, mapq=60, cigar="100M", mtid=0, mpos=p, isize=-300, seq="A" * 100, qual="I" * 100))
        bamio.write_bam(bg, s["contigs"], s["lens"], sorted(pairs, key=lambda r: r["pos"]))
        subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", "bamidx"), bg])
        clip_bam, clip = os.path.join(sd, "e.clip.bam"), os.path.join(sd, "e.clip")
        bamio.write_bam(clip_bam, s["contigs"], s["lens"], [])
        open(clip, "w").close()
        e = out[str(seed)] = {"records": len(s["qnames"])}
        for tag, w in M.ANCHOR_RUNS:
            sv = os.path.join(sd, f"o.{tag}.sv")
            r = ref(["getsv"] + RT.LOOSE + ["-w", str(w), "-F", fbam, clip_bam, bg, clip, sv, os.path.join(sd, "x.fq")])
            e[tag] = {"sv": open(sv).read(), "stdout": r.stdout}
    return out


SECTIONS = (("small", small), ("random", random), ("large", large), ("model_anchor", model_anchor))


def main():
    assert os.path.exists(REF), "build the reference first: make -C oracle ref"
    os.makedirs(OUT, exist_ok=True)
    for name, fn in SECTIONS:
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        with tempfile.TemporaryDirectory() as d:
            data = fn(d)
        with open(os.path.join(OUT, name + ".json"), "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
        print(name, os.path.getsize(os.path.join(OUT, name + ".json")), "bytes")


if __name__ == "__main__":
    main()
