#!/usr/bin/env python3
"""Regenerate tests/golden/random/*.json: what the REAL reference (oracle/_ref/seeksv_ref and oracle/_ref/bamidx, built by
`make -C oracle ref`) writes for the randomized inputs of tests/test_random_oracle_vs_reference.py and
tests/test_random_cli_vs_reference_gpu.py.  The inputs are made by the tests' own generators (seeded), so the tests rebuild
them and compare against what is stored here: the sha256 of every output, and the getsv -B tables whole (the oracle test
parses them).  CPU only.

usage: python tests/golden/make_random_reference.py
"""
import gzip
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
import test_random_cli_vs_reference_gpu as C  # noqa: E402
import test_random_oracle_vs_reference as R  # noqa: E402
import test_somatic_stage as S  # noqa: E402
from test_random_differential_gpu import random_sample  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
BAMIDX = os.path.join(ROOT, "oracle", "_ref", "bamidx")
OUT = os.path.join(HERE, "random")


def ref(args):
    r = subprocess.run([REF] + args, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r


def gz_text(path):
    with gzip.open(path, "rt") as f:
        return f.read()


def oracle_vs_reference(d):
    out = {"random": {}, "unsorted": {}}
    for seed in range(100, 112):
        names, lens, b, rng, recs = random_sample(seed, safe=True, want_records=True)
        bam = os.path.join(d, f"s{seed}.bam")
        R.write_sample(bam, names, lens, recs)
        e = out["random"][str(seed)] = {"getclip": {}, "getsv": {}}
        for tag, flags, kw in R.GETCLIP_RUNS:
            pre = os.path.join(d, f"s{seed}{tag}")
            ref(["getclip"] + flags + ["-o", pre, bam])
            e["getclip"][tag] = {"clip": R.sha(gz_text(pre + ".clip.gz")), "fq": R.sha(gz_text(pre + ".clip.fq.gz"))}
        jfile = os.path.join(d, "j.txt")
        R.write_junctions(jfile, R.random_junctions(rng, names, lens))
        empty_bam, empty_clip = os.path.join(d, "e.clip.bam"), os.path.join(d, "e.clip")
        bamio.write_bam(empty_bam, names, lens, [])
        open(empty_clip, "w").close()
        for q, L in R.GETSV_RUNS:
            sv = os.path.join(d, f"o{q}.sv")
            r = ref(["getsv", "-d", "0", "-f", "0", "-b", "0", "-T", "100000", "-q", str(q), "-L", str(L), "-B", jfile, empty_bam, bam, empty_clip, sv, os.path.join(d, "x.fq")])
            e["getsv"][str(q)] = {"sv": open(sv).read(), "stdout": r.stdout}
    for seed in range(300, 306):
        names, lens, b, rng, recs = random_sample(seed, safe=True, want_records=True, unsorted=True)
        bam = os.path.join(d, f"u{seed}.bam")
        R.write_sample(bam, names, lens, recs, index=False)
        e = out["unsorted"][str(seed)] = {"getclip": {}}
        for tag, flags, kw in R.GETCLIP_RUNS:
            pre = os.path.join(d, f"u{seed}{tag}")
            r = ref(["getclip"] + flags + ["-o", pre, bam])
            e["getclip"][tag] = {"clip": R.sha(gz_text(pre + ".clip.gz")), "fq": R.sha(gz_text(pre + ".clip.fq.gz"))}
        e["flushes"] = r.stderr.count("Output merged soft-clipped reads of")
    return out


def cli_vs_reference(d):
    out = {"getsv": {}, "getclip": {}}
    for seed in range(8):
        sd = os.path.join(d, f"j{seed}")
        os.makedirs(sd)
        bg, clip_bam, clip_gz = C.make_inputs(seed, sd)
        e = out["getsv"][str(seed)] = {}
        for tag, flags in C.GETSV_RUNS:
            sv = os.path.join(sd, f"ref.{tag}.sv")
            r = ref(["getsv"] + flags + [clip_bam, bg, clip_gz, sv, os.path.join(sd, "r.fq")])
            text = open(sv).read()
            e[tag] = {"sv": C.sha(text), "stdout": C.sha(r.stdout), "sv_lines": text.count("\n")}
        for tag, flags in C.SOMATIC_RUNS:
            sv = os.path.join(sd, f"ref.{tag}.sv")
            ref(["somatic"] + flags + [bg, clip_gz, os.path.join(sd, "ref.loose.sv"), sv])
            e[tag] = {"sv": C.sha(open(sv).read())}
    for seed in range(200, 206):
        bam = os.path.join(d, f"g{seed}.bam")
        C.getclip_sample(bam, seed)
        e = out["getclip"][str(seed)] = {}
        for tag, flags in C.GETCLIP_RUNS:
            pre = os.path.join(d, f"g{seed}{tag}")
            ref(["getclip"] + flags + ["-o", pre, bam])
            e[tag] = {ext: C.gz_sha(f"{pre}.{ext}") for ext in C.GZ_OUTPUTS}
    bam = os.path.join(d, "u.bam")
    C.unmapped_pairs_sample(bam)
    ref(["getclip", "-o", os.path.join(d, "u"), bam])
    e = out["unmapped_pairs"] = {}
    for ext in C.GZ_OUTPUTS:
        e[ext] = C.gz_sha(os.path.join(d, f"u.{ext}"))
        e[ext + ".lines"] = gz_text(os.path.join(d, f"u.{ext}")).count("\n")
    bam = os.path.join(d, "t.bam")
    C.table_columns_sample(bam)
    ref(["getclip", "-o", os.path.join(d, "t"), bam])
    out["table_columns"] = {"clip.gz": C.gz_sha(os.path.join(d, "t.clip.gz")), "clip.fq.gz": C.gz_sha(os.path.join(d, "t.clip.fq.gz")),
                            "clip.gz.lines": gz_text(os.path.join(d, "t.clip.gz")).count("\n")}
    return out


def somatic_vs_reference(d):
    w, b, forms = S.multimap_forms()
    bam = os.path.join(d, "normal.bam")
    bamio.soa_to_bam(bam, w.names, w.lens, b)
    subprocess.run([BAMIDX, bam], check=True, capture_output=True)
    tumor = os.path.join(HERE, "somatic", "tumor.sv")
    out = {}
    for name, (blob, env) in forms.items():
        clip = os.path.join(d, f"{name}.clip.gz")
        with open(clip, "wb") as f:
            f.write(blob)
        sv = os.path.join(d, f"{name}.ref.sv")
        ref(["somatic", "-n", "0", bam, clip, tumor, sv])
        rows = [l.split("\t") for l in open(sv).read().splitlines()]
        out[name] = {"rows": len(rows), "digest": S.rows_digest(rows)}
    return out


def main():
    assert os.path.exists(REF), "build the reference first: make -C oracle ref"
    os.makedirs(OUT, exist_ok=True)
    for name, fn in (("oracle_vs_reference", oracle_vs_reference), ("cli_vs_reference", cli_vs_reference), ("somatic_vs_reference", somatic_vs_reference)):
        with tempfile.TemporaryDirectory() as d:
            data = fn(d)
        with open(os.path.join(OUT, name + ".json"), "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
        print(name, os.path.getsize(os.path.join(OUT, name + ".json")), "bytes")


if __name__ == "__main__":
    main()
