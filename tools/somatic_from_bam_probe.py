#!/usr/bin/env python3
"""What `seeksv somatic -K` is worth.  The pair is bench.py's config-5 shape (human + HBV tumor at 60x against its normal at 30x, 2 % of the
records in pairs with one unmapped end) at --frac of the genome, written here with bench.py's own writer at zlib level 6.  The tumor's table comes from one
`seeksv run`; then, --reps times and alternating,
  two commands   seeksv getclip -Z -o N normal.bam  &&  seeksv somatic -Z normal.bam N.clip.gz T.sv.txt two.sv     (--parent-exe: another build's binary, the parent commit's)
  one command    seeksv somatic -K normal.bam T.sv.txt one.sv
each with SSV_TIMING=1 and a time limit of its own: wall clock exec to exit, cpu_s (user + system time of all threads), the SSV_TIMING laps, the `somatic_probe`
group's kernel time, and the sha256 of both outputs, which must be equal.  One JSON document, to --out.
usage: python tools/somatic_from_bam_probe.py [--frac F] [--reps R] [--parent-exe PATH] [--limit SECONDS] [--out profiles/somatic_from_bam.json]"""
import argparse
import hashlib
import json
import os
import re
import resource
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from seeksv_amd import synth  # noqa: E402


def timed(cmd, env, limit):
    c0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=limit)
    dt = time.perf_counter() - t0
    c1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    if r.returncode != 0:
        raise RuntimeError(" ".join(cmd[:3]) + ": " + r.stderr[-400:])
    return r, dict(wall_s=round(dt, 3), cpu_s=round(c1.ru_utime - c0.ru_utime + c1.ru_stime - c0.ru_stime, 2), laps_s={k: v for k, v in bench.timing_phases(r.stderr).items() if not k.startswith("(")},
                   detail=[l[9:] for l in r.stderr.splitlines() if l.startswith("[timing] (")])


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=1 / 16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--parent-exe", default=None)
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "somatic_from_bam.json"))
    args = ap.parse_args()
    exe = os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
    parent = args.parent_exe or exe
    kw = dict(genome_frac=args.frac, n_sv=max(8, round(10000 * args.frac)), hbv=True, unmap_permille=20)
    tumor = synth.Workload(depth=60.0, n_integrations=50, **kw)
    normal = synth.Workload(depth=30.0, **kw)
    where = bench.room_for(int((tumor.n_total + normal.n_total) * 400 + tumor.genome_len * 1.1))
    d = tempfile.mkdtemp(prefix="ssv_somK_", dir=where)
    env = dict(os.environ, SSV_TIMING="1")
    env.pop("SSV_BGZF_LEVEL", None)
    out = dict(what="seeksv getclip + seeksv somatic (two commands, clip.gz between them) against seeksv somatic -K (one decode, look-ups on the GPU)", genome_frac=args.frac,
               normal_records=normal.n_total, tumor_records=tumor.n_total, bam_level=6, two_commands_exe=os.path.relpath(parent, ROOT), cpus=bench.effective_cpus(), reps=[])
    try:
        t0 = time.perf_counter()
        tbam, nbam, fa = os.path.join(d, "tumor.bam"), os.path.join(d, "normal.bam"), os.path.join(d, "ref.fa")
        bench.write_workload_bam(tumor, tbam, 6)
        bench.write_workload_bam(normal, nbam, 6)
        tumor.write_fasta(fa, bench.effective_cpus())
        out["files_made_s"] = round(time.perf_counter() - t0, 1)
        out["normal_bam_bytes"] = os.path.getsize(nbam)
        timed([exe, "run", tbam, fa, os.path.join(d, "T")], env, args.limit)
        table = os.path.join(d, "T.sv.txt")
        out["tumor_rows"] = sum(1 for l in open(table) if not l.startswith("@"))
        os.remove(tbam)
        for rep in range(args.reps):
            two, one = os.path.join(d, "two.sv"), os.path.join(d, "one.sv")
            _, g = timed([parent, "getclip", "-Z", "-o", os.path.join(d, "N"), nbam], env, args.limit)
            _, s = timed([parent, "somatic", "-Z", nbam, os.path.join(d, "N.clip.gz"), table, two], env, args.limit)
            rk, k = timed([exe, "somatic", "-K", nbam, table, one], env, args.limit)
            m = re.search(r"somatic -K: (\d+) probes, (\d+) bytes of text, (\d+) passes; somatic_probe kernel time ([0-9.e+-]+) ms in (\d+) launches", rk.stderr)
            probe = dict(probes=int(m.group(1)), text_bytes=int(m.group(2)), passes=int(m.group(3)), somatic_probe_kernel_ms=float(m.group(4)), launches=int(m.group(5))) if m else None
            sums = dict(two_commands=sha(two), one_command=sha(one))
            out["reps"].append(dict(getclip=g, somatic=s, two_commands_wall_s=round(g["wall_s"] + s["wall_s"], 3), two_commands_cpu_s=round(g["cpu_s"] + s["cpu_s"], 2),
                                    somatic_K=k, somatic_probe=probe, sha256=sums, outputs_equal=sums["two_commands"] == sums["one_command"],
                                    files_between=sum(os.path.getsize(os.path.join(d, "N" + x)) for x in (".clip.gz", ".clip.fq.gz", ".unmapped_1.fq.gz", ".unmapped_2.fq.gz"))))
            if not out["reps"][-1]["outputs_equal"]:
                raise RuntimeError("the two paths' outputs differ")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(dict(out=os.path.relpath(args.out, ROOT), reps=[dict(two_commands_wall_s=r["two_commands_wall_s"], somatic_K_wall_s=r["somatic_K"]["wall_s"]) for r in out["reps"]])))


if __name__ == "__main__":
    main()
