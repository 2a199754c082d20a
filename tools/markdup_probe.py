#!/usr/bin/env python3
"""What `seeksv run -M` costs.  The sample is bench.py's config-5 tumor shape without the virus contig (human at 60x, 2 % of the records in pairs with
one unmapped end; with hbv=True the generator's last contig comes out with a few records out of order, which -M refuses as not coordinate sorted) at --frac of the genome, written here with bench.py's own writer at zlib level 6.  Then, --reps times and alternating,
  base      <parent-exe> run tumor.bam ref.fa B        (--parent-exe: another build's binary, the parent commit's - the base for the run without -M)
  plain     seeksv run tumor.bam ref.fa P
  marking   seeksv run -M tumor.bam ref.fa M
each with SSV_TIMING=1 and a time limit of its own: wall clock exec to exit, cpu_s, the SSV_TIMING laps, the resident bytes per record `run` reports, and for -M
the records marked and the kernel time of the dup_select / dup_mark / dup_retain groups.  base and plain must write the same table (sha256).  One JSON
document, to --out.
usage: python tools/markdup_probe.py [--frac F] [--reps R] [--parent-exe PATH] [--limit SECONDS] [--out profiles/markdup.json]"""
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
    laps = {k: v for k, v in bench.timing_phases(r.stderr).items() if not k.startswith("(")}
    d = dict(wall_s=round(dt, 3), cpu_s=round(c1.ru_utime - c0.ru_utime + c1.ru_stime - c0.ru_stime, 2), laps_s=laps)
    m = re.search(r"\(run: (\d+) records kept in (\d+) batches, (\d+) CIGAR operations, (\d+) bytes of bases \+ qualities: ([0-9.e+-]+) bytes a record", r.stderr)
    if m:
        d["resident"] = dict(records=int(m.group(1)), batches=int(m.group(2)), seqqual_bytes=int(m.group(4)), bytes_per_record=float(m.group(5)))
    m = re.search(r"\[seeksv\] -M: marked (\d+) \+ (\d+) duplicate records \((\d+) groups\) of (\d+)", r.stderr)
    if m:
        d["marked"] = dict(heads=int(m.group(1)), tails=int(m.group(2)), groups=int(m.group(3)), records=int(m.group(4)))
    m = re.search(r"\(-M kernel time: dup_select ([0-9.e+-]+) ms in (\d+) launches, dup_mark ([0-9.e+-]+) ms in (\d+) launches, dup_retain ([0-9.e+-]+) ms in (\d+) launches; "
                  r"hold-back at most (\d+) records, (\d+) digests", r.stderr)
    if m:
        d["dup_kernel_ms"] = dict(dup_select=float(m.group(1)), dup_mark=float(m.group(3)), dup_retain=float(m.group(5)), total=round(float(m.group(1)) + float(m.group(3)) + float(m.group(5)), 3),
                                  launches=int(m.group(2)) + int(m.group(4)) + int(m.group(6)), held_max=int(m.group(7)), set_entries=int(m.group(8)))
    return r, d


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=1 / 32)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--parent-exe", default=None)
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "markdup.json"))
    args = ap.parse_args()
    exe = os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
    parent = args.parent_exe or exe
    tumor = synth.Workload(depth=60.0, genome_frac=args.frac, n_sv=max(8, round(10000 * args.frac)), unmap_permille=20)
    where = bench.room_for(int(tumor.n_total * 400 + tumor.genome_len * 1.1))
    d = tempfile.mkdtemp(prefix="ssv_markdup_", dir=where)
    env = dict(os.environ, SSV_TIMING="1")
    env.pop("SSV_BGZF_LEVEL", None)
    out = dict(what="seeksv run (the parent's binary, then this build's) against seeksv run -M on one device-generated sample", genome_frac=args.frac, records=tumor.n_total, bam_level=6,
               base_exe=os.path.relpath(parent, ROOT), base_is_another_build=os.path.realpath(parent) != os.path.realpath(exe), cpus=bench.effective_cpus(), reps=[])
    try:
        t0 = time.perf_counter()
        bam, fa = os.path.join(d, "tumor.bam"), os.path.join(d, "ref.fa")
        bench.write_workload_bam(tumor, bam, 6)
        tumor.write_fasta(fa, bench.effective_cpus())
        out["files_made_s"] = round(time.perf_counter() - t0, 1)
        out["bam_bytes"] = os.path.getsize(bam)
        for rep in range(args.reps):
            _, b = timed([parent, "run", bam, fa, os.path.join(d, "B")], env, args.limit)
            _, p = timed([exe, "run", bam, fa, os.path.join(d, "P")], env, args.limit)
            _, m = timed([exe, "run", "-M", bam, fa, os.path.join(d, "M")], env, args.limit)
            sums = {k: sha(os.path.join(d, k + ".sv.txt")) for k in "BPM"}
            out["reps"].append(dict(base=b, plain=p, marking=m, sha256_sv_txt=sums, plain_equals_base=sums["B"] == sums["P"],
                                    marking_extra_wall_s=round(m["wall_s"] - p["wall_s"], 3)))
            if not out["reps"][-1]["plain_equals_base"]:
                raise RuntimeError("run without -M does not write the base's table")
        walls = lambda k: [r[k]["wall_s"] for r in out["reps"]]  # noqa: E731
        out["summary"] = dict(base_wall_s=walls("base"), plain_wall_s=walls("plain"), marking_wall_s=walls("marking"),
                              plain_within_base_spread=min(walls("plain")) <= max(walls("base")),
                              decode_lap_s=[r["marking"]["laps_s"].get("bam_read(wait)+gpu_inflate+decode") for r in out["reps"]],
                              markdup_lap_s=[r["marking"]["laps_s"].get("gpu_markdup+scan(wait h2d+kernels)") for r in out["reps"]],
                              scan_lap_s_without=[r["plain"]["laps_s"].get("gpu_scan(wait h2d+kernels)") for r in out["reps"]])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(out=os.path.relpath(args.out, ROOT), summary=out.get("summary"))))


if __name__ == "__main__":
    main()
