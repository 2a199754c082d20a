#!/usr/bin/env python3
"""What `seeksv run -A -S` costs; a sibling of tools/splitread_probe.py, whose sample, timing and parsing it uses.  --reps times and
alternating, each command a process of its own under its own time limit, on the coordinate-sorted synthetic sample at --frac of the genome (it has NO SA
tags: the legs give the cost of the descriptor and of walking every source's fields for nothing):
  base        BASE run -A sorted.bam ref.fa B        (BASE: --base-exe, a `seeksv` built from the commit before the mode; this build when none is given)
  splitread   seeksv run -A sorted.bam ref.fa A
  sa          seeksv run -A -S sorted.bam ref.fa S
Per command: wall clock, the SSV_TIMING laps, the groups' kernel time and launches as the run prints them, the counts, the table's sha256.  A library leg
follows: --reads named reads as SAM text in three batches, every 16th a 60M40S primary whose SA names the 60H40M piece - with the supplementary records
present (every virtual candidate redundant) and absent (every pair from an SA entry).  No pass or fail threshold: one JSON document, to --out.
usage: python tools/splitread_sa_probe.py [--frac F] [--reps R] [--limit SECONDS] [--base-exe PATH] [--reads N] [--out profiles/splitread_sa.json]"""
import argparse
import json
import os
import random
import re
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import coordsort_probe as cp  # noqa: E402
import splitread_probe as sp  # noqa: E402
from seeksv_amd import synth  # noqa: E402

SA_COUNTS = ("sa_tags", "sa_multi", "sa_refused", "virtuals", "sa_redundant", "pairs_from_sa", "sa_dropped_length")


def timed_sa(cmd, env, limit):
    r, d = cp.timed(cmd, env, limit)
    m = re.search(r"\[seeksv\] -S: " + ", ".join(k + r" (\d+)" for k in SA_COUNTS), r.stderr)
    if m:
        d["sa_counts"] = {k: int(m.group(i + 1)) for i, k in enumerate(SA_COUNTS)}
    m = re.search(r"\(-A -S kernel time: splitread_sa_aux ([0-9.e+-]+) ms in (\d+) launches, splitread_sa_scan ([0-9.e+-]+) ms in (\d+) launches, splitread_sa_finish ([0-9.e+-]+) ms in "
                  r"(\d+) launches; the scans held the pump for ([0-9.e+-]+) s; candidate store (\d+) bytes\)", r.stderr)
    if m:
        d["splitread_kernel_ms"] = dict(splitread_sa_aux=float(m.group(1)), aux_launches=int(m.group(2)), splitread_sa_scan=float(m.group(3)), scan_launches=int(m.group(4)),
                                        splitread_sa_finish=float(m.group(5)), finish_launches=int(m.group(6)))
        d["scans_held_the_pump_s"] = float(m.group(7))
        d["candidate_store_bytes"] = int(m.group(8))
    return d


def library_leg(n_reads, reps, with_supplementary, seed=13):
    from seeksv_amd.device import Context
    rng = random.Random(seed)
    read = "".join(rng.choice("ACGT") for _ in range(100))
    qual = "I" * 100
    lines = []
    for k in range(n_reads):
        p = rng.randrange(1000, 200000000)
        if k % 16 == 15:
            lines.append(f"n{k}\t0\tc0\t{p}\t60\t60M40S\t*\t0\t0\t{read}\t{qual}\tNM:i:0\tSA:Z:c0,{p + 5000},+,60S40M,60,0;\n")
            if with_supplementary:
                lines.append(f"n{k}\t2048\tc0\t{p + 5000}\t60\t60H40M\t*\t0\t0\t{read[60:]}\t{qual[60:]}\tNM:i:0\tSA:Z:c0,{p},+,60M40S,60,0;\n")
        else:
            lines.append(f"n{k}\t0\tc0\t{p}\t60\t100M\t*\t0\t0\t{read}\t{qual}\tNM:i:0\n")
    third = (len(lines) + 2) // 3
    texts = ["".join(lines[a:a + third]).encode() for a in range(0, len(lines), third)]
    out = dict(reads=n_reads, split_reads_planted=n_reads // 16, supplementary_records_present=with_supplementary, text_bytes=sum(len(t) for t in texts), batches=len(texts), reps=[])
    with Context(0) as ctx:
        for _ in range(reps):
            ctx.prof_enable(1)
            ctx.prof_reset()
            ctx.samdec_begin(["c0"])
            ctx.samdec_any_order(True)
            ctx.samdec_sorted(False)
            ctx.rt_begin_original_sa(1, ["c0"])
            scan_wall = 0.0
            for k, t in enumerate(texts):
                b = ctx.samdec_decode(t, last=k == len(texts) - 1)
                nm = ctx.samdec_names()
                t0 = time.perf_counter()
                ctx.rt_scan_aux(b, nm, ctx.samdec_aux())
                scan_wall += time.perf_counter() - t0
            t0 = time.perf_counter()
            r = ctx.rt_finish()
            finish_wall = time.perf_counter() - t0
            groups = {g: {k: round(v, 4) if isinstance(v, float) else v for k, v in ctx.prof_get(g).items()} for g in ("splitread_sa_aux", "splitread_sa_scan", "splitread_sa_finish", "bam_decode")}
            ctx.prof_enable(0)
            out["reps"].append(dict(scan_wall_s=round(scan_wall, 4), finish_wall_s=round(finish_wall, 4), pairs=int(r.n_pairs), groups=groups, stats=ctx.rt_original_stats(),
                                    sa_stats=ctx.rt_original_sa_stats()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=1 / 64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--base-exe", default=None)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splitread_sa.json"))
    args = ap.parse_args()
    exe = os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
    base = args.base_exe or exe
    tumor = synth.Workload(depth=60.0, genome_frac=args.frac, n_sv=max(8, round(10000 * args.frac)), unmap_permille=20)
    where = bench.room_for(int(tumor.n_total * 600 + tumor.genome_len * 1.1))
    d = tempfile.mkdtemp(prefix="ssv_splitread_sa_", dir=where)
    env = dict(os.environ, SSV_TIMING="1")
    env.pop("SSV_BGZF_LEVEL", None)
    out = dict(what="seeksv run -A (the base build) against seeksv run -A and run -A -S (this build) on one coordinate-sorted sample without SA tags; then library sessions whose SA tags pair",
               genome_frac=args.frac, records=tumor.n_total, cpus=bench.effective_cpus(), base_is_an_earlier_build=args.base_exe is not None, reps=[])
    try:
        bam, fa = os.path.join(d, "sorted.bam"), os.path.join(d, "ref.fa")
        bench.write_workload_bam(tumor, bam, 6)
        tumor.write_fasta(fa, bench.effective_cpus())
        out["bam_bytes"] = os.path.getsize(bam)
        for rep in range(args.reps):
            b = sp.timed([base, "run", "-A", bam, fa, os.path.join(d, "B")], env, args.limit)
            a = sp.timed([exe, "run", "-A", bam, fa, os.path.join(d, "A")], env, args.limit)
            s = timed_sa([exe, "run", "-A", "-S", bam, fa, os.path.join(d, "S")], env, args.limit)
            sums = {k: cp.sha(os.path.join(d, k + ".sv.txt")) for k in ("B", "A", "S")}
            out["reps"].append(dict(base=b, splitread=a, sa=s, sha256_sv_txt=sums))
        col = lambda k, f: [r[k].get(f) for r in out["reps"]]  # noqa: E731
        lap = lambda k, name: [sum(v for n, v in r[k]["laps_s"].items() if name in n) for r in out["reps"]]  # noqa: E731
        out["summary"] = {k: dict(wall_s=col(k, "wall_s"), decode_lap_s=lap(k, "gpu_inflate+decode"), scan_lap_s=lap(k, "gpu_splitread_scan"), kernel_ms=col(k, "splitread_kernel_ms"),
                                  scans_held_the_pump_s=col(k, "scans_held_the_pump_s")) for k in ("base", "splitread", "sa")}
        if args.reads > 0:
            out["library_leg"] = [library_leg(args.reads, args.reps, True), library_leg(args.reads, args.reps, False)]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(out=os.path.relpath(args.out, ROOT), summary=out.get("summary"))))


if __name__ == "__main__":
    main()
