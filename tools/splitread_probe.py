#!/usr/bin/env python3
"""What `seeksv run -A` costs.  The sample is tools/pairdup_probe.py's: the human-only synthetic shape at --frac of the genome, coordinate
sorted.  Then, --reps times and alternating, each command a process of its own under its own time limit,
  plain       BASE run sorted.bam ref.fa P
  splitread   seeksv run -A sorted.bam ref.fa A
BASE is --base-exe, a `seeksv` built from the commit before the stage, or this build when none is given (recorded).  Per command: wall clock exec to exit,
cpu_s, the SSV_TIMING laps - the decode's and, for -A, the scans' and the finish's -, the closing line's six counts, the kernel time of the splitread_scan /
splitread_finish groups and the candidate store's bytes.  The generator plants NO supplementary records: that leg times the select over every record of the
sample plus the gather, the sort and the pairing of all one-side-clipped reads, none of which pairs (every name comes once).  A second leg therefore goes
through the library: --reads named reads as SAM text in three batches through the device decoder in its default form, every 16th a primary (60M40S) plus a
hard-clipped supplementary record (60H40M) - a session whose names do pair: the two groups' kernel time, the wall clock of the scans and of the finish, the
counts.  No pass or fail threshold: one JSON document, to --out.
usage: python tools/splitread_probe.py [--frac F] [--reps R] [--limit SECONDS] [--base-exe PATH] [--reads N] [--out profiles/splitread.json]"""
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
from seeksv_amd import synth  # noqa: E402

COUNTS = ("pairs", "pairs_borrowed", "candidates", "hard_clipped", "dropped_no_carrier", "dropped_length")


def timed(cmd, env, limit):
    r, d = cp.timed(cmd, env, limit)
    m = re.search(r"\[seeksv\] -A: (\d+) pairs \((\d+) with a borrowed seq\) of (\d+) one-side-clipped records \((\d+) hard-clipped\); dropped at the pairing: (\d+) without a record that "
                  r"carries the read, (\d+) for unequal read lengths", r.stderr)
    if m:
        d["counts"] = {k: int(m.group(i + 1)) for i, k in enumerate(COUNTS)}
    m = re.search(r"\(-A kernel time: splitread_scan ([0-9.e+-]+) ms in (\d+) launches, splitread_finish ([0-9.e+-]+) ms in (\d+) launches; the scans held the pump for ([0-9.e+-]+) s; "
                  r"candidate store (\d+) bytes\)", r.stderr)
    if m:
        d["splitread_kernel_ms"] = dict(splitread_scan=float(m.group(1)), scan_launches=int(m.group(2)), splitread_finish=float(m.group(3)), finish_launches=int(m.group(4)))
        d["scans_held_the_pump_s"] = float(m.group(5))
        d["candidate_store_bytes"] = int(m.group(6))
    return d


def pairing_leg(n_reads, reps, seed=13):
    """the library leg -> dict: per repetition the kernel ms of the two groups, the wall clock of the three scans and of the finish, the counts"""
    from seeksv_amd.device import Context
    rng = random.Random(seed)
    read = "".join(rng.choice("ACGT") for _ in range(100))
    qual = "I" * 100
    lines = []
    for k in range(n_reads):
        p = rng.randrange(1000, 200000000)
        if k % 16 == 15:
            lines.append(f"n{k}\t0\tc0\t{p}\t60\t60M40S\t*\t0\t0\t{read}\t{qual}\nn{k}\t2048\tc0\t{p + 5000}\t60\t60H40M\t*\t0\t0\t{read[60:]}\t{qual[60:]}\n")
        else:
            lines.append(f"n{k}\t0\tc0\t{p}\t60\t100M\t*\t0\t0\t{read}\t{qual}\n")
    third = (len(lines) + 2) // 3
    texts = ["".join(lines[a:a + third]).encode() for a in range(0, len(lines), third)]
    out = dict(reads=n_reads, split_reads_planted=n_reads // 16, text_bytes=sum(len(t) for t in texts), batches=len(texts), reps=[])
    with Context(0) as ctx:
        for _ in range(reps):
            ctx.prof_enable(1)
            ctx.prof_reset()
            ctx.samdec_begin(["c0"])
            ctx.samdec_any_order(True)
            ctx.samdec_sorted(False)
            ctx.rt_begin_original(1, ["c0"])
            scan_wall = 0.0
            for k, t in enumerate(texts):
                b = ctx.samdec_decode(t, last=k == len(texts) - 1)
                nm = ctx.samdec_names()
                t0 = time.perf_counter()
                ctx.rt_scan(b, nm)
                scan_wall += time.perf_counter() - t0
            t0 = time.perf_counter()
            r = ctx.rt_finish()
            finish_wall = time.perf_counter() - t0
            st = ctx.rt_original_stats()
            groups = {g: {k: round(v, 4) if isinstance(v, float) else v for k, v in ctx.prof_get(g).items()} for g in ("splitread_scan", "splitread_finish", "bam_decode")}
            ctx.prof_enable(0)
            out["reps"].append(dict(scan_wall_s=round(scan_wall, 4), finish_wall_s=round(finish_wall, 4), pairs=int(r.n_pairs), groups=groups, stats=st))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=1 / 64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--base-exe", default=None)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splitread.json"))
    args = ap.parse_args()
    exe = os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
    base = args.base_exe or exe
    tumor = synth.Workload(depth=60.0, genome_frac=args.frac, n_sv=max(8, round(10000 * args.frac)), unmap_permille=20)
    where = bench.room_for(int(tumor.n_total * 600 + tumor.genome_len * 1.1))
    d = tempfile.mkdtemp(prefix="ssv_splitread_", dir=where)
    env = dict(os.environ, SSV_TIMING="1")
    env.pop("SSV_BGZF_LEVEL", None)
    out = dict(what="seeksv run (the base build) against seeksv run -A (this build) on one coordinate-sorted sample without supplementary records; then a library session whose names pair",
               genome_frac=args.frac, records=tumor.n_total, cpus=bench.effective_cpus(), base_is_an_earlier_build=args.base_exe is not None, reps=[])
    try:
        t0 = time.perf_counter()
        bam, fa = os.path.join(d, "sorted.bam"), os.path.join(d, "ref.fa")
        bench.write_workload_bam(tumor, bam, 6)
        tumor.write_fasta(fa, bench.effective_cpus())
        out["files_made_s"] = round(time.perf_counter() - t0, 1)
        out["bam_bytes"] = os.path.getsize(bam)
        for rep in range(args.reps):
            p = timed([base, "run", bam, fa, os.path.join(d, "P")], env, args.limit)
            a = timed([exe, "run", "-A", bam, fa, os.path.join(d, "A")], env, args.limit)
            sums = {k: cp.sha(os.path.join(d, k + ".sv.txt")) for k in ("P", "A")}
            out["reps"].append(dict(plain=p, splitread=a, sha256_sv_txt=sums, extra_wall_s=round(a["wall_s"] - p["wall_s"], 3)))
        col = lambda k, f: [r[k].get(f) for r in out["reps"]]  # noqa: E731
        lap = lambda k, name: [sum(v for n, v in r[k]["laps_s"].items() if name in n) for r in out["reps"]]  # noqa: E731
        out["summary"] = dict(plain_wall_s=col("plain", "wall_s"), splitread_wall_s=col("splitread", "wall_s"), extra_wall_s=[r["extra_wall_s"] for r in out["reps"]],
                              decode_lap_s=lap("splitread", "gpu_inflate+decode"), scan_lap_s=lap("splitread", "gpu_splitread_scan"), finish_lap_s=lap("splitread", "splitread (run -A"),
                              kernel_ms=col("splitread", "splitread_kernel_ms"), scans_held_the_pump_s=col("splitread", "scans_held_the_pump_s"),
                              candidate_store_bytes=col("splitread", "candidate_store_bytes"), counts=col("splitread", "counts"))
        if args.reads > 0:
            out["library_leg"] = pairing_leg(args.reads, args.reps)
            out["summary"]["library_leg"] = [dict(scan_wall_s=r["scan_wall_s"], finish_wall_s=r["finish_wall_s"], kernel_ms={g: v["total_ms"] for g, v in r["groups"].items()},
                                                  pairs=r["pairs"], store_bytes=r["stats"]["store_bytes"]) for r in out["library_leg"]["reps"]]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(out=os.path.relpath(args.out, ROOT), summary=out.get("summary"))))


if __name__ == "__main__":
    main()
