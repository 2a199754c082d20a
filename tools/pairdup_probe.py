#!/usr/bin/env python3
"""What `seeksv run -D` costs.  The sample is tools/coordsort_probe.py's: the human-only synthetic shape at --frac of the genome, coordinate
sorted, and the same records permuted with a seeded generator.  Then, --reps times and alternating, each command a process of its own,
  plain        BASE run sorted.bam ref.fa P            unsorted       BASE run -u shuffled.bam ref.fa U
  pairs        seeksv run -D sorted.bam ref.fa D       unsorted_pairs seeksv run -u -D shuffled.bam ref.fa UD
BASE is --base-exe, a `seeksv` built from the commit before the stage (the commands without -D are compared as that build runs them), or this build when none
is given (recorded).  Per command: wall clock exec to exit, cpu_s, the SSV_TIMING laps; for -D the closing line's counts (pairs marked, groups, pairs, records
that take part), the kernel time of the pairdup_ends / pairdup_join / pairdup_mark groups and the bytes of rows, keys and indices beside the records; for -u
what tools/coordsort_probe.py records.  The synthetic sample's read names are one per record (bench.py's writer numbers the records), so no two of its records are
mates by name: those commands time the retention with rows, the compaction, the name sort and the join, and never reach the pair sorts.  A second leg
therefore goes through the library: --pairs pairs of 20-base reads at random places of one contig, every 16th a copy of the pair before it with 5 bases
soft-clipped, as SAM text in read-name order through the device decoder, ssv_pairdup_retain and one ssv_pairdup_mark - the three groups' kernel time, the call's
wall clock, the counts.  No pass or fail threshold: one JSON document, to --out.
usage: python tools/pairdup_probe.py [--frac F] [--reps R] [--limit SECONDS] [--base-exe PATH] [--pairs N] [--out profiles/pairdup.json]"""
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


def timed(cmd, env, limit):
    r, d = cp.timed(cmd, env, limit)
    m = re.search(r"\[seeksv\] -D: marked (\d+) duplicate pairs \((\d+) groups of two or more\) of (\d+) pairs; (\d+) of (\d+) records that take part have no mate by name, (\d+) records", r.stderr)
    if m:
        d["marked"] = dict(pairs_marked=int(m.group(1)), records_marked=2 * int(m.group(1)), groups_many=int(m.group(2)), pairs=int(m.group(3)), unpaired=int(m.group(4)),
                           taking_part=int(m.group(5)), records=int(m.group(6)))
    m = re.search(r"\(-D kernel time: pairdup_ends ([0-9.e+-]+) ms in (\d+) launches, pairdup_join ([0-9.e+-]+) ms in (\d+) launches, pairdup_mark ([0-9.e+-]+) ms in (\d+) launches; "
                  r"resident at the peak beside the records: (\d+) bytes of rows, (\d+) bytes of keys and indices\)", r.stderr)
    if m:
        d["pairdup_kernel_ms"] = dict(pairdup_ends=float(m.group(1)), pairdup_join=float(m.group(3)), pairdup_mark=float(m.group(5)),
                                      total=round(float(m.group(1)) + float(m.group(3)) + float(m.group(5)), 3), launches=int(m.group(2)) + int(m.group(4)) + int(m.group(6)))
        d["pairdup_extra_bytes"] = dict(rows=int(m.group(7)), keys_and_indices=int(m.group(8)))
    return d


def mark_leg(n_pairs, reps, seed=11):
    """the library leg -> dict: per repetition the kernel ms and launches of the three groups, the wall clock of ssv_pairdup_mark, its counts"""
    from seeksv_amd.device import Context
    rng = random.Random(seed)
    seq, hi, lo = "ACGTACGTACGTACGTACGT", "I" * 20, "5" * 20
    lines, p1 = [], 0
    for k in range(n_pairs):
        copy = k % 16 == 15
        if not copy:
            p1 = rng.randrange(1000, 200000000)
        a, cig, q = (p1 + 5, "5S15M", lo) if copy else (p1, "20M", hi)
        lines.append(f"n{k}\t97\tc0\t{a + 1}\t60\t{cig}\tc0\t{p1 + 201}\t0\t{seq}\t{q}\nn{k}\t145\tc0\t{p1 + 201}\t60\t20M\tc0\t{a + 1}\t0\t{seq}\t{q}\n")
    text = "".join(lines).encode()
    out = dict(pairs=n_pairs, copies_planted=n_pairs // 16, text_bytes=len(text), reps=[])
    chunk = 64 << 20
    with Context(0) as ctx:
        for _ in range(reps):
            ctx.prof_enable(1)
            ctx.prof_reset()
            ctx.samdec_begin(["c0"])
            ctx.samdec_any_order(True)
            ctx.samdec_sorted(True)
            batches = []
            for at in range(0, len(text), chunk):
                b = ctx.samdec_decode(text[at:at + chunk], last=at + chunk >= len(text))
                batches.append(ctx.pairdup_retain(b, ctx.samdec_names()))
            t0 = time.perf_counter()
            st = ctx.pairdup_mark(batches)
            wall = time.perf_counter() - t0
            groups = {g: {k: round(v, 4) if isinstance(v, float) else v for k, v in ctx.prof_get(g).items()} for g in ("pairdup_ends", "pairdup_join", "pairdup_mark")}
            ctx.prof_enable(0)
            for b in batches:
                ctx.batch_release(b)
            out["reps"].append(dict(batches=len(batches), mark_wall_s=round(wall, 4), groups=groups, stats=st))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=1 / 64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--base-exe", default=None)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairdup.json"))
    args = ap.parse_args()
    exe = os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
    base = args.base_exe or exe
    tumor = synth.Workload(depth=60.0, genome_frac=args.frac, n_sv=max(8, round(10000 * args.frac)), unmap_permille=20)
    where = bench.room_for(int(tumor.n_total * 1200 + tumor.genome_len * 1.1))
    d = tempfile.mkdtemp(prefix="ssv_pairdup_", dir=where)
    env = dict(os.environ, SSV_TIMING="1")
    env.pop("SSV_BGZF_LEVEL", None)
    out = dict(what="seeksv run / run -u (the base build) against seeksv run -D / run -u -D (this build) on one sample, sorted and in a seeded random order", genome_frac=args.frac,
               records=tumor.n_total, cpus=bench.effective_cpus(), base_is_an_earlier_build=args.base_exe is not None, reps=[])
    try:
        t0 = time.perf_counter()
        bam, shuffled, fa = os.path.join(d, "sorted.bam"), os.path.join(d, "shuffled.bam"), os.path.join(d, "ref.fa")
        bench.write_workload_bam(tumor, bam, 6)
        out["records_shuffled"] = cp.shuffle_bam(bam, shuffled, 4096)
        tumor.write_fasta(fa, bench.effective_cpus())
        out["files_made_s"] = round(time.perf_counter() - t0, 1)
        out["bam_bytes"] = dict(sorted=os.path.getsize(bam), shuffled=os.path.getsize(shuffled))
        for rep in range(args.reps):
            p = timed([base, "run", bam, fa, os.path.join(d, "P")], env, args.limit)
            dd = timed([exe, "run", "-D", bam, fa, os.path.join(d, "D")], env, args.limit)
            u = timed([base, "run", "-u", shuffled, fa, os.path.join(d, "U")], env, args.limit)
            ud = timed([exe, "run", "-u", "-D", shuffled, fa, os.path.join(d, "UD")], env, args.limit)
            sums = {k: cp.sha(os.path.join(d, k + ".sv.txt")) for k in ("P", "D", "U", "UD")}
            out["reps"].append(dict(plain=p, pairs=dd, unsorted=u, unsorted_pairs=ud, sha256_sv_txt=sums, pairs_extra_wall_s=round(dd["wall_s"] - p["wall_s"], 3),
                                    unsorted_pairs_extra_wall_s=round(ud["wall_s"] - u["wall_s"], 3)))
        col = lambda k, f: [r[k].get(f) for r in out["reps"]]  # noqa: E731
        out["summary"] = dict(plain_wall_s=col("plain", "wall_s"), pairs_wall_s=col("pairs", "wall_s"), unsorted_wall_s=col("unsorted", "wall_s"), unsorted_pairs_wall_s=col("unsorted_pairs", "wall_s"),
                              pairs_lap_s=[r["pairs"]["laps_s"].get("gpu_pair_duplicates") for r in out["reps"]],
                              unsorted_pairs_lap_s=[r["unsorted_pairs"]["laps_s"].get("gpu_pair_duplicates") for r in out["reps"]],
                              pairs_kernel_ms=col("pairs", "pairdup_kernel_ms"), unsorted_pairs_kernel_ms=col("unsorted_pairs", "pairdup_kernel_ms"),
                              pairs_extra_bytes=col("pairs", "pairdup_extra_bytes"), unsorted_pairs_resident_peak_bytes=col("unsorted_pairs", "resident_peak_bytes"),
                              marked=col("pairs", "marked"), unsorted_marked=col("unsorted_pairs", "marked"))
        if args.pairs > 0:
            out["library_leg"] = mark_leg(args.pairs, args.reps)
            out["summary"]["library_leg"] = [dict(mark_wall_s=r["mark_wall_s"], kernel_ms={g: v["total_ms"] for g, v in r["groups"].items()}, pairs_marked=r["stats"]["pairs_marked"]) for r in out["library_leg"]["reps"]]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(out=os.path.relpath(args.out, ROOT), summary=out.get("summary"))))


if __name__ == "__main__":
    main()
