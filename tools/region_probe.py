#!/usr/bin/env python3
"""What `seeksv run -L` / `-X` cost.  The sample is tools/coordsort_probe.py's: bench.py's config-5 tumor shape without the virus contig (human at
60x, 2 % of the records in pairs with one unmapped end, coordinate sorted) at --frac of the genome, written with bench.py's own writer, and the same records
permuted with a seeded generator as a second BAM.  Three BED files are made from the BAM's header: `all` (every contig from end to end: every record is kept -
the cost of the flags and scan alone, since ssv_region_retain copies as ssv_batch_retain does), `targets` (300-base targets, evenly spaced, about 2 % of the
genome) and `exclude` (10,000-base regions, evenly spaced, about 1 %).  Then, --reps times and alternating, each command a process of its own:
  plain     BASE run sorted.bam ref.fa P          (BASE: --base-exe, a `seeksv` built from the commit before the stage, or this build when none is given)
  all       seeksv run -L all.bed sorted.bam ref.fa A
  targets   seeksv run -L targets.bed sorted.bam ref.fa T
  exclude   seeksv run -X exclude.bed sorted.bam ref.fa X
  unsorted  seeksv run -u -L targets.bed shuffled.bam ref.fa U
each with SSV_TIMING=1 and a time limit of its own: wall clock exec to exit, cpu_s, the SSV_TIMING laps, the resident records and bytes, the closing line
(kept of records, regions, contigs), the kernel time and launches of the region_select / region_gather groups, and the table's sha256.  No pass or fail
threshold: one JSON document, to --out.
usage: python tools/region_probe.py [--frac F] [--reps R] [--limit SECONDS] [--base-exe PATH] [--out profiles/region_select.json]"""
import argparse
import gzip
import json
import os
import re
import shutil
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import coordsort_probe as cp  # noqa: E402
from seeksv_amd import synth  # noqa: E402


def bam_contigs(path):
    """-> [(name, length)] of a BAM's header"""
    with gzip.open(path, "rb") as f:
        head = f.read(8)
        l_text, = struct.unpack_from("<i", head, 4)
        f.read(l_text)
        n_ref, = struct.unpack("<i", f.read(4))
        out = []
        for _ in range(n_ref):
            l, = struct.unpack("<i", f.read(4))
            name = f.read(l)[:-1].decode()
            out.append((name, struct.unpack("<i", f.read(4))[0]))
    return out


def write_bed(path, contigs, width, step):
    """regions of `width` bases every `step` bases on every contig (step None: the whole contig) -> (regions, bases covered)"""
    n = covered = 0
    with open(path, "w") as f:
        for name, length in contigs:
            starts = [0] if step is None else range(step // 2, length, step)
            for s in starts:
                e = length if step is None else min(length, s + width)
                if e > s:
                    f.write(f"{name}\t{s}\t{e}\n")
                    n += 1
                    covered += e - s
    return n, covered


def timed(cmd, env, limit):
    r, d = cp.timed(cmd, env, limit)
    m = re.search(r"\[seeksv\] -([LX]): kept (\d+) of (\d+) records \((\d+) regions on (\d+) contigs\)", r.stderr)
    if m:
        d["kept"] = dict(option="-" + m.group(1), kept=int(m.group(2)), records=int(m.group(3)), regions=int(m.group(4)), contigs=int(m.group(5)))
    m = re.search(r"\(-[LX] kernel time: region_select ([0-9.e+-]+) ms in (\d+) launches, region_gather ([0-9.e+-]+) ms in (\d+) launches\)", r.stderr)
    if m:
        d["region_kernel_ms"] = dict(region_select=float(m.group(1)), select_launches=int(m.group(2)), region_gather=float(m.group(3)), gather_launches=int(m.group(4)))
    return r, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=1 / 64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--base-exe", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_select.json"))
    args = ap.parse_args()
    exe = os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
    base = args.base_exe or exe
    tumor = synth.Workload(depth=60.0, genome_frac=args.frac, n_sv=max(8, round(10000 * args.frac)), unmap_permille=20)
    where = bench.room_for(int(tumor.n_total * 1200 + tumor.genome_len * 1.1))
    d = tempfile.mkdtemp(prefix="ssv_region_", dir=where)
    env = dict(os.environ, SSV_TIMING="1")
    env.pop("SSV_BGZF_LEVEL", None)
    out = dict(what="seeksv run against run -L (everything kept; 2 % of the genome in 300-base targets), run -X (1 %) and run -u -L on the same records in a seeded random order",
               genome_frac=args.frac, records=tumor.n_total, cpus=bench.effective_cpus(), base_is_an_earlier_build=args.base_exe is not None, reps=[])
    try:
        t0 = time.perf_counter()
        bam, shuffled, fa = os.path.join(d, "sorted.bam"), os.path.join(d, "shuffled.bam"), os.path.join(d, "ref.fa")
        bench.write_workload_bam(tumor, bam, 6)
        out["records_shuffled"] = cp.shuffle_bam(bam, shuffled, 4096)
        tumor.write_fasta(fa, bench.effective_cpus())
        contigs = bam_contigs(bam)
        genome = sum(l for _, l in contigs)
        beds = {}
        for tag, width, step in (("all", 0, None), ("targets", 300, 15000), ("exclude", 10000, 1000000)):
            path = os.path.join(d, tag + ".bed")
            n, covered = write_bed(path, contigs, width, step)
            beds[tag] = path
            out.setdefault("beds", {})[tag] = dict(regions=n, bases=covered, share_of_genome=round(covered / genome, 5))
        out["files_made_s"] = round(time.perf_counter() - t0, 1)
        out["contigs"] = len(contigs)
        commands = (("plain", [base, "run", bam, fa], "P"), ("all", [exe, "run", "-L", beds["all"], bam, fa], "A"), ("targets", [exe, "run", "-L", beds["targets"], bam, fa], "T"),
                    ("exclude", [exe, "run", "-X", beds["exclude"], bam, fa], "X"), ("unsorted", [exe, "run", "-u", "-L", beds["targets"], shuffled, fa], "U"))
        for rep in range(args.reps):
            one = {}
            for tag, cmd, prefix in commands:
                _, one[tag] = timed(cmd + [os.path.join(d, prefix)], env, args.limit)
                one[tag]["sha256_sv_txt"] = cp.sha(os.path.join(d, prefix + ".sv.txt"))
            one["all_equals_plain"] = one["all"]["sha256_sv_txt"] == one["plain"]["sha256_sv_txt"]
            out["reps"].append(one)
        pick = lambda tag, key: [r[tag].get(key) for r in out["reps"]]  # noqa: E731
        out["summary"] = {tag: dict(wall_s=pick(tag, "wall_s"), kept=pick(tag, "kept"), region_kernel_ms=pick(tag, "region_kernel_ms"),
                                    resident=pick(tag, "resident")) for tag, _, _ in commands}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(out=os.path.relpath(args.out, ROOT), summary=out.get("summary"))))


if __name__ == "__main__":
    main()
