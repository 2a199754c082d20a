#!/usr/bin/env python3
"""What `seeksv run -u` costs.  The sample is bench.py's config-5 tumor shape without the virus contig (human at 60x, 2 % of the records in pairs with
one unmapped end: the shape tools/markdup_probe.py uses, which is coordinate sorted) at --frac of the genome, written with bench.py's own writer; its records are
then read back, permuted with a seeded generator and written as a second BAM.  Then, --reps times and alternating,
  plain     seeksv run sorted.bam ref.fa P
  unsorted  seeksv run -u shuffled.bam ref.fa U
  shortcut  seeksv run -u sorted.bam ref.fa S
each with SSV_TIMING=1 and a time limit of its own: wall clock exec to exit, cpu_s, the SSV_TIMING laps, and for -u the closing line (records, batches in and out, or
"already in coordinate order"), the kernel time of the sort_keys / sort_radix / sort_gather groups and the resident bytes at the peak.  The tables of plain and
unsorted need not be equal byte for byte (records at one place keep the order of the permuted input, not of the sorted file): their sha256 are recorded, nothing
hangs on them.  No pass or fail threshold: one JSON document, to --out.
usage: python tools/coordsort_probe.py [--frac F] [--reps R] [--limit SECONDS] [--out profiles/coordsort.json]"""
import argparse
import gzip
import hashlib
import json
import os
import re
import resource
import shutil
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from seeksv_amd import synth  # noqa: E402

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_block(data, level=1):
    comp = zlib.compressobj(level, zlib.DEFLATED, -15)
    c = comp.compress(data) + comp.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(c) + 25) + c + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def shuffle_bam(src, dst, seed):
    """the records of src in a seeded random order -> dst (the header as it is); -> number of records"""
    data = gzip.open(src, "rb").read()      # BGZF = concatenated gzip members
    l_text, = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, p)
    p += 4
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", data, p)
        p += 8 + l
    starts = []
    at = p
    while at < len(data):
        starts.append(at)
        at += 4 + struct.unpack_from("<i", data, at)[0]
    starts.append(at)
    order = np.random.RandomState(seed).permutation(len(starts) - 1)
    stream = data[:p] + b"".join(data[starts[i]:starts[i + 1]] for i in order.tolist())
    with open(dst, "wb") as f:
        for k in range(0, len(stream), 0xff00):
            f.write(bgzf_block(stream[k:k + 0xff00]))
        f.write(BGZF_EOF)
    return len(starts) - 1


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
    m = re.search(r"\[seeksv\] -u: sorted (\d+) records from (\d+) into (\d+) batches", r.stderr)
    if m:
        d["sorted"] = dict(records=int(m.group(1)), batches_in=int(m.group(2)), batches_out=int(m.group(3)))
    m = re.search(r"\[seeksv\] -u: (\d+) records in (\d+) batches already in coordinate order", r.stderr)
    if m:
        d["already_sorted"] = dict(records=int(m.group(1)), batches=int(m.group(2)))
    m = re.search(r"\(-u kernel time: sort_keys ([0-9.e+-]+) ms in (\d+) launches, sort_radix ([0-9.e+-]+) ms in (\d+) launches, sort_gather ([0-9.e+-]+) ms in (\d+) launches; "
                  r"resident at the peak: (\d+) \+ (\d+) bytes of records, (\d+) bytes of keys and indices\)", r.stderr)
    if m:
        d["sort_kernel_ms"] = dict(sort_keys=float(m.group(1)), sort_radix=float(m.group(3)), sort_gather=float(m.group(5)), total=round(float(m.group(1)) + float(m.group(3)) + float(m.group(5)), 3),
                                   launches=int(m.group(2)) + int(m.group(4)) + int(m.group(6)))
        d["resident_peak_bytes"] = int(m.group(7)) + int(m.group(8)) + int(m.group(9))
    return r, d


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=1 / 256)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coordsort.json"))
    args = ap.parse_args()
    exe = os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
    tumor = synth.Workload(depth=60.0, genome_frac=args.frac, n_sv=max(8, round(10000 * args.frac)), unmap_permille=20)
    where = bench.room_for(int(tumor.n_total * 1200 + tumor.genome_len * 1.1))
    d = tempfile.mkdtemp(prefix="ssv_coordsort_", dir=where)
    env = dict(os.environ, SSV_TIMING="1")
    env.pop("SSV_BGZF_LEVEL", None)
    out = dict(what="seeksv run on a sorted sample against seeksv run -u on the same records in a seeded random order, and -u on the sorted file", genome_frac=args.frac,
               records=tumor.n_total, cpus=bench.effective_cpus(), reps=[])
    try:
        t0 = time.perf_counter()
        bam, shuffled, fa = os.path.join(d, "sorted.bam"), os.path.join(d, "shuffled.bam"), os.path.join(d, "ref.fa")
        bench.write_workload_bam(tumor, bam, 6)
        out["records_shuffled"] = shuffle_bam(bam, shuffled, 4096)
        tumor.write_fasta(fa, bench.effective_cpus())
        out["files_made_s"] = round(time.perf_counter() - t0, 1)
        out["bam_bytes"] = dict(sorted=os.path.getsize(bam), shuffled=os.path.getsize(shuffled))
        for rep in range(args.reps):
            _, p = timed([exe, "run", bam, fa, os.path.join(d, "P")], env, args.limit)
            _, u = timed([exe, "run", "-u", shuffled, fa, os.path.join(d, "U")], env, args.limit)
            _, s = timed([exe, "run", "-u", bam, fa, os.path.join(d, "S")], env, args.limit)
            sums = {k: sha(os.path.join(d, k + ".sv.txt")) for k in "PUS"}
            out["reps"].append(dict(plain=p, unsorted=u, shortcut=s, sha256_sv_txt=sums, shortcut_equals_plain=sums["P"] == sums["S"], unsorted_equals_plain=sums["P"] == sums["U"],
                                    unsorted_extra_wall_s=round(u["wall_s"] - p["wall_s"], 3), shortcut_extra_wall_s=round(s["wall_s"] - p["wall_s"], 3)))
        walls = lambda k: [r[k]["wall_s"] for r in out["reps"]]  # noqa: E731
        out["summary"] = dict(plain_wall_s=walls("plain"), unsorted_wall_s=walls("unsorted"), shortcut_wall_s=walls("shortcut"),
                              sort_lap_s=[r["unsorted"]["laps_s"].get("gpu_coordinate_sort") for r in out["reps"]],
                              shortcut_lap_s=[r["shortcut"]["laps_s"].get("gpu_coordinate_sort") for r in out["reps"]],
                              sort_kernel_ms=[r["unsorted"].get("sort_kernel_ms") for r in out["reps"]],
                              resident_peak_bytes=[r["unsorted"].get("resident_peak_bytes") for r in out["reps"]])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(out=os.path.relpath(args.out, ROOT), summary=out.get("summary"))))


if __name__ == "__main__":
    main()
