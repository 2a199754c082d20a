#!/usr/bin/env python3
"""Summary of a `rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv` run of `seeksv getsv -F <SAM text>` (or `seeksv getclip <SAM text>`): per k_sam_* kernel the
number of launches and the total time, their sum per chunk (launches of k_sam_count = chunks), and next to it the host-to-device copies of the same run
(bytes, time, GB/s) - the time the text takes to cross the host link.

usage: python tools/samdec_kstats.py DIR [TEXT_BYTES]     (the directory rocprofv3 wrote into: *_kernel_trace.csv, *_memory_copy_trace.csv anywhere below it)"""
import csv
import glob
import os
import sys


def rows(d, suffix):
    out = []
    for p in glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True):
        with open(p, newline="") as f:
            out += list(csv.DictReader(f))
    return out


def main():
    d = sys.argv[1]
    kern = {}
    for r in rows(d, "kernel_trace.csv"):
        name = r.get("Kernel_Name", "")
        dt = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        key = name.split("(")[0].split("<")[0].replace("ssv::", "").replace("void ", "").strip()
        k = kern.setdefault(key, [0, 0.0])
        k[0] += 1
        k[1] += dt
    sam = {k: v for k, v in kern.items() if k.startswith("k_sam_")}
    chunks = max(1, sam.get("k_sam_count", [1])[0])
    total = sum(v[1] for v in sam.values())
    for k, v in sorted(sam.items(), key=lambda kv: -kv[1][1]):
        print(f"{k:16s} {v[0]:5d} launches {v[1]:9.3f} ms  {v[1] / chunks:8.3f} ms/chunk")
    scans = sum(v[1] for k, v in kern.items() if k.startswith("k_scan_"))
    print(f"k_sam_* sum      {total:9.3f} ms over {chunks} chunks = {total / chunks:.3f} ms/chunk   (all k_scan_* of the run, the -F kernels' included: {scans:.3f} ms)")
    tid = {k: v for k, v in kern.items() if k.startswith("k_tid_")}  # (a coordinate-sorted original, ssv_samdec_sorted: the contig lists behind the decode)
    if tid:
        print(f"k_tid_* sum      {sum(v[1] for v in tid.values()):9.3f} ms over {chunks} chunks = {sum(v[1] for v in tid.values()) / chunks:.3f} ms/chunk")
    rt = sum(v[1] for k, v in kern.items() if k.startswith("k_rt_"))
    print(f"k_rt_* sum       {rt:9.3f} ms")
    dirs = {}
    for r in rows(d, "memory_copy_trace.csv"):
        dt = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        k = dirs.setdefault(r.get("Direction", "?").replace("MEMORY_COPY_", ""), [0, 0.0, 0, 0.0])
        k[0] += 1
        k[1] += dt
        if dt > 0.5:  # the chunks of text (everything else is a few bytes)
            k[2] += 1
            k[3] += dt
    for name, k in sorted(dirs.items()):
        print(f"copies {name:18s} {k[0]:6d} in {k[1]:9.3f} ms; above 0.5 ms each: {k[2]} in {k[3]:.3f} ms = {k[3] / chunks:.3f} ms/chunk")
    if len(sys.argv) > 2 and "HOST_TO_DEVICE" in dirs and dirs["HOST_TO_DEVICE"][3] > 0:
        nb = int(sys.argv[2])
        print(f"text {nb} bytes over the host link in {dirs['HOST_TO_DEVICE'][3]:.3f} ms: {nb / dirs['HOST_TO_DEVICE'][3] / 1e6:.1f} GB/s")

if __name__ == "__main__":
    main()
