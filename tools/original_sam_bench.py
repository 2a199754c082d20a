#!/usr/bin/env python3
"""`getclip` on the original alignments as SAM text at a user's size: tools/samdec_bench.py's seeded records sorted by (contig, position) and written twice,
as BAM and as SAM text (the same records; one record in twenty is soft-clipped and carries MUNMAP, so it ships bases + qualities AND goes through the
unmapped-pair side channel), then `SSV_TIMING=1 seeksv getclip` on the text and `seeksv getclip -Z` on the BAM - the comparison base - alternating, --repeat
times each.  Per run: the phases, the total, and for the text its bytes per second of the reading phase.  The two forms' clip.gz and clip.fq.gz must be
equal; the side channel's files name their reads differently (the BAM writer numbers them without padding) and are compared by their line counts.
Kernel and copy times come from ONE traced run of the binary on the text this tool leaves in --out (tools/samdec_kstats.py sums it up):

    SSV_CLEAN_EXIT=1 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR/prof -o t -- seeksv_amd/bin/seeksv getclip -o DIR/t DIR/o.sam
    python tools/samdec_kstats.py DIR/prof <bytes of o.sam>

usage: python tools/original_sam_bench.py [--records N] [--split 0.05] [--out DIR] [--json FILE] [--repeat 3] [--chunk-kb KB]
"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import readthrough_bench as RB  # noqa: E402
import samdec_bench as SB  # noqa: E402
from seeksv_amd import host, synth  # noqa: E402

L = RB.L


def sorted_batch(n, split, names, lens):
    """RB.f_batches' records as one batch in (contig, position) order"""
    parts = list(RB.f_batches(n, split, names, lens, 17, per=1 << 20))
    cat = {k: np.concatenate([p[k] for p in parts]) for k in ("tid", "pos", "flag", "mapq", "n_cigar", "l_qseq", "mtid", "mpos", "isize", "xc")}
    c0 = np.concatenate([p["cigar"][p["cigar_off"]] for p in parts])
    c1 = np.concatenate([p["cigar"][np.minimum(p["cigar_off"].astype(np.int64) + 1, len(p["cigar"]) - 1)] for p in parts])
    sq = np.concatenate([p["seqqual"].reshape(-1, L // 2 + L) for p in parts])
    order = np.lexsort((cat["pos"], cat["tid"]))
    cat = {k: v[order] for k, v in cat.items()}
    c0, c1, sq = c0[order], c1[order], sq[order]
    two = cat["n_cigar"] == 2
    keep = np.stack([np.ones(n, bool), two], axis=1).reshape(-1)
    cat["cigar"] = np.stack([c0, c1], axis=1).reshape(-1)[keep]
    cat["cigar_off"] = np.zeros(n, np.uint32)
    cat["cigar_off"][1:] = np.cumsum(cat["n_cigar"][:-1], dtype=np.uint64).astype(np.uint32)
    cat["seq_off"] = np.arange(n, dtype=np.uint64) * (L // 2 + L)
    cat["seqqual"] = sq.reshape(-1)
    return cat


def piece(b, a, e):
    """records [a, e) of a batch as a batch of its own"""
    out = {k: b[k][a:e] for k in ("tid", "pos", "flag", "mapq", "n_cigar", "l_qseq", "mtid", "mpos", "isize", "xc")}
    c_a, c_e = int(b["cigar_off"][a]), int(b["cigar_off"][e - 1]) + int(b["n_cigar"][e - 1])
    out["cigar"] = b["cigar"][c_a:c_e]
    out["cigar_off"] = b["cigar_off"][a:e] - np.uint32(c_a)
    out["seq_off"] = b["seq_off"][a:e] - b["seq_off"][a]
    out["seqqual"] = b["seqqual"][a * (L // 2 + L):e * (L // 2 + L)]
    return out


def gz_lines(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4_000_000)
    ap.add_argument("--split", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--chunk-kb", default=None)
    a = ap.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="original_sam_bench_")
    os.makedirs(d, exist_ok=True)
    w = synth.Workload(genome_frac=1 / 1024, depth=30, n_sv=40)
    lens = [int(x) for x in w.lens]
    bam, sam = os.path.join(d, "o.bam"), os.path.join(d, "o.sam")
    t0 = time.perf_counter()
    if not (os.path.exists(bam) and os.path.exists(sam)):
        b = sorted_batch(a.records, a.split, w.names, lens)
        step = 1 << 20
        host.write_bam(bam, w.names, w.lens, (piece(b, s, min(s + step, a.records)) for s in range(0, a.records, step)))
        with open(sam, "wb") as f:
            f.write(("@HD\tVN:1.0\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(w.names, lens))).encode())
            for s in range(0, a.records, step):
                f.write(SB.text_of(piece(b, s, min(s + step, a.records)), s, list(w.names)))
        del b
    out = dict(records=a.records, split=a.split, bam_bytes=os.path.getsize(bam), text_bytes=os.path.getsize(sam), generate_s=round(time.perf_counter() - t0, 1), runs=[])
    env = dict(os.environ, SSV_TIMING="1")
    if a.chunk_kb:
        env["SSV_SAM_CHUNK_KB"] = a.chunk_kb
    forms = [("text", [], sam), ("bam_Z", ["-Z"], bam)]
    for k in range(a.repeat):
        for tag, mode, ff in forms:  # alternating
            r, _ = RB.timed([RB.SEEKSV, "getclip"] + mode + ["-o", os.path.join(d, tag), ff], env)
            read = r["phases_s"].get("sam_read(wait)+gpu_decode" if tag == "text" else "bam_read(wait)+gpu_inflate+decode")
            run = dict(form=tag, run=k, read_decode_s=read, total_s=r["total_s"], cpu_s=r["cpu_s"], phases_s=r["phases_s"], records_per_s=round(a.records / r["total_s"]))
            if tag == "text" and read:
                run["text_GB_per_s"] = round(out["text_bytes"] / read / 1e9, 2)
            out["runs"].append(run)
            print(f"[original_sam_bench] {json.dumps(run)}", file=sys.stderr, flush=True)
    out["clip_equal"] = all(gz_lines(os.path.join(d, "text" + e)) == gz_lines(os.path.join(d, "bam_Z" + e)) for e in (".clip.gz", ".clip.fq.gz"))
    out["clip_rows"] = gz_lines(os.path.join(d, "text.clip.gz")).count(b"\n")
    out["unmapped_lines"] = {tag: [gz_lines(os.path.join(d, tag + e)).count(b"\n") for e in (".unmapped_1.fq.gz", ".unmapped_2.fq.gz")] for tag in ("text", "bam_Z")}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
