#!/usr/bin/env python3
"""`getsv -F` on SAM text at a user's size: tools/readthrough_bench.py's seeded read-through file written twice, as BAM and as SAM text (the same
records; the text's numbers are zero-padded so that the file can be written with numpy), then `seeksv getsv -F` on the text and `seeksv getsv -Z -F` on the
BAM - the comparison base - alternating, --repeat times each.  Per run: the `readthrough (-F)` phase (SSV_TIMING=1) and, for the text, its bytes per second.
Kernel and copy times come from ONE traced run of the binary on the files this tool leaves in --out (tools/samdec_kstats.py sums it up):

    SSV_CLEAN_EXIT=1 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR/prof -o t -- \
        seeksv_amd/bin/seeksv getsv -F DIR/f.sam DIR/s.clip.bam DIR/s.bam DIR/s.clip.gz DIR/o.sv DIR/o.fq
    python tools/samdec_kstats.py DIR/prof <bytes of f.sam>

Kernel trace AND memory-copy trace, no counters: the condition to read off - the sum of the k_sam_* kernels per chunk against the time that chunk's text
takes to cross the host link - needs both from the same run.  SSV_CLEAN_EXIT=1: the command otherwise leaves through _exit, and the profiler, which writes
its files when the process ends the regular way, writes nothing.  The binary itself, not this driver: the trace then holds one process.

usage: python tools/samdec_bench.py [--records N] [--split 0.05] [--out DIR] [--json FILE] [--repeat 3] [--only-text] [--chunk-kb KB]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import readthrough_bench as RB  # noqa: E402
from seeksv_amd import host, synth  # noqa: E402

L = RB.L
NT16 = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)


def digits(v, width):
    """[m] integers -> [m, width] ASCII digits, zero-padded"""
    v = np.asarray(v, np.int64)
    return ((v[:, None] // 10 ** np.arange(width - 1, -1, -1)[None, :]) % 10 + 48).astype(np.uint8)


def text_of(b, first, names):
    """one batch of RB.f_batches as SAM record text (bytes).  Split pairs (2j, 2j + 1) share the name s<2j>, as the BAM writer names them."""
    m = len(b["tid"])
    idx = np.arange(first, first + m)
    split = b["n_cigar"] == 2
    name_no = np.where(split, idx // 2 * 2, idx)
    tab = np.full((m, 1), 9, np.uint8)
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    flag = b["flag"].astype(np.int64)  # (in hex: a decimal FLAG must not begin with 0 - libbam reads that as octal)
    a = np.concatenate([np.full((m, 1), ord("s"), np.uint8), digits(name_no, 10), tab, np.broadcast_to(np.frombuffer(b"0x", np.uint8), (m, 2)),
                        hexd[(flag >> 4) & 15][:, None], hexd[flag & 15][:, None], tab], axis=1)
    co = b["cigar_off"].astype(np.int64)
    c0 = b["cigar"][co]
    c1 = b["cigar"][np.minimum(co + 1, len(b["cigar"]) - 1)]
    ops = np.frombuffer(b"MIDNSHP=X", np.uint8)
    cig_split = np.concatenate([digits(c0 >> 4, 2), ops[c0 & 15][:, None], digits(c1 >> 4, 2), ops[c1 & 15][:, None]], axis=1)
    cig_whole = np.concatenate([digits(c0 >> 4, 5), ops[c0 & 15][:, None]], axis=1)
    cig = np.where(split[:, None], cig_split, cig_whole)
    sq = b["seqqual"].reshape(m, L // 2 + L)
    packed = sq[:, :L // 2]
    seq = np.stack([NT16[packed >> 4], NT16[packed & 15]], axis=2).reshape(m, L)
    qual = sq[:, L // 2:] + 33
    tail = np.frombuffer(b"\t*\t0\t0\t", np.uint8)
    c = np.concatenate([tab, digits(b["pos"].astype(np.int64) + 1, 10), tab, digits(b["mapq"], 2), tab, cig, np.broadcast_to(tail, (m, len(tail))), seq, tab, qual,
                        np.full((m, 1), 10, np.uint8)], axis=1)
    nm = [np.frombuffer(n.encode(), np.uint8) for n in names]
    nlen = np.array([len(x) for x in nm], np.int64)[b["tid"]]
    wa, wc = a.shape[1], c.shape[1]
    start = np.zeros(m + 1, np.int64)
    start[1:] = np.cumsum(wa + nlen + wc)
    out = np.empty(int(start[-1]), np.uint8)
    out[start[:-1, None] + np.arange(wa)[None, :]] = a
    for t, x in enumerate(nm):
        rows = np.flatnonzero(b["tid"] == t)
        out[start[rows, None] + wa + np.arange(len(x))[None, :]] = x[None, :]
    out[(start[:-1] + wa + nlen)[:, None] + np.arange(wc)[None, :]] = c
    return out.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--split", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--only-text", action="store_true")
    ap.add_argument("--chunk-kb", default=None)
    a = ap.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="samdec_bench_")
    os.makedirs(d, exist_ok=True)
    w = synth.Workload(genome_frac=1 / 1024, depth=30, n_sv=40)
    lens = [int(x) for x in w.lens]
    bam, fbam, fsam = os.path.join(d, "s.bam"), os.path.join(d, "f.bam"), os.path.join(d, "f.sam")
    t0 = time.perf_counter()
    if not os.path.exists(bam):
        host.write_bam(bam, w.names, w.lens, [w.generate_host(0, w.n_total)])
    if not os.path.exists(fbam):
        host.write_bam(fbam, w.names, w.lens, RB.f_batches(a.records, a.split, w.names, lens, 17, per=1 << 20))  # (the same batches as the text below: the generator draws per batch)
    if not os.path.exists(fsam):
        with open(fsam, "wb") as f:
            f.write(("@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(w.names, lens))).encode())
            first = 0
            for b in RB.f_batches(a.records, a.split, w.names, lens, 17, per=1 << 20):
                f.write(text_of(b, first, list(w.names)))
                first += len(b["tid"])
    fa = os.path.join(d, "ref.fa")
    with open(fa, "w") as f:
        f.write(w.reference_fasta())
    p = os.path.join(d, "s")
    subprocess.run([RB.SEEKSV, "getclip", "-o", p, bam], check=True, capture_output=True)
    subprocess.run([RB.SEEKSV, "realign", fa, p + ".clip.fq.gz", p + ".clip.bam"], check=True, capture_output=True)
    out = dict(records=a.records, split=a.split, bam_bytes=os.path.getsize(fbam), text_bytes=os.path.getsize(fsam), generate_s=round(time.perf_counter() - t0, 1), runs=[])
    env = dict(os.environ, SSV_TIMING="1")
    if a.chunk_kb:
        env["SSV_SAM_CHUNK_KB"] = a.chunk_kb
    args = [p + ".clip.bam", bam, p + ".clip.gz"]
    forms = [("text", [], fsam)] + ([] if a.only_text else [("bam_Z", ["-Z"], fbam)])
    sv = {}
    for k in range(a.repeat):
        for tag, mode, ff in forms:  # alternating
            o = os.path.join(d, f"o.{tag}.sv")
            r, _ = RB.timed([RB.SEEKSV, "getsv"] + mode + ["-F", ff] + args + [o, os.path.join(d, "o.fq")], env)
            ph = r["phases_s"].get("readthrough (-F)")
            run = dict(form=tag, run=k, readthrough_F_s=ph, total_s=r["total_s"], cpu_s=r["cpu_s"], records_per_s=round(a.records / ph) if ph else None)
            if tag == "text" and ph:
                run["text_GB_per_s"] = round(out["text_bytes"] / ph / 1e9, 2)
            sv[tag] = [l for l in open(o) if not l.startswith("@")]
            out["runs"].append(run)
            print(f"[samdec_bench] {json.dumps(run)}", file=sys.stderr, flush=True)
    if len(sv) == 2:
        out["sv_rows"] = len(sv["text"])
        out["sv_equal"] = sv["text"] == sv["bam_Z"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
