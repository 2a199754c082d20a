#!/usr/bin/env python3
"""`getsv -F` at a user's size: a seeded read-through BAM (every record 100 bp; a share of them split alignments in pairs, the rest 100M, which the
ends test drops) next to a synthetic sample, then `seeksv getsv` with and without -F on the same inputs, host reader and -Z.  Per run: wall clock,
user + system seconds of the child and its SSV_TIMING=1 phase lines (the -F pass is `readthrough (-F)`).  Where oracle/_ref/seeksv_ref exists the
real reference's `getsv -F` on the same files is timed too (the CPU reference: one thread).  Kernel times: run it again under
`rocprofv3 --kernel-trace --stats -- python tools/readthrough_bench.py --only-z` (a run of its own).

The split pairs share a name through the host writer's naming of records with the mate-unmapped flag (8): records 2j and 2j + 1 are both
"s<2j>" - flag 8 does not take part in FindJunction's filter.

usage: python tools/readthrough_bench.py [--records N] [--split 0.05] [--out DIR] [--json FILE] [--only-z] [--no-ref]
"""
import argparse
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seeksv_amd import host, synth  # noqa: E402

SEEKSV = os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
BAMIDX = os.path.join(ROOT, "oracle", "_ref", "bamidx")
L = 100


def f_batches(n, split, names, lens, seed, per=1 << 22):
    """the read-through file in batches of `per` records, in read order: every record on a random contig (-Z reads it with ssv_bamdec_any_order)"""
    rng = np.random.RandomState(seed)
    nt = len(lens)
    for a in range(0, n, per):
        print(f"[readthrough_bench] writing records {a}..", file=sys.stderr, flush=True)
        m = min(per, n - a)
        idx = np.arange(a, a + m)
        tid = rng.randint(0, nt, m).astype(np.int32)
        pos = (rng.randint(0, 1 << 30, m) % (np.asarray(lens, np.int64)[tid] - 2 * L)).astype(np.int32)
        is_split = ((idx // 2) * 2654435761 % 1000003) < split * 1000003   # pairs (2j, 2j + 1) together
        s = rng.randint(15, L - 15, m).astype(np.uint32)
        first = (idx % 2 == 0)
        # same-strand pairs: the 3'-clipped part first, the 5'-clipped part second; one pair in four on opposite strands, both 5'-clipped
        opp = ((idx // 2) % 4 == 0)
        rev = np.where(opp & ~first, 16, 0)
        c0 = np.where(~is_split, (L << 4) | 0, np.where(first & ~opp, ((L - s) << 4) | 0, (s << 4) | 4)).astype(np.uint32)
        c1 = np.where(~is_split, 0, np.where(first & ~opp, (s << 4) | 4, ((L - s) << 4) | 0)).astype(np.uint32)
        ncig = np.where(is_split, 2, 1).astype(np.uint16)
        cig = np.stack([c0, c1], axis=1).reshape(-1)
        keep = np.stack([np.ones(m, bool), is_split], axis=1).reshape(-1)
        cigar = cig[keep]
        cigar_off = np.zeros(m, np.uint32)
        cigar_off[1:] = np.cumsum(ncig[:-1], dtype=np.uint64).astype(np.uint32)
        acgt = np.array([1, 2, 4, 8], np.uint8)                                  # A C G T in BAM's 4-bit code
        packed = (acgt[rng.randint(0, 4, m * (L // 2))] << 4) | acgt[rng.randint(0, 4, m * (L // 2))]
        sq = np.concatenate([packed.reshape(m, L // 2), np.full((m, L), 30, np.uint8)], axis=1).reshape(-1)
        yield dict(tid=tid, pos=pos, flag=(np.where(is_split, 8, 0) | rev).astype(np.uint16), mapq=np.full(m, 60, np.uint8), n_cigar=ncig,
                   l_qseq=np.full(m, L, np.int32), mtid=np.full(m, -1, np.int32), mpos=np.full(m, -1, np.int32), isize=np.zeros(m, np.int32),
                   cigar_off=cigar_off, cigar=cigar, xc=np.zeros(m, np.uint8), seq_off=(np.arange(m, dtype=np.uint64) * (L // 2 + L)), seqqual=sq)


def timed(cmd, env=None):
    c0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.perf_counter()
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    while True:  # (a line a minute while a long command runs: the reference binary takes many minutes at this size)
        try:
            so, se = p.communicate(timeout=60)
            break
        except subprocess.TimeoutExpired:
            print(f"[readthrough_bench] {os.path.basename(cmd[0])} running for {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)
    r = subprocess.CompletedProcess(cmd, p.returncode, so, se)
    dt = time.perf_counter() - t0
    c1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    assert r.returncode == 0, (cmd, r.stderr[-600:])
    phases = {}
    for line in r.stderr.splitlines():
        if line.startswith("[timing] "):
            try:
                name, sec, _ = line[9:].rsplit(" ", 2)
                phases[name] = round(float(sec), 3)
            except ValueError:
                pass
    return dict(total_s=round(dt, 3), cpu_s=round(c1.ru_utime - c0.ru_utime + c1.ru_stime - c0.ru_stime, 2), phases_s=phases), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200_000_000)
    ap.add_argument("--split", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-z", action="store_true")
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="rt_bench_")
    os.makedirs(d, exist_ok=True)
    w = synth.Workload(genome_frac=1 / 1024, depth=30, n_sv=40)
    bam, fbam = os.path.join(d, "s.bam"), os.path.join(d, "f.bam")
    t0 = time.perf_counter()
    if not os.path.exists(bam):
        host.write_bam(bam, w.names, w.lens, [w.generate_host(0, w.n_total)])
        subprocess.run([BAMIDX, bam], check=False, capture_output=True)
    if not os.path.exists(fbam):
        host.write_bam(fbam, w.names, w.lens, f_batches(a.records, a.split, w.names, [int(x) for x in w.lens], 17))
    fa = os.path.join(d, "ref.fa")
    with open(fa, "w") as f:
        f.write(w.reference_fasta())
    p = os.path.join(d, "s")
    subprocess.run([SEEKSV, "getclip", "-o", p, bam], check=True, capture_output=True)
    subprocess.run([SEEKSV, "realign", fa, p + ".clip.fq.gz", p + ".clip.bam"], check=True, capture_output=True)
    out = dict(records=a.records, split=a.split, f_bytes=os.path.getsize(fbam), sample_records=int(w.n_total), generate_s=round(time.perf_counter() - t0, 1))
    env = dict(os.environ, SSV_TIMING="1")
    args = [p + ".clip.bam", bam, p + ".clip.gz", os.path.join(d, "o.sv"), os.path.join(d, "o.fq")]
    for mode in (["-Z"],) if a.only_z else ([], ["-Z"]):
        tag = "z" if mode else "host"
        out[f"getsv_{tag}"], _ = timed([SEEKSV, "getsv"] + mode + args, env)
        print(f"[readthrough_bench] getsv {tag}: {json.dumps(out[f'getsv_{tag}'])}", file=sys.stderr, flush=True)
        out[f"getsv_F_{tag}"], r = timed([SEEKSV, "getsv"] + mode + ["-F", fbam] + args, env)
        print(f"[readthrough_bench] getsv -F {tag}: {json.dumps(out[f'getsv_F_{tag}'])}", file=sys.stderr, flush=True)
        out[f"getsv_F_{tag}"]["sv_lines"] = open(args[3]).read().count("\n")
        ph = out[f"getsv_F_{tag}"]["phases_s"].get("readthrough (-F)")
        if ph:
            out[f"getsv_F_{tag}"]["f_records_per_s"] = round(a.records / ph)
    if not a.no_ref and os.path.exists(REF):
        print("[readthrough_bench] the reference binary (one thread: minutes at this size)", file=sys.stderr, flush=True)
        out["cpu_reference_getsv_F"], _ = timed([REF, "getsv", "-F", fbam] + args[:3] + [os.path.join(d, "ref.sv"), os.path.join(d, "ref.fq")])
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
