#!/usr/bin/env python3
"""What `seeksv run -P` costs, and what the same reads cost on the way it replaces.  The sample is bench.py's config-5 shape (human + HBV
tumor at 60x, 2 % of the records in pairs with one unmapped end) at --frac of the genome, written here with bench.py's own writer.  Alternating, --reps times:
  run        SSV_TIMING=1 seeksv run     tumor.bam ref.fa A        wall clock exec to exit
  run -P     SSV_TIMING=1 seeksv run -P  tumor.bam ref.fa B        the difference is the leg; its own lap and detail line are reported beside it
  chain      cat A.unmapped_[12].fq.gz | seeksv realign -P ref.fa - F.bam   (wall clock and phases), then seeksv getsv -F F.bam ... : the `readthrough (-F)` lap
             --chain-exe: another build's binary for these two commands (the parent commit's)
and whether B.sv.txt and the stdout of `run -P` equal the chain's.  One JSON line.
usage: python tools/run_split_bench.py [--frac F] [--reps R] [--chain-exe PATH] [--aln "-c 500"]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from seeksv_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=1 / 64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--chain-exe", default=None)
    ap.add_argument("--aln", default="")
    args = ap.parse_args()
    exe = os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
    chain_exe = args.chain_exe or exe
    tumor = synth.Workload(depth=60.0, n_integrations=50, genome_frac=args.frac, n_sv=max(8, round(10000 * args.frac)), hbv=True, unmap_permille=20)
    where = bench.room_for(int(tumor.n_total * 400 + tumor.genome_len * 1.1))
    d = tempfile.mkdtemp(prefix="ssv_runP_", dir=where)
    env = dict(os.environ, SSV_TIMING="1")
    aln = args.aln.split()
    out = dict(records=tumor.n_total, genome_frac=args.frac, aln=args.aln, chain_exe=os.path.relpath(chain_exe, ROOT), reps=[])
    try:
        t0 = time.perf_counter()
        bam, fa = os.path.join(d, "tumor.bam"), os.path.join(d, "ref.fa")
        bench.write_workload_bam(tumor, bam, -2)
        tumor.write_fasta(fa, bench.effective_cpus())
        out["files_made_s"] = round(time.perf_counter() - t0, 1)
        env.pop("SSV_BGZF_LEVEL", None)

        def timed(cmd, **kw):
            t = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, env=env, **kw)
            s = time.perf_counter() - t
            if r.returncode != 0:
                raise RuntimeError(" ".join(cmd[:3]) + ": " + r.stderr[-400:])
            return r, round(s, 3)
        a_opts = ["-a", args.aln] if aln else []
        for rep in range(args.reps):
            A, B = os.path.join(d, "A"), os.path.join(d, "B")
            ra, sa = timed([exe, "run"] + a_opts + [bam, fa, A])
            rb, sb = timed([exe, "run", "-P"] + a_opts + [bam, fa, B])
            pb = bench.timing_phases(rb.stderr)
            leg = next((v for k, v in pb.items() if k.startswith("readthrough (run -P")), None)
            with open(os.path.join(d, "u12.fq.gz"), "wb") as f:
                for k in "12":
                    f.write(open(f"{A}.unmapped_{k}.fq.gz", "rb").read())
            rc, sc = timed([chain_exe, "realign", "-P"] + aln + [fa, os.path.join(d, "u12.fq.gz"), os.path.join(d, "F.bam")])
            rd, sd = timed([chain_exe, "getsv", "-Z", "-F", os.path.join(d, "F.bam"), A + ".clip.bam", bam, A + ".clip.gz", os.path.join(d, "C.sv.txt"), os.path.join(d, "C.u.fq")])
            pd = bench.timing_phases(rd.stderr)
            pc = bench.timing_phases(rc.stderr)
            out["reps"].append(dict(
                run_s=sa, run_P_s=sb, leg_by_difference_s=round(sb - sa, 3), leg_lap_s=leg,
                leg_detail=[l[9:] for l in rb.stderr.splitlines() if l.startswith("[timing] (run -P")],
                leg_closing_line=[l for l in rb.stderr.splitlines() if l.startswith("[seeksv realign]")][-1],
                chain_realign_P_s=sc, chain_realign_P_phases_s=pc, chain_realign_P_without_reference_and_index_s=round(sum(v for k, v in pc.items() if k in ("read fastq", "align", "write bam")), 3),
                chain_getsv_F_s=sd, chain_readthrough_lap_s=pd.get("readthrough (-F)"),
                chain_closing_line=[l for l in rc.stderr.splitlines() if l.startswith("[seeksv realign]")][-1],
                F_bam_bytes=os.path.getsize(os.path.join(d, "F.bam")),
                table_equals_chain=open(B + ".sv.txt", "rb").read() == open(os.path.join(d, "C.sv.txt"), "rb").read(), stdout_equals_chain=rb.stdout == rd.stdout,
                table_rows=sum(1 for l in open(B + ".sv.txt") if not l.startswith("@")),
                table_rows_without_P=sum(1 for l in open(A + ".sv.txt") if not l.startswith("@"))))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
