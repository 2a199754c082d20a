"""The read cap of libbam 0.1.16's pileup (bam_plp_push / bam_plp_next) as a plain per-read model: no ring, no batches, one heap of the
ends of the reads the pileup still holds.  Written from the library's rule, not from oracle/seeksv_oracle.c or the kernels: the tests hold
both against it (and all of them against what the real reference wrote, tests/golden/pileup_cap/reference.json).

records: dicts with tid, pos (0-based), flag, mapq and cigar (text), in file order."""
import heapq

import numpy as np

import bamio

MAXCNT = 8000                          # bam_plp_t.maxcnt; two nodes of the pool are always allocated besides the live reads
MASK = 4 | 256 | 512 | 1024            # BAM_DEF_MASK; read_bam turns MAPQ < -q into UNMAP


def passes(r, min_mapq):
    return r["tid"] >= 0 and r["mapq"] >= min_mapq and not (r["flag"] & MASK)


def ref_span(cigar):
    """bam_calend: M, D, N advance the reference ('=' and 'X' do not in this version)"""
    return sum(l for l, op in bamio.parse_cigar(cigar) if op in (0, 2, 3))


def dropped_reads(records, min_mapq=20, parent_rule=False, trace=None):
    """-> indices of the reads that bam_plp_push drops.  parent_rule: a read without any M/D/N operation is never live (what this project
    computed before the reference pinned the rule).  trace: a list that receives (index, live reads before the read) per passing read."""
    dropped, ends = [], []
    tid, pos = 0, 0                    # where libbam's iterator stands: the start of the read pushed last ((0, 0) before the first one)
    for i, r in enumerate(records):
        if not passes(r, min_mapq):
            continue
        if r["tid"] != tid:
            ends = []                  # the other contig's reads are freed on the way
        elif r["pos"] != pos:
            while ends and ends[0] <= r["pos"] - 1:
                heapq.heappop(ends)    # the columns before this start have been emitted: nodes with end <= column are freed
        if trace is not None:
            trace.append((i, len(ends)))
        if r["tid"] == tid and r["pos"] == pos and 2 + len(ends) > MAXCNT:
            dropped.append(i)
            continue
        end = r["pos"] + ref_span(r["cigar"])
        keep = end > pos or r["tid"] > tid          # iter->pos, iter->tid: still the read before
        if parent_rule:
            keep = end > r["pos"]
        if keep:
            heapq.heappush(ends, end)
        tid, pos = r["tid"], r["pos"]
    return dropped


def depth(records, dropped, min_mapq, tid, lo, hi):
    """per-column depth of columns lo..hi (1-based, inclusive) of one contig: every M base of a read that passes and is not dropped"""
    diff = np.zeros(hi - lo + 2, np.int64)
    gone = set(dropped)
    for i, r in enumerate(records):
        if r["tid"] != tid or i in gone or not passes(r, min_mapq):
            continue
        col = r["pos"] + 1
        for l, op in bamio.parse_cigar(r["cigar"]):
            if op == 0:
                a, b = max(col, lo), min(col + l - 1, hi)
                if a <= b:
                    diff[a - lo] += 1
                    diff[b - lo + 1] -= 1
            if op in (0, 2, 3):
                col += l
    return np.cumsum(diff)[:-1]
