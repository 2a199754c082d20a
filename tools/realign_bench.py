#!/usr/bin/env python3
"""The GPU re-aligner (ssv_realign_*) at the size of the bench workload: index of the whole synthetic genome (generated in
HBM), then queries cut from it - half of them real placements (both strands, 0.5 % substitutions), half random sequence like the bulk of
a sample's soft clips.  usage: python tools/realign_bench.py [--index hash|sorted|both] [--max-occ N] [--rounds R] [--gapped] [--alts K [--family N]] [--split SHARE [--rows]] [genome_frac] [n_queries] [query_len]
--gapped: half of the random queries give way to a third class, real placements that carry one insertion or deletion of 1-3 bases at least 12 bases
from either end; every round then runs the set through ssv_realign_query and through ssv_realign_query_gapped (`seeksv realign -g`) and reports both.
--alts K: every round also runs the set through ssv_realign_query_alts with max_alt K (`seeksv realign -S K`) and reports the query kernel, the scan and
k_ra_alt_compact ("realign_alts"), the number of alternates, and whether the primaries are the plain call's.  --family N (with --alts) first plants N elements of
64 bases in 5 copies each into the reference (word-aligned 2-bit copies on the device, before any index is built) and gives N of the random queries' places to a
fourth class: 60 bases of such an element; reported: how many come back with all five copies (primary + 4 alternates).
--split SHARE: that share of the real placements become reads of two loci - their second half comes from another place of the reference, same substitutions,
either strand -, and every round also runs the set through ssv_realign_query_split (`seeksv realign -P`): reported are the split query kernel's time beside the
plain kernel's on the same set, how many planted splits come back at both planted places, and whether the primaries without a mate are the plain call's.
--rows (with --split): every round also runs the set through ssv_realign_split_batch (`seeksv run -P`: the records built on the device) with names and
qualities: reported are the `realign_rows` group (k_rr_sizes, three scans, k_rr_rows) beside `realign_query` of the same call, the batch's sizes, and whether hits
and mates are the split call's.
--index both builds and queries the two kinds of index in one process, alternating (hash, sorted, hash, sorted, ...), R times each: one JSON line
with a list of rounds per kind.  Index bytes are computed from the sizes the library allocates, not measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seeksv_amd import _abi, synth  # noqa: E402
from seeksv_amd.device import Context  # noqa: E402


def index_bytes(kind, samples):
    """(bytes the index keeps, bytes allocated while it is built) for ceil(n_bases / 4) sampled positions"""
    if kind == "hash":
        slots = 1024
        while slots < 2 * samples:
            slots <<= 1
        return 4 * slots, 4 * slots
    bits = min(30, max(0, int(samples).bit_length() - 1))
    kept = 12 * samples + 4 * ((1 << bits) + 1)
    tiles = (samples + 2047) // 2048
    return kept, kept + 12 * samples + 4 * 256 * tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", choices=["hash", "sorted", "both"], default="hash")
    ap.add_argument("--max-occ", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--gapped", action="store_true")
    ap.add_argument("--alts", type=int, default=0)
    ap.add_argument("--family", type=int, default=0)
    ap.add_argument("--split", type=float, default=0.0)
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("genome_frac", nargs="?", type=float, default=1.0)
    ap.add_argument("n_queries", nargs="?", type=int, default=2_000_000)
    ap.add_argument("query_len", nargs="?", type=int, default=60)
    args = ap.parse_args()
    frac, nq, qlen = args.genome_frac, args.n_queries, args.query_len
    if args.family and (not args.alts or qlen > 60):
        ap.error("--family needs --alts and queries of at most 60 bases")
    if args.split and (not 0 < args.split <= 1 or qlen < 60):
        ap.error("--split needs a share in (0, 1] and queries of at least 60 bases (two pieces of 30)")
    if args.rows and not args.split:
        ap.error("--rows needs --split")
    import torch
    w = synth.Workload(genome_frac=frac, depth=1, n_sv=0)
    t = time.perf_counter()
    words, off = w.reference_2bit(0)
    torch.cuda.synchronize()
    t_ref = time.perf_counter() - t
    fam_words = None
    if args.family:   # N x 5 distinct two-word places inside one contig each; place 0 of a family is copied over the other four
        f = np.random.RandomState(13)
        cand = np.unique(f.randint(0, (int(off[-1]) >> 5) // 4 - 1, 8 * args.family * 5)) * 4
        inside = np.searchsorted(off, cand * 32, side="right") == np.searchsorted(off, cand * 32 + 63, side="right")
        cand = f.permutation(cand[inside])[:args.family * 5]
        assert len(cand) == args.family * 5, "too few places for the families"
        fam_words = cand.reshape(args.family, 5)
        src = torch.as_tensor(fam_words[:, 0], device=words.device)
        for k in range(1, 5):
            dst = torch.as_tensor(fam_words[:, k], device=words.device)
            words[dst] = words[src]
            words[dst + 1] = words[src + 1]
        torch.cuda.synchronize()
    ctx = Context(0)
    ctx.prof_enable(1)
    # queries
    rng = np.random.RandomState(11)
    G = int(off[-1])
    n_real = nq // 2
    tid = rng.randint(0, len(off) - 1, n_real)
    start = (off[tid] + (rng.random_sample(n_real) * (np.diff(off)[tid] - qlen)).astype(np.int64)).astype(np.int64)
    wh = words.cpu().numpy().view(np.uint64)
    idx = start[:, None] + np.arange(qlen)[None, :]
    codes = ((wh[idx >> 5] >> ((idx & 31) * 2).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
    sub = rng.random_sample(codes.shape) < 0.005
    codes = np.where(sub, (codes + 1 + rng.randint(0, 3, codes.shape)) & 3, codes).astype(np.uint8)
    n_split = int(n_real * args.split)
    if n_split:   # the first n_split real placements: bases [qlen / 2, qlen) from another place (a generator of its own: the other classes stay what they are without --split)
        sp = np.random.RandomState(15)
        tid2 = sp.randint(0, len(off) - 1, n_split)
        start2 = (off[tid2] + (sp.random_sample(n_split) * (np.diff(off)[tid2] - qlen)).astype(np.int64)).astype(np.int64)
        idx2 = start2[:, None] + np.arange(qlen // 2, qlen)[None, :]
        codes2 = ((wh[idx2 >> 5] >> ((idx2 & 31) * 2).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
        codes[:n_split, qlen // 2:] = np.where(sub[:n_split, qlen // 2:], codes[:n_split, qlen // 2:], codes2)
    rev = rng.random_sample(n_real) < 0.5
    codes[rev] = (3 - codes[rev])[:, ::-1]
    junk = rng.randint(0, 4, (nq - n_real, qlen)).astype(np.uint8)
    n_gap = (nq - n_real) // 2 if args.gapped else 0
    if n_gap:   # the third class takes the place of the first n_gap random queries (a generator of its own: the other two classes stay what they are without --gapped)
        g = np.random.RandomState(12)
        gtid = g.randint(0, len(off) - 1, n_gap)
        gstart = (off[gtid] + (g.random_sample(n_gap) * (np.diff(off)[gtid] - qlen - 3)).astype(np.int64)).astype(np.int64)
        glen = g.randint(1, 4, n_gap)
        gins = g.random_sample(n_gap) < 0.5
        gat = 12 + (g.random_sample(n_gap) * (qlen - 24 - glen + 1)).astype(np.int64)   # the gap (and an insertion's bases) lie in [12, qlen - 12)
        col = np.arange(qlen)[None, :]
        behind = col >= (gat + np.where(gins, glen, 0))[:, None]
        gidx = gstart[:, None] + col + np.where(behind, np.where(gins, -glen, glen)[:, None], 0)
        gcodes = ((wh[gidx >> 5] >> ((gidx & 31) * 2).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
        inserted = gins[:, None] & (col >= gat[:, None]) & ~behind
        gcodes = np.where(inserted, g.randint(0, 4, gcodes.shape), gcodes).astype(np.uint8)
        gsub = g.random_sample(gcodes.shape) < 0.005
        gcodes = np.where(gsub, (gcodes + 1 + g.randint(0, 3, gcodes.shape)) & 3, gcodes).astype(np.uint8)
        grev = g.random_sample(n_gap) < 0.5
        gcodes[grev] = (3 - gcodes[grev])[:, ::-1]
        junk[:n_gap] = gcodes
    n_fam = args.family
    if n_fam:   # the fourth class, behind the third: bases 2..2 + qlen of a family's element, either strand
        f = np.random.RandomState(14)
        fidx = (fam_words[:, 0] * 32 + 2)[:, None] + np.arange(qlen)[None, :]
        fcodes = ((wh[fidx >> 5] >> ((fidx & 31) * 2).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
        frev = f.random_sample(n_fam) < 0.5
        fcodes[frev] = (3 - fcodes[frev])[:, ::-1]
        assert n_gap + n_fam <= len(junk)
        junk[n_gap:n_gap + n_fam] = fcodes
    allc = np.concatenate([codes, junk])
    order = rng.permutation(nq)
    allc = allc[order]
    lut = np.frombuffer(b"ACGT", np.uint8)
    text = lut[allc].tobytes().decode()
    seqs = [text[i * qlen:(i + 1) * qlen] for i in range(nq)]
    if args.rows:   # names like getclip's, qualities of forty values
        r = np.random.RandomState(16)
        qtext = (33 + r.randint(2, 42, nq * qlen)).astype(np.uint8).tobytes().decode()
        quals = [qtext[i * qlen:(i + 1) * qlen] for i in range(nq)]
        names = [f"read{i}/{1 + (i & 1)}" for i in range(nq)]
    is_split = order < n_split
    is_real = (order < n_real) & ~is_split
    exp_tid = np.full(nq, -1)
    exp_tid[is_real] = tid[order[is_real]]
    exp_pos = np.full(nq, -1, np.int64)
    exp_pos[is_real] = (start - off[tid])[order[is_real]]
    exp_tid[is_split], exp_pos[is_split] = tid[order[is_split]], (start - off[tid])[order[is_split]]   # the first half's place; the second half's:
    exp_tid2, exp_pos2 = np.full(nq, -1), np.full(nq, -1, np.int64)
    if n_split:
        exp_tid2[is_split], exp_pos2[is_split] = tid2[order[is_split]], (start2 - off[tid2])[order[is_split]]
    is_gap = (order >= n_real) & (order < n_real + n_gap)
    exp_len = np.zeros(nq, np.int64)
    if n_gap:
        exp_tid[is_gap] = gtid[order[is_gap] - n_real]
        exp_pos[is_gap] = (gstart - off[gtid])[order[is_gap] - n_real]
        exp_len[is_gap] = np.where(gins, -glen, glen)[order[is_gap] - n_real]
    is_fam = (order >= n_real + n_gap) & (order < n_real + n_gap + n_fam)
    fam_of = order[is_fam] - n_real - n_gap
    is_junk = ~is_real & ~is_split & ~is_gap & ~is_fam
    samples = (G + 3) // 4

    def one(kind):
        ctx.prof_reset()
        t = time.perf_counter()
        if kind == "hash":
            built = {"index_dropped": ctx.realign_index(words.data_ptr(), off, _abi.MEM_DEVICE)}
        else:
            built = {"index_stats": ctx.realign_index_sorted(words.data_ptr(), off, args.max_occ, _abi.MEM_DEVICE), "max_occ": args.max_occ}
        t_index = time.perf_counter() - t
        t = time.perf_counter()
        hits = ctx.realign(seqs)
        t_query = time.perf_counter() - t
        prof = ctx.prof_all()
        ok_real = int(((hits["tid"] == exp_tid) & (hits["pos"] - hits["q_beg"] == exp_pos) & (hits["mapq"] > 0))[is_real].sum())
        kept, peak = index_bytes(kind, samples)
        flags = hits["pad"][:, 0]
        out = dict(built, index_wall_s=round(t_index, 3), index_kernel_ms=round(prof["realign_index"]["total_ms"], 2),
                   index_positions_per_s=round(samples / (prof["realign_index"]["total_ms"] * 1e-3)), index_GB=round(kept / 1e9, 2), index_build_GB=round(peak / 1e9, 2),
                   query_wall_s=round(t_query, 3), query_kernel_ms=round(prof["realign_query"]["total_ms"], 2),
                   queries_per_s_kernel=round(nq / (prof["realign_query"]["total_ms"] * 1e-3)), real_placed_correctly=ok_real,
                   junk_unaligned=int((hits["tid"][is_junk] == -1).sum()), masked=int((flags & 1).astype(bool).sum()), over_limit=int((flags & 2).astype(bool).sum()))
        plain = hits
        if args.alts:   # the same queries once more, with their other loci
            ctx.prof_reset()
            t = time.perf_counter()
            h2, _, aoff, alts = ctx.realign_alts(seqs, args.alts)
            t_query = time.perf_counter() - t
            prof = ctx.prof_all()
            q_ms, a_ms = prof["realign_query"]["total_ms"], prof["realign_alts"]["total_ms"]
            cut = (h2["pad"][:, 0] & _abi.RA_F_ALT_CUT) != 0
            h2["pad"][:, 0] &= ~np.uint8(_abi.RA_F_ALT_CUT)
            n_alt = np.diff(aoff)
            out["alts"] = dict(max_alt=args.alts, query_wall_s=round(t_query, 3), query_kernel_ms=round(q_ms, 2), scan_compact_kernel_ms=round(a_ms, 3),
                               scan_compact_launches=int(prof["realign_alts"]["launches"]),
                               queries_per_s_kernels=round(nq / ((q_ms + a_ms) * 1e-3)), alternates=int(aoff[-1]), queries_with_alternates=int((n_alt > 0).sum()),
                               cut=int(cut.sum()), primaries_equal_plain=bool(h2.tobytes() == plain.tobytes()),
                               real_with_alternates=int((n_alt > 0)[is_real].sum()), junk_with_alternates=int((n_alt > 0)[is_junk].sum()))
            if n_fam:   # primary + 4 alternates = the five planted places (the diagonal of a 60-base query is its copy's base 2 on either strand)
                want = np.sort(fam_words[fam_of] * 32 + 2, axis=1)
                qi = np.flatnonzero(is_fam)
                full = n_alt[qi] == 4
                got = np.full((len(qi), 5), -1, np.int64)
                got[:, 0] = off[np.maximum(h2["tid"][qi], 0)] + h2["pos"][qi] - h2["q_beg"][qi]
                for k in range(4):
                    a = alts[np.where(full, aoff[qi] + k, 0)] if len(alts) else None
                    if a is not None:
                        got[:, 1 + k] = np.where(full, off[np.maximum(a["tid"], 0)] + a["pos"] - a["q_beg"], -1)
                out["alts"].update(family_queries=int(len(qi)), family_with_four_alternates=int(full.sum()),
                                   family_all_five_copies_back=int((np.sort(got, axis=1) == want).all(axis=1).sum()),
                                   family_primary_mapq0=int((h2["mapq"][qi] == 0).sum()))
        if n_split:   # the same queries once more, with their second pieces
            ctx.prof_reset()
            t = time.perf_counter()
            h3, mates = ctx.realign_split(seqs)
            t_query = time.perf_counter() - t
            q_ms = ctx.prof_all()["realign_query"]["total_ms"]
            has = mates["tid"] >= 0

            def at(h, etid, epos):
                return (h["tid"] == etid) & (h["pos"] - h["q_beg"] == epos)
            both = has & ((at(h3, exp_tid, exp_pos) & at(mates, exp_tid2, exp_pos2)) | (at(h3, exp_tid2, exp_pos2) & at(mates, exp_tid, exp_pos)))
            out["split"] = dict(split_reads=int(is_split.sum()), query_wall_s=round(t_query, 3), query_kernel_ms=round(q_ms, 2), plain_query_kernel_ms=out["query_kernel_ms"],
                                queries_per_s_kernel=round(nq / (q_ms * 1e-3)), mates=int(has.sum()), split_reads_with_mate=int(has[is_split].sum()),
                                planted_splits_back_at_both_places=int(both[is_split].sum()), both_pieces_mapq_above_0=int((both & (h3["mapq"] > 0) & (mates["mapq"] > 0))[is_split].sum()),
                                plain_call_split_reads_mapq0=int((plain["mapq"] == 0)[is_split & (plain["tid"] >= 0)].sum()),
                                real_with_mate=int(has[is_real].sum()), junk_with_mate=int(has[is_junk].sum()),
                                primaries_without_mate_equal_plain=bool(h3[~has].tobytes() == plain[~has].tobytes()))
        if args.rows:   # ... and once more with their records built on the device
            ctx.prof_reset()
            t = time.perf_counter()
            h4, m4, b, _ = ctx.realign_split_batch(seqs, names, quals)
            t_query = time.perf_counter() - t
            prof = ctx.prof_all()
            r_ms = prof["realign_rows"]["total_ms"]
            n_rec, n_ops, sq = int(b.n), int(b.n_cigar_total), int(b.seqqual_bytes)
            written = n_rec * (64 + 4 + 4 + 2 + 1 + 2 + 1 + 1 + 4 + 4 + 4 + 4 + 4 + 8 + 4 + 8) + n_ops * 4 + sq   # line, columns, name offset; operations; bases + qualities
            out["rows"] = dict(call_wall_s=round(t_query, 3), query_kernel_ms=round(prof["realign_query"]["total_ms"], 2), rows_kernels_ms=round(r_ms, 3),
                               rows_launch_groups=int(prof["realign_rows"]["launches"]), records=n_rec, cigar_operations=n_ops, seqqual_bytes=sq,
                               bytes_written=written, bytes_read=2 * nq * qlen + 64 * nq, GB_per_s=round((written + 2 * nq * qlen + 64 * nq) / (r_ms * 1e-3) / 1e9, 1),
                               reads_per_s_rows_kernels=round(nq / (r_ms * 1e-3)), hits_and_mates_equal_split_call=bool(h4.tobytes() == h3.tobytes() and m4.tobytes() == mates.tobytes()))
        if args.gapped:   # the same queries once more, with gaps
            at_locus = (hits["tid"] == exp_tid) & (hits["mapq"] > 0)
            out["ungapped_gap_class_at_its_contig"] = int(at_locus[is_gap].sum())
            ctx.prof_reset()
            t = time.perf_counter()
            hits, gaps = ctx.realign(seqs, gapped=True)
            t_query = time.perf_counter() - t
            prof = ctx.prof_all()
            q_ms, g_ms = prof["realign_query"]["total_ms"], prof["realign_gap"]["total_ms"]
            placed = (hits["tid"] == exp_tid) & (hits["pos"] - hits["q_beg"] == exp_pos) & (hits["mapq"] > 0)
            out["gapped"] = dict(query_wall_s=round(t_query, 3), query_kernel_ms=round(q_ms, 2), gap_kernel_ms=round(g_ms, 2), queries_per_s_kernels=round(nq / ((q_ms + g_ms) * 1e-3)),
                                 real_placed_correctly=int((placed & (gaps["len"] == 0))[is_real].sum()), real_with_a_gap=int((gaps["len"] != 0)[is_real].sum()),
                                 junk_unaligned=int((hits["tid"][is_junk] == -1).sum()),
                                 planted_gap_found=int((placed & (gaps["len"] == exp_len))[is_gap].sum()), gap_class_with_another_gap=int(((gaps["len"] != 0) & ~(placed & (gaps["len"] == exp_len)))[is_gap].sum()),
                                 gap_class_without_gap=int((gaps["len"] == 0)[is_gap].sum()))
        return out

    kinds = ["hash", "sorted"] if args.index == "both" else [args.index]
    out = {"genome_bases": G, "sampled_positions": samples, "reference_2bit_s": round(t_ref, 3), "queries": nq, "query_len": qlen, "real": int(is_real.sum()), "junk": int(is_junk.sum()), "with_planted_gap": int(is_gap.sum()), "from_a_planted_family": int(is_fam.sum()), "split_in_two_loci": int(is_split.sum()),
           "rounds": {k: [] for k in kinds}}
    for _ in range(args.rounds):
        for k in kinds:
            out["rounds"][k].append(one(k))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
