"""CPU: the hand-made geometry of tests/getsv_window_inputs.py.  (a) Every family really reaches the edge it is for - an input that stopped reaching it
would leave tests/test_getsv_windows_gpu.py green and empty; the module's constants are the headers'.  (b) The oracle's answer for it is not a
table of zeros.  (c) The oracle is held against a SECOND plain implementation: depth as a numpy difference array per contig (only M covers; M, D, N
advance; the MAPQ and flag filter of orc_depth), and the discordant tally with the candidate rule of the index query brute force over every record
(calend > beg && pos < end, no sorted shortcut).  No golden of the real reference can exist for these inputs - its planner makes the windows - so two
independent plain implementations that agree are what pins the reference here; the discordant geometry itself is pinned by tests/golden."""
import os
import re

import numpy as np
import pytest

import getsv_window_inputs as W
import oracle_lib as O

QS = (20, 0)
CSRC = os.path.join(O.ROOT, "seeksv_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------------
# the constants
# ---------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_headers():
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("getsv_kernels.h", "clip_kernels.h", "common.h")}

    def const(f, name):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", text[f])
        assert m, (f, name)
        return int(m.group(1))

    assert 1 << const("getsv_kernels.h", "TILE_SHIFT") == W.TILE
    assert const("common.h", "WAVE") == W.WAVE
    assert const("getsv_kernels.h", "GC_COLS") == W.GC_COLS
    assert const("getsv_kernels.h", "GC_DENSE_MIN") == W.GC_DENSE_MIN
    m = re.search(r"constexpr\s+int\s+GC_JC\s*=\s*(\d+)\s*,\s*GC_WC\s*=\s*(\d+)\s*;", text["getsv_kernels.h"])
    assert m and (int(m.group(1)), int(m.group(2))) == (W.GC_JC, W.GC_WC)
    assert re.search(r"constexpr\s+int\s+CS_TILE\s*=\s*BLOCK\s*\*\s*CS_ITEMS\s*\*\s*CS_SUB\s*;", text["clip_kernels.h"])
    assert const("common.h", "BLOCK") * const("clip_kernels.h", "CS_ITEMS") * const("clip_kernels.h", "CS_SUB") == W.CS_TILE
    # k_depth_prefix: four scans of a wavefront per round; window_at_or_before: a probe per lane
    body = text["getsv_kernels.h"].split("void k_depth_prefix", 1)[1].split("\n}\n", 1)[0]
    m = re.search(r"base\s*\+=\s*WAVE\s*\*\s*(\d+)", body)
    assert m and int(m.group(1)) * W.WAVE == W.PREFIX_ROUND
    body = text["getsv_kernels.h"].split("window_at_or_before(", 1)[1].split("\n}\n", 1)[0]
    assert re.search(r"step\s*=\s*\(hi - lo \+ WAVE - 1\)\s*/\s*WAVE", body)
    assert W.WINDOW_COUNTS == (1, 63, 64, 65, 4095, 4096, 4097, 4160, 4161)


# ---------------------------------------------------------------------------------------------------------------------
# every family reaches its edge
# ---------------------------------------------------------------------------------------------------------------------
def tile_of_column(c):
    return (c - 1) >> 9      # the column of a record's base at 0-based pos c - 1


def scan_tile_counts(flags, at=0):
    return np.add.reduceat(flags[at:].astype(np.int64), np.arange(0, len(flags) - at, W.CS_TILE))


def most_in_any_scan_tile(flags):
    """the most candidates any CS_TILE records in a row hold: wherever the stream is cut into batches"""
    c = np.concatenate(([0], np.cumsum(flags.astype(np.int64))))
    k = min(W.CS_TILE, len(flags))
    return int((c[k:] - c[:-k]).max())


@pytest.mark.parametrize("name", W.CASES)
def test_case_is_well_formed(name):
    """what the ABI asks of every input - windows sorted, disjoint, non-empty - and what these inputs promise: their sizes, reads that end on their contig"""
    names, lens, b, j, w, r, p, mean, sd = W.case(name)
    n = len(b["tid"])
    assert 0 < n <= 40000 and len(names) == len(lens)
    assert w.dtype == r.dtype == p.dtype == W._abi.INTERVAL_DTYPE and j.dtype == W._abi.JUNCTION_DTYPE
    assert np.all(w["beg"] <= w["end"])
    same = w["tid"][1:] == w["tid"][:-1]
    assert np.all((w["tid"][1:] > w["tid"][:-1]) | (same & (w["end"][:-1] < w["beg"][1:])))
    cols = int((w["end"].astype(np.int64) - w["beg"] + 1).sum())
    assert cols <= (21000 if name.startswith("long_window") else 12500)
    assert np.all(b["pos"] >= 0) and np.all((b["tid"] >= 0) & (b["tid"] < len(lens)))
    assert np.all(W.calends(b) <= np.array(lens)[b["tid"]])                       # every read's last column <= its contig's length
    assert np.all(W.ref_spans(b) <= b["max_ref_span"]) and b["max_ref_span"] == W.ref_spans(b).max()
    assert np.all(p["beg"] == p["end"]) and np.all(r["beg"] <= r["end"])
    assert len(W._abi.runs_of_tid(b["tid"])) <= 48                                # the batch goes to k_getsv_scan_runs with its runs
    # no range reaches into a second window (the ABI excludes it)
    for t, beg, end in r.tolist():
        assert int(((w["tid"] == t) & (w["beg"] <= end) & (w["end"] >= beg)).sum()) <= 1
    # every kind of CIGAR the passes tell apart
    ops = set((b["cigar"] & 15).tolist())
    assert {0, 1, 2, 3, 4, 5, 7} <= ops and b["n_cigar"].max() > 5


def search_rounds(n, k):
    """window_at_or_before replayed: n windows of which the first k are <= the key -> rounds of WAVE probes until the answer k - 1 is known"""
    lo, hi, rounds = 0, n, 0
    while hi - lo > 0:
        rounds += 1
        step = (hi - lo + W.WAVE - 1) // W.WAVE
        le = sum(1 for lane in range(W.WAVE) if lo + lane * step < min(hi, k))      # probes lo, lo + step, ...: a prefix of the lanes is <= the key
        if le == 0:
            hi = lo
            break
        last_le = lo + (le - 1) * step
        lo, hi = last_le + 1, min(last_le + step, hi)
    assert lo - 1 == k - 1
    return rounds


@pytest.mark.parametrize("n_win", W.WINDOW_COUNTS)
def test_window_counts(n_win):
    names, lens, b, j, w, r, p, mean, sd = W.case(f"window_counts_{n_win}")
    assert len(w) == n_win and len(lens) == 1 and len(b["tid"]) >= W.CS_TILE
    # every window is asked for (a range each): the deepest search over them takes 1 round up to WAVE windows, 2 up to WAVE * (WAVE + 1), then 3
    rounds = max(search_rounds(n_win, k) for k in range(1, n_win + 1))
    assert rounds == (1 if n_win <= W.WAVE else (2 if n_win <= W.SEARCH_TWO_ROUNDS else 3))
    length = w["end"] - w["beg"] + 1
    assert length.min() >= 1 and length.max() <= 3 and (n_win < 63 or set(length.tolist()) == {1, 2, 3})
    gap = w["beg"][1:] - w["end"][:-1] - 1
    assert n_win < 63 or set(gap.tolist()) == {0, 1}                              # [x, x], [x + 1, ...]: end < next.beg is all the ABI asks
    assert np.array_equal(r, w) and len(p) == int((length == 1).sum() + 2 * (length > 1).sum())
    if n_win >= 4095:   # hundreds of windows in one genome tile, and far more than GC_WC in a dense workgroup's columns
        assert np.bincount(tile_of_column(w["beg"])).max() > 150
        assert most_in_any_scan_tile(W.candidate_flags(lens, b, w, j)) >= W.GC_DENSE_MIN


def test_window_lengths():
    names, lens, b, j, w, r, p, mean, sd = W.case("window_lengths")
    W_, R_ = W.WAVE, W.PREFIX_ROUND
    assert set(W.WINDOW_LENGTHS) == {1, 2, W_ - 1, W_, W_ + 1, R_ - 1, R_, R_ + 1, 2 * R_ - 1, 2 * R_, 2 * R_ + 1, 4 * R_ + 1}
    length = (w["end"] - w["beg"] + 1).tolist()
    assert sorted(length) == sorted(2 * list(W.WINDOW_LENGTHS))
    for l in W.WINDOW_LENGTHS:
        a, s = [k for k in range(len(w)) if length[k] == l]
        assert (w["beg"][a] - 1) % W.TILE == 0                                    # from a genome tile's first column on
        if l == 1: assert w["beg"][s] % W.TILE == 0                               # a tile's last column
        else: assert tile_of_column(w["beg"][s]) < tile_of_column(w["end"][s]) and (w["beg"][s] - 1) % W.TILE != 0
        for q in ((0, w["beg"][a], w["beg"][a]), (0, w["end"][a], w["end"][a]), (0, w["beg"][a], w["end"][a]), (0, w["beg"][s], w["end"][s])):
            assert q in r.tolist()
    assert max(tile_of_column(w["end"]) - tile_of_column(w["beg"])) >= 2          # a window of three genome tiles


@pytest.mark.parametrize("variant", ("dense", "seam", "sparse", "one_long"))
def test_long_window(variant):
    names, lens, b, j, w, r, p, mean, sd = W.case(f"long_window_{variant}")
    assert len(w) == 1 and w[0].tolist() == (0, 1, lens[0]) and lens[0] == W.LONG_LEN > 4 * W.GC_COLS
    flags = W.candidate_flags(lens, b, w, j)
    on = b["tid"] == 0
    assert np.array_equal(flags, on)                                              # the window marks its whole contig, and nothing else is marked
    if variant == "sparse":
        assert most_in_any_scan_tile(flags) < W.GC_DENSE_MIN                      # no scan tile is dense, wherever the stream is cut
        depth = W._per_record(b, "M")[on].sum() / W.LONG_LEN                      # "about 5-fold"
        assert 3 < depth < 8
    else:
        counts = scan_tile_counts(flags)
        assert counts.min() >= W.GC_DENSE_MIN and len(counts) >= (5 if variant == "seam" else 9)                 # every scan tile is k_getsv_cand_dense's
        fold = W._per_record(b, "M").sum() / W.LONG_LEN
        reach = b["pos"][W.CS_TILE - 1::W.CS_TILE].astype(np.int64) - b["pos"][:-W.CS_TILE + 1:W.CS_TILE]   # from a scan tile's first start to its last
        if variant == "seam":   # reads on the last columns of every workgroup's range, and across its end
            assert 70 < fold < 110 and reach.min() > W.GC_COLS - 100 and np.median(reach) > W.GC_COLS
        else:                   # several hundred-fold with D and N counted; a workgroup's reads end half way through its range
            assert fold > 150 and reach.max() < W.GC_COLS * 3 // 4
        # a dense workgroup's columns begin at its first record: all but the first and last lie strictly inside the window
        c0 = b["pos"][::W.CS_TILE].astype(np.int64) + 1
        inside = (c0 > w["beg"][0]) & (c0 + W.GC_COLS - 1 < w["end"][0])
        assert inside.sum() >= (3 if variant == "seam" else 5) and inside[1:-3].all()
    starts = set(r["beg"].tolist()) | set(r["end"].tolist())
    for k in range(1, W.LONG_LEN // W.GC_COLS + 1):
        assert {k * W.GC_COLS, k * W.GC_COLS + 1, k * W.GC_COLS + 2} <= starts     # offsets 4095, 0, 1 (mod 4096) from column 1
    spans = W.ref_spans(b)
    if variant == "one_long":
        i = int(np.argmax(spans))
        assert spans[i] > 9000 and np.sort(spans)[-2] <= 450 and len(spans) // 2 < i < len(spans) - W.CS_TILE
    else:
        assert (spans > W.GC_COLS).sum() > (50 if variant == "dense" else 0)                                      # reads that leave a workgroup's columns (the per-read way)


def test_contig_edges():
    names, lens, b, j, w, r, p, mean, sd = W.case("contig_edges")
    n_t, span = len(lens), b["max_ref_span"]
    wl = w.tolist()
    assert any(beg == 1 and span > beg for t, beg, end in wl)                                           # beg - span < 0
    assert any(t < n_t and end == lens[t] for t, beg, end in wl)                                        # ends on the contig's last column
    assert any(t < n_t and end == lens[t] + 1000 and tile_of_column(end) >= (lens[t] >> 9) + 1 for t, beg, end in wl)   # t1 >= ntile
    assert lens[1] == 0 and {0, 2} <= set(b["tid"].tolist()) and 1 not in set(b["tid"].tolist())
    assert lens[2] % W.TILE == 0 and lens[3] % W.TILE == 1 and lens[2] > 0
    assert any(t >= n_t for t, beg, end in wl) and any(t >= n_t for t in p["tid"].tolist()) and any(t >= n_t for t in r["tid"].tolist())
    assert -1 in j["down_tid"].tolist() and any(t >= n_t for t in j["up_tid"].tolist())
    assert any(int(x["beg"]) - span < 0 for x in j) and any(int(x["end"]) > lens[int(x["up_tid"])] for x in j if x["up_tid"] < n_t)
    # reads whose last base is their contig's last, one of them alone in the contig's last genome tile; reads without a mate contig next to the junction without a down contig
    assert all(np.any((b["tid"] == t) & (W.calends(b) == lens[t])) for t in (0, 2, 3))
    assert np.any((b["tid"] == 3) & (b["pos"] >> 9 == lens[3] >> 9))
    k = int(np.flatnonzero(j["down_tid"] == -1)[0])
    near = (b["tid"] == j["up_tid"][k]) & (b["mtid"] == -1) & (W.calends(b) > j["beg"][k]) & (b["pos"] < j["end"][k])
    assert near.sum() >= 4 and O.discordant([b], j, mean, sd, 4, 0)[k] == 0
    assert len(b["tid"]) >= W.CS_TILE


@pytest.mark.parametrize("variant", ("dense", "spread", "sparse", "one_long"))
def test_mixed_junction_widths(variant):
    name = f"mixed_junction_widths_{variant}"
    names, lens, b, j, w, r, p, mean, sd = W.case(name)
    S = W.MIXED_STRETCH
    width = j["end"] - j["beg"]
    assert len(j) == 61 and width[0] == 100000 and j["beg"][0] < j["beg"][1:].min() and np.all(j["up_tid"] == 0)
    assert j["up_pos"][0] - j["beg"][0] > 20000 and S < j["up_pos"][0] < S + W.GC_COLS     # its pairs lie where a walk must start 21,000 bp back to meet it
    assert width[1:].min() >= 50 and width[1:].max() <= 700
    in_stretch = (j["beg"] >= S) & (j["end"] <= S + W.GC_COLS)
    assert in_stretch.sum() >= 40 > W.GC_JC
    under = (j["beg"][1:] > j["beg"][0]) & (j["end"][1:] < j["end"][0])
    assert under.sum() >= 50 and (j["beg"][1:] >= j["end"][0]).sum() >= 5 and ((j["beg"][1:] < j["end"][0]) & (j["end"][1:] > j["end"][0])).sum() >= 1
    nested = sum(1 for a in range(1, 61) for c in range(1, 61) if j["beg"][a] < j["beg"][c] and j["end"][c] < j["end"][a])
    assert nested >= 7
    combos = set(zip(j["up_strand"].tolist(), j["down_strand"].tolist()))
    assert combos == {(43, 43), (45, 43), (43, 45)} and W.DESIGNED[name] == list(range(61))
    one = w[w["beg"] == w["end"]]
    assert len(one) == 40 > W.GC_WC and len(set(tile_of_column(one["beg"]).tolist())) == 1          # 40 windows of one column in one genome tile
    flags = W.candidate_flags(lens, b, w, j)
    sorted_ = bool(np.all(np.diff(b["tid"]) >= 0))
    if variant == "sparse":
        assert not sorted_ and most_in_any_scan_tile(flags) < W.GC_DENSE_MIN
    else:
        assert sorted_ and scan_tile_counts(flags).min() >= W.GC_DENSE_MIN
    if variant == "spread":   # a dense workgroup whose records lie further apart than the GC_COLS / TILE + 1 genome tiles it keeps bits for
        assert (b["pos"][-1] >> 9) - (b["pos"][0] >> 9) > 100 and len(b["tid"]) < W.CS_TILE
    if variant in ("dense", "one_long"):
        assert int(((b["pos"] >= S - 1500) & (b["pos"] < S + W.GC_COLS + 1500)).sum()) > 30000
    spans = W.ref_spans(b)
    if variant == "one_long":
        i = int(np.argmax(spans))
        assert spans[i] > 9000 and np.sort(spans)[-2] <= 450 and len(spans) // 3 < i < len(spans) - W.CS_TILE


def test_outside_queries():
    names, lens, b, j, w, r, p, mean, sd = W.case("outside_queries")
    n_t = len(lens)
    wl, pl, rl = w.tolist(), [(t, c) for t, c, _ in p.tolist()], r.tolist()
    inside = lambda t, c: any(wt == t and beg <= c <= end for wt, beg, end in wl)
    t0, b0, e0 = wl[0]
    assert t0 == 0 and any(t == 0 and c < b0 for t, c in pl)                                           # before the first window of the first contig
    gaps = [(t, e + 1) for (t, _, e), (t2, b2, _) in zip(wl, wl[1:]) if t == t2 and b2 == e + 2]
    assert gaps and all(g in pl for g in gaps)                                                          # a gap of one column
    assert all((t, e + 1) in pl and (t, beg) in pl and (t, e) in pl for t, beg, e in wl)               # one column behind every window; both ends
    windowless = set(b["tid"].tolist()) - set(w["tid"].tolist())
    assert windowless and any(t in windowless for t, c in pl)                                           # records, but no window
    assert any(t >= n_t for t, c in pl)
    assert sum(1 for t, c in pl if not inside(t, c)) >= 9
    own = lambda t, beg: next((x for x in wl if x[0] == t and x[1] <= beg <= x[2]), None)
    assert all(own(t, beg) for t, beg, end in rl)                                                       # every range starts inside a window
    assert any(end == own(t, beg)[2] and beg > own(t, beg)[1] for t, beg, end in rl)                    # ends exactly on the last column
    assert any(beg == own(t, beg)[1] and end < own(t, beg)[2] for t, beg, end in rl)                    # starts exactly on the first
    assert any(beg == end for t, beg, end in rl)
    past = [(t, beg, end) for t, beg, end in rl if end > own(t, beg)[2]]
    assert len(past) >= 4 and any(end == own(t, beg)[2] + 1 for t, beg, end in past)                    # into a gap; one of them by a single column
    # the contig with the junctions has no depth window
    assert set(j["up_tid"].tolist()) == {1} and 1 not in w["tid"].tolist()


def test_genome_scale():
    names, lens, b, j, w, r, p, mean, sd = W.case("genome_scale")
    assert len(lens) == 3366 and lens[0] == 248956422 and lens[W.GENOME_BIG] == 2 ** 29 - 1 and sum(1 for l in lens if l == 0) > 20
    used = [0, W.GENOME_BIG, 3365]
    assert sorted(set(b["tid"].tolist())) == used == sorted(set(w["tid"].tolist())) == sorted(set(j["up_tid"].tolist()))
    assert sum((l >> 9) + 1 for l in lens) > 2 ** 21                                                    # genome tiles: the tile map's size
    for t in used:
        on = b["tid"] == t
        assert on.sum() > 4000 and b["pos"][on].min() >= lens[t] - 6000 and W.calends(b)[on].max() == lens[t]
        assert w["end"][w["tid"] == t].max() == lens[t] and w["beg"][w["tid"] == t].min() >= lens[t] - 6000
    assert all(x["up_tid"] != x["down_tid"] for x in j) and np.all(j["end"] <= np.array(lens)[j["up_tid"]])
    assert int(W.calends(b).max()) == 2 ** 29 - 1


@pytest.mark.parametrize("what", ("no_windows", "no_junctions", "neither"))
def test_nothing_to_do(what):
    names, lens, b, j, w, r, p, mean, sd = W.case(f"nothing_to_do_{what}")
    assert (len(w) == 0) == (what != "no_junctions") and (len(j) == 0) == (what != "no_windows") and len(r) and len(p)
    for q in QS:
        rs, pd, mx = O.depth([b], w, r, p, q)
        oc = O.discordant([b], j, mean, sd, 4, q)
        if len(w) == 0: assert mx == 0 and not rs.any() and not pd.any()
        else: assert mx > 0 and rs.all()
        assert len(oc) == len(j) and (len(j) == 0 or oc.sum() > 0)


# ---------------------------------------------------------------------------------------------------------------------
# a second plain implementation, and the oracle's answers are not trivial
# ---------------------------------------------------------------------------------------------------------------------
def depth_model(b, q, windows, ranges, points):
    """-> range sums, point depths, max depth.  Per contig a difference array over the columns its reads cover: +1 where an M operation begins, -1
    behind its end; the running sum, masked by the windows' columns.  Reads: MAPQ >= q, none of UNMAP | SECONDARY | QCFAIL | DUP.  No read cap: the
    caller asserts that the depth stays far below it."""
    n = len(b["tid"])
    nc = b["n_cigar"].astype(np.int64)
    rec = np.repeat(np.arange(n), nc)
    op, ln = (b["cigar"] & 15).astype(np.int64), (b["cigar"] >> 4).astype(np.int64)
    adv = np.where((op == 0) | (op == 2) | (op == 3), ln, 0)
    before = np.cumsum(adv) - adv
    first = np.repeat(before[np.minimum(b["cigar_off"].astype(np.int64), max(len(before) - 1, 0))], nc) if len(before) else before
    col = b["pos"].astype(np.int64)[rec] + 1 + before - first                         # 1-based column an operation begins at
    ok = (b["mapq"].astype(np.int64) >= q) & ((b["flag"] & W.F_DEPTH_MASK) == 0) & (b["tid"] >= 0)
    covers = (op == 0) & (ln > 0) & ok[rec]
    contig = {}
    for t in np.unique(b["tid"][rec][covers]).tolist():
        m = covers & (b["tid"][rec] == t)
        lo, hi = int(col[m].min()), int((col[m] + ln[m]).max())
        diff = np.zeros(hi - lo + 1, np.int64)
        np.add.at(diff, col[m] - lo, 1)
        np.add.at(diff, col[m] + ln[m] - lo, -1)
        depth = np.cumsum(diff)[:-1]
        inside = np.zeros(len(depth), bool)
        for wt, beg, end in windows.tolist():
            if wt == t:
                inside[min(max(beg - lo, 0), len(depth)):min(max(end + 1 - lo, 0), len(depth))] = True
        depth = depth * inside
        contig[t] = (lo, depth, np.concatenate(([0], np.cumsum(depth))))
    mx = max([int(d.max()) for _, d, _ in contig.values()] + [0])
    rs = np.zeros(len(ranges), np.uint64)
    for k, (t, beg, end) in enumerate(ranges.tolist()):
        if t in contig:
            lo, d, pre = contig[t]
            a, z = min(max(beg - lo, 0), len(d)), min(max(end + 1 - lo, 0), len(d))
            rs[k] = pre[z] - pre[a]
    pd = np.zeros(len(points), np.int32)
    for k, (t, c, _) in enumerate(points.tolist()):
        if t in contig and 0 <= c - contig[t][0] < len(contig[t][1]):
            pd[k] = contig[t][1][c - contig[t][0]]
    return rs, pd, mx


def discordant_model(b, junctions, mean, sd, times, q):
    """FindDiscordantReadPairs per junction over ALL records: the index query's candidate rule (tid, calend > beg, pos < end) brute force, then the
    read's own conditions and the strand geometry of getsv.cpp:1069-1113 in int64"""
    i64 = lambda k: b[k].astype(np.int64)
    tid, pos, mtid, mpos, lq, isize, flag = i64("tid"), i64("pos"), i64("mtid"), i64("mpos"), i64("l_qseq"), i64("isize"), i64("flag")
    calend = W.calends(b)
    nc = b["n_cigar"].astype(np.int64)
    off = np.minimum(b["cigar_off"].astype(np.int64), len(b["cigar"]) - 1)
    first_op = np.where(nc > 0, b["cigar"][off] & 15, 0)
    last_op = np.where(nc > 0, b["cigar"][np.minimum(off + np.maximum(nc, 1) - 1, len(b["cigar"]) - 1)] & 15, 0)
    rev, mrev = (flag & 16) != 0, (flag & 32) != 0
    lo, hi = mean - sd * times, mean + sd * times
    concordant = (~rev & mrev & (lo <= isize) & (isize <= hi)) | (rev & ~mrev & (isize < 0) & (lo <= -isize) & (-isize <= hi))
    read_ok = (b["mapq"].astype(np.int64) >= q) & (first_op != 5) & (last_op != 5) & ((flag & (1024 | 4 | 8)) == 0) & ~concordant
    min_ins, max_ins = max(lo, 0), hi
    out = np.zeros(len(junctions), np.int32)
    for k, j in enumerate(junctions):
        up, down, us, ds = int(j["up_pos"]), int(j["down_pos"]), chr(j["up_strand"]), chr(j["down_strand"])
        m = (tid == int(j["up_tid"])) & (calend > int(j["beg"])) & (pos < int(j["end"])) & read_ok
        m &= (int(j["down_tid"]) != -1) & (mtid == int(j["down_tid"]))
        if us == "+" and ds == "+":
            ins = up - pos + mpos + lq - down + 1
            m &= (pos + lq <= up + 5) & (mpos + 1 >= down - 5) & ~rev & mrev
            step = up - down + 1
            tandem = (int(j["up_tid"]) == int(j["down_tid"])) & (up > down) & (step + 2 * lq <= max_ins)
            rounds = np.maximum(0, -((ins - min_ins) // max(step, 1))) if step > 0 else np.zeros_like(ins)   # additions of step until ins >= min_ins
            hit = np.where(tandem, ins + rounds * step <= max_ins, (min_ins <= ins) & (ins <= max_ins))
        elif us == "-" and ds == "+":
            ins = pos + 1 - up + 1 + mpos + lq - down + 1
            hit = rev & mrev & (mpos + 1 >= down - 5) & (min_ins <= ins) & (ins <= max_ins)
        elif us == "+" and ds == "-":
            ins = up - pos + down - (mpos + lq) + 1
            hit = ~rev & ~mrev & (pos + lq <= up + 5) & (mpos + lq <= down + 5) & (min_ins <= ins) & (ins <= max_ins)
        else:
            hit = np.zeros(len(pos), bool)
        out[k] = int((m & hit).sum())
    return out


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("name", W.CASES)
def test_oracle_equals_the_plain_models_and_is_not_trivial(name, q):
    names, lens, b, j, w, r, p, mean, sd = W.case(name)
    oc = O.discordant([b], j, mean, sd, 4, q)
    rs, pd, mx = O.depth([b], w, r, p, q)
    assert np.array_equal(oc, discordant_model(b, j, mean, sd, 4, q))
    mrs, mpd, mmx = depth_model(b, q, w, r, p)
    assert np.array_equal(rs, mrs), np.flatnonzero(rs != mrs)[:8]
    assert np.array_equal(pd, mpd), np.flatnonzero(pd != mpd)[:8]
    assert mx == mmx < 7000                                   # far below the pileup's cap of 8,000 reads: the cap's own edges are tests/pileup_cap_*'s
    if name.startswith("nothing_to_do"):
        return
    # not a comparison of zeros with zeros
    assert oc.sum() > 0 and np.all(oc[W.DESIGNED[name]] >= 3)  # every junction that was given pairs counts them (3 or 4 each)
    assert mx > 0 and rs.sum() > 0
    inside = np.array([bool(np.any((w["tid"] == t) & (w["beg"] <= c) & (c <= w["end"]))) for t, c, _ in p.tolist()])
    assert inside.sum() >= 2 and (pd[inside] == 0).sum() * 2 < inside.sum()
    if name == "outside_queries":
        assert not pd[~inside].any() and (~inside).sum() >= 9
