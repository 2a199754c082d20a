"""CPU: the designed inputs of tests/clip_events_inputs.py.  (a) The module's constants are the headers'.  (b) Every input reaches the edge it is
named for - read from the model's report (tests/clip_events_model.py), so that a change of the generator or of a kernel's constants that moves
an input off its edge fails here and does not leave tests/test_clip_events_gpu.py green and empty.  (c) The model's table equals the C oracle's
on every input and run, all keys and the event counts (the range cases: the oracle gets the cut batches and the contig the cut left behind), and
equals cluster_bins_model.getclip_model wherever that model applies (whole inputs without ownership).  (d) Where the real reference defines the
result it wrote the same clip and clip.fq texts: their sha256 lie in tests/golden/clip_events/reference.json, made by
tests/golden/make_clip_events_reference.py with oracle/_ref/seeksv_ref - no reference binary is needed here, so nothing is skipped."""
import hashlib
import json
import os
import re

import pytest

import clip_events_inputs as I
import clip_events_model as M
import golden_util as G
import oracle_lib as O
from cluster_bins_model import F_MUNMAP, F_UNMAP, getclip_model
from seeksv_amd import host
from test_hip_golden import assert_tables_equal

CSRC = os.path.join(O.ROOT, "seeksv_amd", "csrc")
ALL = I.names()


def test_constants_are_the_headers():
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("clip_kernels.h", "tile_sort.h", "common.h")}

    def const(f, name):
        m = re.search(r"constexpr\s+int\s+(?:\w+\s*=\s*\d+\s*,\s*)*" + name + r"\s*=\s*(\d+)\s*[;,]", text[f])
        assert m, (f, name)
        return int(m.group(1))

    clip = text["clip_kernels.h"]
    assert const("common.h", "BLOCK") == I.BLOCK and const("common.h", "WAVE") == I.WAVE
    assert re.search(r"constexpr\s+int\s+CC_TILE\s*=\s*BLOCK\s*\*\s*32\s*;", clip) and I.BLOCK * 32 == I.CC_TILE
    assert const("clip_kernels.h", "CE_ITEMS") == I.CE_ITEMS and const("clip_kernels.h", "CE_SUB") == I.CE_SUB
    assert I.BLOCK * I.CE_ITEMS == I.SUB_TILE and I.SUB_TILE * I.CE_SUB == I.CC_TILE
    assert const("tile_sort.h", "WS_W") == I.WS_W and const("tile_sort.h", "WS_TILE") == I.WS_TILE
    assert const("clip_kernels.h", "GROUP") == I.GROUP
    assert re.search(r"for \(int shift = 0; shift < key_bits; shift \+= (\d+)\)", open(os.path.join(CSRC, "radix_sort.h")).read()).group(1) == str(I.RADIX_BITS)
    # k_clip_filter: four lanes per candidate, so 16 candidates a wavefront and 64 a workgroup; the per-wavefront counts go by c >> 4
    body = clip.split("void k_clip_filter(", 1)[1].split("\n}\n", 1)[0]
    assert re.search(r"const int64_t c = t >> 2;", body) and re.search(r"wave_cnt\[c >> 4\]", body)
    assert I.WAVE // 4 == I.FILTER_WAVE and I.BLOCK // 4 == I.FILTER_BLOCK
    # five operations lie in a record's line
    assert re.search(r"return k < (\d+) \? head\(k\)", clip).group(1) == str(I.LINE_OPS) and re.search(r"uint32_t cig\[(\d+)\];", clip).group(1) == str(I.LINE_OPS)
    # k_clip_gather: an unrolled batch of 8 dwords per lane of a group
    body = clip.split("void k_clip_gather(", 1)[1].split("\n}\n", 1)[0]
    assert re.search(r"constexpr int BATCH = (\d+);", body).group(1) == str(I.GATHER_BATCH) and I.GATHER_DWORDS == 128
    assert I.CAND_COUNTS == (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025) and I.TILE_DELTAS == (-17, -16, -15, -1, 0, 1, 15, 16, 17)
    assert I.GAPS == (0, 1, 15, 16, 300) and I.CONTIG_IDS == (1, 2, 255, 256, 257, 4096, 70000)
    assert I.GATHER_LQ == (1, 2, 3, 5, 340, 341, 342, 343, 600) and I.GATHER_NCIG == (5, 6, 7, 21, 300)
    assert max(len(x["recs"]) for x in I.inputs().values()) <= I.MAX_RECORDS == 5 * I.CC_TILE + 17
    assert sorted({x["family"] for x in I.inputs().values()}) == sorted(I.FAMILIES) and all(I.inputs()[n]["family"] == f for n, f in zip(I.FORMS, ("gather", "ends", "tile_edges", "candidate_counts", "contig_switch", "ranges_and_ownership", "side_order")))


# ---------------------------------------------------------------------------------------------------------------------
# (b) every family reaches its edges
# ---------------------------------------------------------------------------------------------------------------------
def one_pass(name, tag="d"):
    t, per_pass = I.modelled(name, tag)
    assert len(per_pass) == 1
    return t, per_pass[0][0], I.report_of(name, tag)[0]


def test_ends_meet_every_byte_lane():
    seen = set()
    for name in I.names("ends"):
        x = I.inputs()[name]
        b = I.batch_of(x["recs"])
        t, ev, rep = one_pass(name)
        want = [i for i, e in enumerate(b["cigar_ends"]) if e != 0xff and (e & 15 == 4 or e >> 4 == 4)]
        assert rep["batches"][0]["cand"] == want
        seen |= {(int(e), i % I.CE_ITEMS) for i, e in enumerate(b["cigar_ends"])}
        # an S at either end gives events unless the other end is an H
        emit = sorted({e.rec for e in ev})
        assert emit == [i for i in want if 5 not in (b["cigar_ends"][i] & 15, b["cigar_ends"][i] >> 4)] and len(emit) >= 15
    values = {a | b << 4 for a in range(9) for b in range(9)} | {0xff}
    assert seen == {(v, lane) for v in values for lane in range(I.CE_ITEMS)}
    x = I.inputs()["ends-0"]
    assert sum(1 for r in x["recs"] if not r["ops"]) == 1 and sum(1 for r in x["recs"] if len(r["ops"]) == 1) == 9


def test_tile_edge_sizes_and_places():
    sizes = I.tile_edge_sizes()
    assert sizes == [k * I.CC_TILE + d for k in range(3) for d in I.TILE_DELTAS if k * I.CC_TILE + d > 0] and len(sizes) == 22
    assert {n % I.CE_ITEMS for n in sizes} == {0, 1, 15} and {n % I.CC_TILE for n in sizes} >= {0, 1, I.CC_TILE - 1}
    for n in sizes + [5 * I.CC_TILE + 1]:
        for tail in ("", "-tail") if n != 5 * I.CC_TILE + 1 else ("",):
            name = f"tile-{n}{tail}"
            x = I.inputs()[name]
            t, ev, rep = one_pass(name)
            B = rep["batches"][0]
            assert B["n"] == n == len(x["recs"]) and B["cand"] == x["expect"]["places"]
            cand = set(B["cand"])
            assert {0, n - 1} <= cand
            ntiles = (n + I.CC_TILE - 1) // I.CC_TILE
            assert len(B["tiles"]) == ntiles and len(B["sub_tiles"]) == (n + I.SUB_TILE - 1) // I.SUB_TILE
            for tl in range(ntiles):
                a = tl * I.CC_TILE
                for p in (0, I.CE_ITEMS - 1, I.CE_ITEMS, 1023, 1024, I.SUB_TILE - 1, I.SUB_TILE, I.CC_TILE - 1):
                    assert a + p >= n or a + p in cand
            tail_start = (n - 1) // I.CC_TILE * I.CC_TILE
            if tail:
                assert B["tiles"][-1] == n - tail_start and set(range(tail_start, n)) <= cand
            else:
                assert all(c <= len(I.TILE_PLACES) + 1 for c in B["tiles"]) and t["n_events"] < 12 * ntiles
                if n % I.CC_TILE == 1:   # the tile that holds one record, its last, as its only candidate
                    assert B["tiles"][-1] == 1 and B["cand"][-1] == n - 1
            # every candidate kind at the places: '5' only, '3' only, both, and one that only -q 0 lets in
            if len(B["cand"]) >= 4:   # (n = 1: one candidate)
                assert {len([e for e in ev if e.rec == i]) for i in B["cand"]} == {0, 1, 2}
                assert I.modelled(name, "q0")[0]["n_events"] > t["n_events"]
    x = I.inputs()["tile-empty-middle"]
    B = one_pass("tile-empty-middle")[2]["batches"][0]
    assert B["tiles"][1] == 0 and B["tiles"][0] >= 8 and B["tiles"][2] >= 8 and B["sub_tiles"][2:4] == [0, 0]
    B = one_pass(f"tile-{5 * I.CC_TILE + 1}")[2]["batches"][0]
    assert len(B["tiles"]) == 6 and B["tiles"][-1] == 1 and all(B["tiles"])


@pytest.mark.parametrize("n", I.CAND_COUNTS)
def test_candidate_counts_and_patterns(n):
    W, FB, BL = I.FILTER_WAVE, I.FILTER_BLOCK, I.BLOCK
    assert {W - 1, W, W + 1, FB - 1, FB, FB + 1, BL - 1, BL, BL + 1} <= set(I.CAND_COUNTS)
    have = [p for p in I.PATTERNS if f"count-{n}-{p}" in I.inputs()]
    assert set(have) >= {"both", "none", "3", "5", "alt", "lone0"} and (n < 3 * W or "gap" in have) and (n <= 63 or set(have) == set(I.PATTERNS))
    for p in have:
        name = f"count-{n}-{p}"
        t, ev, rep = one_pass(name)
        B = rep["batches"][0]
        assert len(B["cand"]) == n and len(B["per_seg"]) == (n + W - 1) // W and len(B["per_block"]) == (n + BL - 1) // BL
        full = n // W
        if p == "both":   # every slot of every filter wavefront taken
            assert B["per_seg"][:full] == [2 * W] * full and sum(B["per_seg"]) == 2 * n and rep["n5"] == rep["n3"] == n
        elif p == "none":
            assert t["n_events"] == 0 and (n < 4 or (I.modelled(name, "q0")[0]["n_events"] > 0 and I.modelled(name, "s")[0]["n_events"] > 0))
        elif p == "3":
            assert (rep["n5"], rep["n3"]) == (0, n)
        elif p == "5":
            assert (rep["n5"], rep["n3"]) == (n, 0)
        elif p == "alt":
            assert set(B["per_cand"]) == ({0, 1, 2} if n >= 4 else {0}) and (n < 5 or I.modelled(name, "s")[0]["n_events"] > t["n_events"])
        elif p == "gap":
            assert B["per_seg"][:3] == [2 * W, 0, 2 * W]
            assert all(I.report_of(name, tag)[0]["batches"][0]["per_seg"][:3] == [2 * W, 0, 2 * W] for tag in ("q0", "s"))
        else:
            place = int(p[4:])
            for tag in ("d", "q0", "s"):
                pc = I.report_of(name, tag)[0]["batches"][0]["per_cand"]
                hit = [k for k, c in enumerate(pc) if c]
                assert len(hit) == 1 and hit[0] % BL == place and pc[hit[0]] == (1, 1, 2)[place % 3]
                last = (n - 1) // BL
                assert hit[0] // BL == (last if last * BL + place < n else 0)   # the last workgroup of k_clip_place that has the place


@pytest.mark.parametrize("name", I.names("contig_switch"))
def test_contig_switch_inputs(name):
    x = I.inputs()[name]
    recs, gap = x["recs"], x["expect"]["gap"]
    t, ev, rep = one_pass(name)
    assert sorted({e.rec for e in ev}) == x["expect"]["kept"] and recs[0]["tid"] == x["initial_last_tid"] and ev[0].rec == 0
    for a, b in x["expect"]["runs"]:
        assert b - a == gap and all(r["flag"] & (F_UNMAP | F_MUNMAP) for r in recs[a:b]) and (a == 0 or not recs[a - 1]["flag"] & 12)
        assert all(r["tid"] not in (recs[a - 1]["tid"],) for r in recs[a:b]) and (gap < 4 or any(M.is_candidate(r) for r in recs[a:b]))
    # without the rule that unmapped-pair records do not count the second records were dropped: their neighbours are on another contig
    for i in x["expect"]["kept"][2:]:
        assert gap == 0 or recs[i - 1]["tid"] != recs[i]["tid"]
    one = [tid for tid in {r["tid"] for r in recs} if sum(1 for r in recs if r["tid"] == tid and not r["flag"] & 12) == 1]
    assert len(one) == 2 and all(M.is_candidate(r) for r in recs if r["tid"] in one)
    cand = x["expect"]["kept"][2]
    assert [cand] in x["cutsets"]
    if gap:
        parts = [[recs[a:b] for a, b in zip([0] + c, c + [len(recs)])] for c in x["cutsets"]]
        assert any(all(r["flag"] & 12 for r in p) and len(p) == gap for cs in parts for p in cs)                   # a batch of unmapped-pair records only
        assert any(0 < sum(1 for r in p if r["flag"] & 12) < len(p) and p[-1]["flag"] & 12 for cs in parts for p in cs)   # a batch that ends inside / with a run
    if gap == 300:
        assert gap > I.BLOCK   # k_last_tid looks at BLOCK records a trip
        first = recs[:cand]
        assert all(r["flag"] & 12 for r in first[-gap:]) and not first[-gap - 1]["flag"] & 12


def test_ranges_and_ownership_inputs():
    recs = I.range_records()
    X = I.inputs()
    whole, _ = M.clip_events([(recs, None)])
    by_rec = lambda ev: sorted({e.rec for e in ev})

    def events(name):
        t, per_pass = I.modelled(name, "d")
        return [e for ev, _ in per_pass for e in ev]

    c = 45
    assert c in by_rec(whole) and 41 in by_rec(whole) and 40 not in by_rec(whole) and M.is_candidate(recs[40])
    assert by_rec(events("range-r0-on")) == [i for i in by_rec(whole) if i >= c]
    assert by_rec(events("range-r0-behind")) == [i for i in by_rec(whole) if i > c]
    assert by_rec(events("range-r1-on")) == [i for i in by_rec(whole) if i < c]
    assert by_rec(events("range-r1-behind")) == [i for i in by_rec(whole) if i <= c]
    assert events("range-empty") == [] and events("range-r1-zero") == []
    assert by_rec(events("range-r0-contig-first")) == [i for i in by_rec(whole) if i >= 40] and 41 in by_rec(events("range-r0-contig-first"))
    assert by_rec(events("range-r0-contig-second")) == [i for i in by_rec(whole) if i >= 41]   # record 40, in front of the range, is its contig's first
    assert len(events("range-two-passes")) == len(whole)
    for tag in "53":
        for edge in ("lo", "hi"):
            for d in (-1, 0, 1):
                x = X[f"own-{edge}-{tag}{d:+d}"]
                key = x["expect"]["key"]
                assert key.side == "53".index(tag) and key in whole
                inside = key in events(x["name"])
                assert inside == ((d <= 0) if edge == "lo" else (d > 0)), x["name"]
                assert 0 < len(events(x["name"])) < len(whole)
    for name in ("own-both-5in", "own-both-3in"):
        x = X[name]
        r = x["expect"]["rec"]
        assert [e.side for e in whole if e.rec == r] == [0, 1] and [e.side for e in events(name) if e.rec == r] == x["expect"]["sides"]
    ev = events("own-across")
    assert {e.tid for e in ev} == {0, 1, 2} and {e.tid for e in whole if e not in ev} == {0, 2}


def test_side_order_inputs():
    X = I.inputs()
    for where in ("start", "straddle"):
        for places in (I.WS_W, I.WS_W + 1):
            name = f"order-{where}-{places}"
            t, ev, rep = one_pass(name)
            assert rep["inversion3"] == places == X[name]["expect"]["inversion"] and rep["n5"] == 0 and rep["ascend5"]
            k3 = [M.sort_key(e) for e in ev]
            at = X[name]["expect"]["at"]
            assert k3[at] == max(k3[:at + places + 1]) and k3[at] > k3[at + places] and k3[at] < k3[at + places + 1]
            assert sum(1 for a, b in zip(k3, k3[1:]) if a > b) == 1   # one read out of place, nothing else
            if where == "straddle":
                assert at <= I.WS_TILE - 1 < I.WS_TILE <= at + places
    t, ev, rep = one_pass("order-equal-keys")
    bins = {}
    for e in ev:
        bins.setdefault((e.side, e.pos), []).append(e.rec)
    assert {k: len(v) for k, v in bins.items()} == X["order-equal-keys"]["expect"]["bins"]
    assert len({X["order-equal-keys"]["recs"][i]["pos"] for i in bins[(1, 224)]}) == 3 and all(v == sorted(v) for v in bins.values())
    t, ev, rep = one_pass("order-falling")
    assert not rep["ascend5"] and rep["inversion3"] > I.WS_W and len({e.tid for e in ev}) == 1
    dup = [k for k in {(e.side, e.pos) for e in ev} if sum(1 for e in ev if (e.side, e.pos) == k) == 2]
    assert {s for s, _ in dup} == {0, 1} and len(dup) == 4
    t, ev, rep = one_pass("order-contig-ids")
    with_events = {tid: {e.side for e in ev if e.tid == tid} for tid in I.CONTIG_IDS}
    assert with_events[1] == {0} and with_events[2] == {1} and with_events[257] == set() and with_events[70000] == {0, 1}
    assert {e.tid for e in ev} == set(I.CONTIG_IDS) - {257} and rep["max_key"] >> 33 == 70000 > 256 * I.BLOCK and rep["ascend5"] and rep["inversion3"] <= I.WS_W
    t, ev, rep = one_pass("order-key-bits")
    top = rep["max3"] >> 33
    assert rep["inversion3"] == I.WS_W + 1 and rep["max_key"] == rep["max3"] and top & (top - 1) == 0 and top > rep["max5"] >> 33
    digits = lambda key: (int(key).bit_length() + I.RADIX_BITS - 1) // I.RADIX_BITS
    assert rep["key_bits"] == int(rep["max3"]).bit_length() and digits(rep["max3"]) == digits(rep["max5"]) + 1 and top == I.KEY_BITS_CONTIG == 128
    assert len({e.tid for e in ev if e.side == 1}) > 1   # '3' keys on both sides of the bit that only the '3' list gives


def test_gather_input():
    x = I.inputs()["gather"]
    (recs, b), = I.batches_of(x)
    entries = x["expect"]["entries"]
    seen = {}
    for i, mis, lq, nc in entries:
        assert int(b["seq_off"][i]) % 4 == mis and recs[i]["lq"] == lq and len(recs[i]["ops"]) == nc and M.is_candidate(recs[i])
        seen.setdefault((lq, nc), set()).add(mis)
    assert all(v == {0, 1, 2, 3} for v in seen.values())
    assert {lq for lq, nc in seen} == set(I.GATHER_LQ) and {nc for lq, nc in seen if lq >= 340} == set(I.GATHER_NCIG)
    assert all((lq, nc) in seen for lq in I.GATHER_LQ if lq >= 340 for nc in I.GATHER_NCIG)
    dwords = lambda lq: ((lq + 1) // 2 + lq + 3) // 4
    assert dwords(340) == dwords(341) == I.GATHER_DWORDS and dwords(342) == dwords(343) == I.GATHER_DWORDS + 1 and (341 + 1) // 2 + 341 == 4 * I.GATHER_DWORDS
    assert min(I.GATHER_NCIG) == I.LINE_OPS and max(I.GATHER_NCIG) > I.GROUP * 16
    # reads of odd length in front of the entries that are off a dword; the last entry ends where the blob ends
    between = [r for r in recs if not M.is_candidate(r)]
    assert len(between) >= 40 and {r["lq"] for r in between} == {1, 2, 3} and {(r["lq"] + 1) // 2 + r["lq"] for r in between} == {2, 3, 5}
    i, mis, lq, nc = entries[-1]
    assert i == len(recs) - 1 and int(b["seq_off"][i]) + (lq + 1) // 2 + lq == len(b["seqqual"]) == x["expect"]["nbytes"] and mis == 3 and lq == 600
    t, ev, rep = one_pass("gather")
    assert {e.rec for e in ev} == {i for i, _, _, _ in entries} and rep["n5"] > 50 and rep["n3"] > 50


# ---------------------------------------------------------------------------------------------------------------------
# (c) the model against the oracle and the second model
# ---------------------------------------------------------------------------------------------------------------------
def last_mapped_tid(recs, default):
    for r in reversed(recs):
        if not r["flag"] & (F_UNMAP | F_MUNMAP):
            return r["tid"]
    return default


def oracle_table(x, tag):
    kw = I.RUN_KW[tag]
    opts = dict(ship_all=x.get("ship_all", False), pad=x.get("pad", True))
    if x["kind"] == "getclip":
        return O.getclip([I.batch_of(x["recs"], **opts)], own=x["own"], initial_last_tid=x["initial_last_tid"], **kw)
    tables = []
    for p in I.passes_of(x):
        state, first, cut = p["initial_last_tid"], None, []
        for recs, (r0, r1) in p["scans"]:
            state = last_mapped_tid(recs[:r0], state)
            if first is None:
                first = state
            else:
                assert state == left   # (the cut batches follow each other for the oracle: what lies in front of a later range must leave the contig the range before left)
            cut.append(recs[r0:r1])
            left = state = last_mapped_tid(recs[r0:r1], state)
        tables.append(O.getclip([I.batch_of(c, **opts) for c in cut if c] or [I.batch_of(x["recs"][:0])], initial_last_tid=first, **kw))
    return host.concat_tables(tables) if len(tables) > 1 else tables[0]


@pytest.mark.parametrize("name", ALL)
def test_model_equals_oracle(name):
    x = I.inputs()[name]
    for tag in x["runs"]:
        t, per_pass = I.modelled(name, tag)
        assert t["n_events"] == sum(len(ev) for ev, _ in per_pass)
        assert_tables_equal(t, oracle_table(x, tag))
        if x["kind"] == "getclip" and x["own"] is None:
            assert_tables_equal(t, getclip_model(x["recs"], initial_last_tid=x["initial_last_tid"], **I.RUN_KW[tag])[0])
        for ev, scans in per_pass:   # (b) is (a) in the order of the keys, BAM order kept inside a bin
            order = M.table_order(ev)
            keys = [M.sort_key(e) for e in order]
            assert keys == sorted(keys) and all(ev.index(a) < ev.index(b) for a, b in zip(order, order[1:]) if M.sort_key(a) == M.sort_key(b))


# ---------------------------------------------------------------------------------------------------------------------
# (d) the real reference
# ---------------------------------------------------------------------------------------------------------------------
def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


@pytest.fixture(scope="module")
def reference():
    with open(os.path.join(G.GOLDEN, "clip_events", "reference.json")) as f:
        return json.load(f)


def test_reference_covers_what_it_defines(reference):
    defined = [n for n in ALL if I.reference_defined(I.inputs()[n])]
    assert sorted(reference) == sorted(defined) and len(defined) >= 170
    assert {I.inputs()[n]["family"] for n in defined} == set(I.FAMILIES) - {"ranges_and_ownership"}   # (ownership and ranges: the reference has neither)


@pytest.mark.parametrize("name", [n for n in ALL if I.reference_defined(I.inputs()[n])])
def test_model_equals_reference(reference, name):
    x = I.inputs()[name]
    want = reference[name]
    assert sorted(want) == sorted(x["runs"])
    for tag in x["runs"]:
        t, _ = I.modelled(name, tag, True)
        clip, fq = host.format_clip_outputs(t, x["names"])
        assert sha(clip) == want[tag]["clip"], tag
        assert sha(fq) == want[tag]["fq"], tag
        assert t["n_clusters"] == want[tag]["rows"]
