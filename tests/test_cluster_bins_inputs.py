"""CPU: the designed samples of tests/cluster_bins_inputs.py hold what their families claim - read from the model's per-bin report, so that a
change of the generator (or of a kernel's constants) that silently moves an input off its path fails here, not nowhere."""
import math
import os
import re

import pytest

import cluster_bins_inputs as I
from cluster_bins_model import _strings, minm, rate_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{f}-{c}" for f, c in I.SAMPLE_IDS]
SWEEPS = [f for f in I.FAMILIES if f[0] == "a"]


def test_constants_are_the_headers():
    text = "".join(open(os.path.join(ROOT, "seeksv_amd", "csrc", f)).read() for f in ("clip_kernels.h", "common.h"))
    for name, value in I.CONSTANTS.items():
        m = re.findall(r"^constexpr int %s = (\d+);" % name, text, re.M)
        assert m == [str(value)], (name, m)
    assert re.findall(r"^constexpr int BIN_SL = (\w+);", text, re.M) == ["PACK_MAX_LQ"]


def bin_of(bins):
    return {(b["tid"], b["side"], b["pos"]): b for b in bins}


def rate_of(tag):
    return I.RUN_KW[tag].get("match_rate", 0.9)


AIMED = [(f, c) for f, c in I.SAMPLE_IDS if f != "c"]   # (family c aims at depths, not at clusters: test_bin_depths_and_the_ends_of_the_event_list)


@pytest.mark.parametrize("family,cls", AIMED, ids=[f"{f}-{c}" for f, c in AIMED])
def test_every_joiner_lands_in_its_cluster(family, cls):
    s = I.sample(family, cls)
    checked = 0
    for tag, _, kw in I.runs_of(family):
        t, bins, recs = I.modelled(family, cls, tag)
        rate = rate_of(tag)
        landed = {(recs[i]["tag"], (b["tid"], b["side"], b["pos"])): k for b in bins for i, k in zip(b["recs"], b["assign"])}
        for rtag, (key, k, rates) in s["aims"].items():
            if rate in rates if rates is not None else rate > 0:
                assert landed[(rtag, key)] == k, (tag, rtag, key)
                checked += 1
    assert checked >= 100


@pytest.mark.parametrize("family,cls", I.SAMPLE_IDS, ids=IDS)
def test_length_class_and_entry_alignments(family, cls):
    """the longest clipped read is the class's; among the events of multi-event bins all four misalignments of a read's entry (its offset in the
    batch's bytes) meet both parities of the base the right side starts at"""
    s = I.sample(family, cls)
    t, bins, recs = I.modelled(family, cls, I.runs_of(family)[0][0])
    longest = max(r["lq"] for r in recs if I.events_of(r))
    own = {"a": I.B4_CAP, "d": I.B4_CAP}.get(family[0], 0)   # the sweep and the merge rules reach 256 bases themselves
    assert longest == (max(cls, own) if cls else own or longest) and (cls or longest <= I.B4_CAP)
    if cls > I.B4_CAP:
        assert longest > I.B4_CAP   # k_cluster_bins
    seen = set()
    for b in bins:
        if b["n_events"] > 1:
            for i in b["recs"]:
                for side, pos, begin, ll, lr in I.events_of(recs[i]):
                    if "53"[side] == b["side"] and pos == b["pos"]:
                        seen.add((int(s["batch"]["seq_off"][i]) & 3, (begin + ll) & 1))
    assert len(seen) == 8, sorted(seen)


@pytest.mark.parametrize("cls", I.CLASSES)
def test_cluster_counts(cls):
    t, bins, recs = I.modelled("b", cls, "t090")
    B = bin_of(bins)
    want = I.sample("b", cls)["expect"]["clusters"]
    assert sorted({K for K, key in want}) == sorted(I.COUNTS) and {1, 2, 3, 4, 5, 63, 64, 65, 66, 70} <= set(I.COUNTS)
    for K, key in want:
        assert B[key]["n_clusters"] == K, key
    for side in "53":
        assert {K for K, key in want if key[1] == side} == set(I.COUNTS)
    # the event between an early and a late cluster: it passes the late founder on both sides, the early cluster took it
    for xtag, ltag, key, early in I.sample("b", cls)["both"]:
        x, l = (next(r for r in recs if r["tag"] == g) for g in (xtag, ltag))
        (sx, px, bx, llx, lrx), (sl_, pl, bl, lll, lrl) = I.events_of(x)[0], I.events_of(l)[0]
        xs, ls = _strings(x, bx, llx, lrx), _strings(l, bl, lll, lrl)
        n1, n2 = min(llx, lll), min(lrx, lrl)
        assert rate_ok(int((xs[0][llx - n1:] == ls[0][lll - n1:]).sum()), n1, 0.9) and rate_ok(int((xs[2][:n2] == ls[2][:n2]).sum()), n2, 0.9)
        b = B[key]
        assert b["assign"][[recs[i]["tag"] for i in b["recs"]].index(xtag)] == early < B[key]["n_clusters"] - 1
    assert len(I.sample("b", cls)["both"]) == 2 * sum(1 for K in I.COUNTS if K >= 5)
    # the cuts fall inside a deep bin and inside a bin of more than CL_CACHE clusters
    cuts = I.cuts_of("b", cls)
    many = max(bins, key=lambda b: b["n_clusters"])
    assert many["n_clusters"] > I.CL_CACHE and any(min(many["recs"]) < c <= max(many["recs"]) for c in cuts)


@pytest.mark.parametrize("cls", [c for c in I.CLASSES if c])
def test_class_bins_of_the_class_length(cls):
    t, bins, recs = I.modelled("e", cls, "t090")
    B = bin_of(bins)
    want = I.sample("e", cls)["expect"]["clusters"]
    assert sorted(K for K, key in want) == [5, 5, 66, 66]
    for K, key in want:
        assert B[key]["n_clusters"] == K
        assert max(recs[i]["lq"] for i in B[key]["recs"]) == cls
    if cls > I.B4_CAP + 2:   # sides of 255 and 256 bases, equal and one longer
        sides = {(int(t["left_len"][k]), int(t["right_len"][k])) for k in range(t["n_clusters"])}
        assert {x for lr in sides for x in lr} >= {255, 256, 257}


@pytest.mark.parametrize("cls", I.CLASSES)
def test_bin_depths_and_the_ends_of_the_event_list(cls):
    s = I.sample("c", cls)
    assert not s["aims"]   # (why test_every_joiner_lands_in_its_cluster leaves this family out)
    for tag, _, kw in I.RUNS:
        t, bins, recs = I.modelled("c", cls, tag)
        B = bin_of(bins)
        want = s["expect"]["depths"]
        assert {d for d, key in want} >= set(I.DEPTHS) and {2, 15, 16, 17, 63, 64, 65, 66, 128, 129, 130} <= set(I.DEPTHS)
        for d, key in want:
            assert B[key]["n_events"] == d, key
        for side in "53":
            assert {d for d, key in want if key[1] == side} >= set(I.DEPTHS)
        # slot 0 is a deep '5' bin of contig 0; the last B4_DEEP slots are one '3' bin of the last contig, the table ends with its clusters
        first, last = bins[0], bins[-1]
        assert (first["tid"], first["side"], first["pos"]) == s["expect"]["first"] and first["side"] == "5" and first["n_events"] > I.CL_CACHE
        assert (last["tid"], last["side"], last["pos"]) == s["expect"]["last"] and last["side"] == "3" and last["tid"] == 2 and last["n_events"] == I.B4_DEEP
        assert last["row0"] + last["n_clusters"] == t["n_clusters"]
    # '3' bins: events of records that start at different places, records of other bins in between
    mixed = 0
    for b in bins:
        if b["side"] == "3" and b["n_events"] >= I.B4_DEEP:
            starts = [recs[i]["pos"] for i in b["recs"]]
            mixed += len(set(starts)) > 5 and b["recs"][-1] - b["recs"][0] + 1 > len(b["recs"])
    assert mixed >= 8
    cuts = I.cuts_of("c", cls)
    deep = max(bins, key=lambda b: b["n_events"])
    assert deep["n_events"] >= 128 and any(min(deep["recs"]) < c <= max(deep["recs"]) for c in cuts)


@pytest.mark.parametrize("family", SWEEPS)
@pytest.mark.parametrize("cls", sorted(I.SWEEP_OWN))
def test_sweep_reaches_both_verdicts_for_every_overlap(family, cls):
    tag = "t" + family[1:]
    rate = rate_of(tag)
    nmax, cap = I.SWEEP_OWN[cls]
    t, bins, recs = I.modelled(family, cls, tag)
    B = bin_of(bins)
    got = {}
    for n, deciding, verdict, key in I.sample(family, cls)["expect"]["sweep"]:
        b = B[key]
        assert b["n_events"] == 2 and b["n_clusters"] == (1 if verdict == "join" else 2), (n, deciding, verdict)
        # the overlap of the deciding side is n and it matches in exactly minm(n) or minm(n) - 1 places; the other side is the same
        (e1, e2) = (I.events_of(recs[i])[0] for i in b["recs"])
        s1, s2 = _strings(recs[b["recs"][0]], *e1[2:]), _strings(recs[b["recs"][1]], *e2[2:])
        nl, nr = min(e1[3], e2[3]), min(e1[4], e2[4])
        ml, mr = int((s1[0][e1[3] - nl:] == s2[0][e2[3] - nl:]).sum()), int((s1[2][:nr] == s2[2][:nr]).sum())
        (nd, md), (no, mo) = ((nl, ml), (nr, mr)) if deciding == "L" else ((nr, mr), (nl, ml))
        assert nd == n and md == minm(n, rate) - (verdict == "new") and mo == no >= 1
        got.setdefault(n, set()).add((deciding, verdict))
    verdicts = {(d, v) for d in "LR" for v in (("join", "new") if rate > 0 else ("join",))}
    assert sorted(got) == list(range(1, nmax + 1)) and all(got[n] == verdicts for n in got)
    assert max(r["lq"] for r in recs) == cap
    listed = {0.55: (100, 180, 200, 220, 340), 0.56: (25, 50, 75, 100, 150), 0.68: (75, 150, 175, 300, 325)}.get(rate)
    if listed:   # where a table of ceil(rate * n) would ask for one match more than the division does
        hit = [n for n in listed if n <= nmax and minm(n, rate) != math.ceil(rate * n)]
        assert hit and all(minm(n, rate) == math.ceil(rate * n) - 1 for n in hit)
    else:
        assert all(minm(n, rate) == math.ceil(rate * n) for n in range(1, nmax + 1))


def test_merge_rule_inputs():
    t, bins, recs = I.modelled("d", 0, "t090")
    lens = {(int(t["left_len"][k]), int(t["right_len"][k])) for k in range(t["n_clusters"])}
    for s in (0, 1, 2, 3, 4, 5, 6, 255):
        assert any(l == s for l, r in lens) and any(r == s for l, r in lens), s
    quals = {int(q) for r in recs for q in r["qual"]}
    assert quals == set(I.QUALS) | {255} and max(I.QUALS) == 93
    assert sum(1 for r in recs if not r["ref"]) >= 20 and sum(1 for r in recs if r["qual"][0] == 255) >= 4
    assert int(t["qual_missing"].sum()) >= 2 and any(len(I.events_of(r)) == 2 and r["ops"][0][0] in (1, 2, 3) for r in recs)
    # a left side of 1 - 3 bases at the very start of a read, in a '5' bin of several events
    B = bin_of(bins)
    short = {recs[i]["ops"][0][0] for b in bins if b["side"] == "5" and b["n_events"] > 1 for i in b["recs"] if recs[i]["ops"][0][1] == "S"}
    assert {1, 2, 3} <= short
    # the carrier rule shows: clusters whose CIGAR is not their founder's
    moved = 0
    for b in bins:
        founders = {}
        for i, k in zip(b["recs"], b["assign"]):
            founders.setdefault(k, i)
        for k, i in founders.items():
            row = b["row0"] + k
            co, nc = int(t["cigar_off"][row]), int(t["n_cigar"][row])
            moved += [(int(c) >> 4, "MIDNSHP=X"[int(c) & 15]) for c in t["cigar"][co:co + nc]] != list(recs[i]["ops"])
    assert moved >= 20
