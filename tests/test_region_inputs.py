"""What tests/region_inputs.py says about its sets, asserted on the CPU: the answers written by hand against the model (tests/region_model.py), the model's
normalise() against the brute-force overlap over the list as given, and the sizes at which the kernels of seeksv_amd/csrc/region_kernels.h change path."""
import random

import pytest

import region_inputs as ri
import region_model as rm

IDS = [s["name"] for s in ri.SETS]


@pytest.mark.parametrize("s", ri.SETS, ids=IDS)
def test_hand_written_answers_and_the_normalised_list(s):
    recs, regions = s["records"], s["regions"]
    norm = rm.normalise(regions, s["lens"])
    # normalised: sorted, no two regions overlapping or abutting, inside the contigs
    assert norm == sorted(norm) and all(0 <= x[1] < x[2] <= s["lens"][x[0]] for x in norm)
    assert all(a[0] < b[0] or a[2] < b[1] for a, b in zip(norm, norm[1:]))
    for exclude, key in ((False, "kept"), (True, "kept_x")):
        got = rm.keep(recs, regions, exclude)
        # the list as given and the normalised one keep the same records (where a set's records reach past a contig's end, no region lies there)
        assert got == rm.keep(recs, norm, exclude)
        if key in s["claim"]:
            assert got == s["claim"][key]
    assert sorted(rm.keep(recs, regions) + rm.keep(recs, regions, True)) == list(range(len(recs)))
    assert [r["isize"] for r in recs] == list(range(len(recs)))
    assert all(r["tid"] < len(s["lens"]) and r["pos"] < s["lens"][r["tid"]] for r in recs if r["tid"] >= 0)


def test_grid():
    s = ri.BY_NAME["grid"]
    recs = s["records"]
    assert rm.normalise(s["regions"], s["lens"]) == ri.GRID_NORMALISED == s["claim"]["normalised"]
    assert s["lens"][1] == 64 and all(r["tid"] == 1 for r in recs) and {x[0] for x in s["regions"]} == {1}
    assert len(recs) == s["claim"]["n"] == 8 * 65 and len(recs) > 2 * ri.TILE and len(recs) % ri.GATHER_GROUP != 0
    assert sorted({r["pos"] for r in recs}) == list(range(-1, 64))
    for c, f in ri.GRID_SHAPES:
        mine = [r for r in recs if r["cigar"] == c and r["flag"] == f]
        assert [r["pos"] for r in mine] == ri.GRID_POSITIONS and all(rm.span(r) == ri.GRID_SPAN[c] for r in mine)
    assert sum(1 for x in ri.NINE_OPS if not x.isdigit()) == 9
    by = {(r["cigar"], r["flag"], r["pos"]): r for r in recs}
    assert len(by) == len(recs)
    for k, want in ri.GRID_EXPECT.items():
        assert rm.overlaps(by[k], s["regions"]) == want, k
    # every shape is looked at on both sides of a boundary
    for c, f in ri.GRID_SHAPES:
        assert {v for k, v in ri.GRID_EXPECT.items() if k[:2] == (c, f)} == {True, False}
    # pos == -1 overlaps nothing whatever the shape, and a flag-4 read at a position is judged like any one-base record
    assert not any(rm.overlaps(r, [(1, 0, 64)]) for r in recs if r["pos"] == -1)
    assert [rm.overlaps(by[("*", 4, p)], s["regions"]) for p in range(64)] == [rm.overlaps(by[("*", 0, p)], s["regions"]) for p in range(64)]
    kept = rm.keep(recs, s["regions"])
    assert 0 < len(kept) < len(recs)


def test_change_lists_differ():
    s = ri.BY_NAME["changes_on_dropped"]
    c = s["claim"]
    assert rm.changes(s["records"])[0] == c["changes_in"]
    out = [s["records"][i] for i in rm.keep(s["records"], s["regions"])]
    assert rm.changes(out)[0] == c["changes_out"] != c["changes_in"]
    out_x = [s["records"][i] for i in rm.keep(s["records"], s["regions"], True)]
    assert rm.changes(out_x)[0] == c["changes_out_x"]
    assert any(r["flag"] & 12 for r in out)                  # a kept record that takes no part in the list


def test_contigs_without_regions_and_the_last_contig():
    s = ri.BY_NAME["contig_order"]
    with_regions = {x[0] for x in s["regions"]}
    assert set(s["claim"]["without_regions"]) == set(range(len(s["lens"]))) - with_regions
    assert s["claim"]["last_contig"] == len(s["lens"]) - 1 in with_regions
    tids = [r["tid"] for r in s["records"]]
    assert tids == sorted(tids) and set(tids) == set(range(4))
    assert min(with_regions) > min(s["claim"]["without_regions"]) and max(s["claim"]["without_regions"]) > min(with_regions)
    assert rm.normalise(s["regions"], s["lens"])[-1] == (3, 990, 1000)          # clipped


def test_region_counts_and_the_list_that_does_not_fit():
    s = ri.BY_NAME["region_counts"]
    norm = rm.normalise(s["regions"], s["lens"])
    per = [sum(1 for x in norm if x[0] == t) for t in range(4)]
    assert per == s["claim"]["per_contig"] and per[3] == ri.MANY == 10000 > ri.LDS_CAPACITY
    many = [x for x in norm if x[0] == 3]
    assert all(x[2] - x[1] == 1 for x in many) and all(b[1] - a[1] == 2 for a, b in zip(many, many[1:]))
    recs = [r for r in s["records"] if r["tid"] == 3]
    assert len(recs) > 2 * ri.TILE                          # whole tiles stay on the contig with the long list
    on = [r for r in recs if r["cigar"] == "1M" and (r["pos"] - ri.MANY_AT) % 2 == 0 and 0 <= r["pos"] - ri.MANY_AT < 2 * ri.MANY]
    between = [r for r in recs if r["cigar"] == "1M" and (r["pos"] - ri.MANY_AT) % 2 == 1 and 0 <= r["pos"] - ri.MANY_AT < 2 * ri.MANY - 1]
    straddling = [r for r in recs if r["cigar"] == "2M" and (r["pos"] - ri.MANY_AT) % 2 == 1 and 0 <= r["pos"] - ri.MANY_AT < 2 * ri.MANY - 1]
    assert on and between and straddling
    assert all(rm.overlaps(r, s["regions"]) for r in on + straddling) and not any(rm.overlaps(r, s["regions"]) for r in between)
    # in front of the first and behind the last region
    assert not rm.overlaps(dict(tid=3, pos=ri.MANY_AT - 1, cigar="1M", flag=0), s["regions"]) and rm.overlaps(dict(tid=3, pos=ri.MANY_AT - 1, cigar="2M", flag=0), s["regions"])
    assert not rm.overlaps(dict(tid=3, pos=ri.MANY_AT + 2 * ri.MANY - 1, cigar="9M", flag=0), s["regions"])


def test_sizes_and_paths():
    assert len(ri.BY_NAME["blocks"]["records"]) == ri.BY_NAME["blocks"]["claim"]["n"] > 2 * ri.BLOCK_RECORDS
    b = ri.BY_NAME["blocks"]["records"]
    tiles = [b[k:k + ri.TILE] for k in range(0, len(b), ri.TILE)]
    assert sum(1 for t in tiles if len({r["tid"] for r in t}) > 1) == 1 and 5000 % ri.TILE != 0      # one tile holds the contig change, inside a workgroup's run of tiles
    kept = rm.keep(b, ri.BY_NAME["blocks"]["regions"])
    assert 0 < len(kept) < len(b) and len(kept) % ri.GATHER_GROUP != 0
    a = ri.BY_NAME["all_kept"]["records"]
    assert all(len({r["tid"] for r in a[k:k + ri.TILE]}) == 2 for k in range(0, len(a), ri.TILE))     # no tile of this set stays on one contig
    for name in ("n0_list", "n0_records", "one_kept", "one_dropped"):
        s = ri.BY_NAME[name]
        assert (len(s["regions"]), len(s["records"])) == {"n0_list": (0, 3), "n0_records": (1, 0), "one_kept": (1, 1), "one_dropped": (1, 1)}[name]
    u = ri.BY_NAME["unplaced"]["records"]
    assert sum(1 for r in u if r["tid"] < 0) == 3


def test_seq_repack():
    s = ri.BY_NAME["seq_repack"]
    recs = s["records"]
    clipped = [i for i, r in enumerate(recs) if r["cigar"][-1] == "S" or "S" in r["cigar"][:3]]
    assert len(clipped) == s["claim"]["clipped"]
    kept = set(rm.keep(recs, s["regions"]))
    # all four kinds on both sides: clipped kept, clipped dropped, unclipped kept, unclipped dropped
    assert {(i in clipped, i in kept) for i in range(len(recs))} == {(True, True), (True, False), (False, True), (False, False)}
    assert {len(recs[i]["seq"]) % 2 for i in clipped} == {0, 1} and any(len(r["seq"]) == 0 for r in recs)
    # a kept clipped record behind a dropped one: its bases move up in the output's array
    assert any(i in kept and i in clipped and any(j not in kept and j in clipped for j in range(i)) for i in range(len(recs)))


def test_normalise_against_brute_force():
    """random lists - unsorted, overlapping, abutting, past the contig's end - and records at every position: the normalised list keeps what the list as given keeps"""
    rng = random.Random(11)
    lens = [50, 30]
    for _ in range(200):
        regions = []
        for _k in range(rng.randrange(0, 7)):
            t = rng.randrange(2)
            a = rng.randrange(0, lens[t] + 5)
            regions.append((t, a, a + rng.randrange(1, 12)))
        norm = rm.normalise(regions, lens)
        assert all(a[0] < b[0] or a[2] < b[1] for a, b in zip(norm, norm[1:])) and all(x[1] < x[2] <= lens[x[0]] for x in norm)
        recs = [dict(tid=t, pos=p, cigar=c, flag=0) for t in (0, 1) for p in range(-1, lens[t]) for c in ("*", "3M", "2M5D1M")]
        recs = [r for r in recs if rm.interval(r)[1] <= lens[r["tid"]]]      # (a record ends inside its contig: only then does the clipping change nothing)
        assert rm.keep(recs, regions) == rm.keep(recs, norm)
    with pytest.raises(ValueError):
        rm.normalise([(0, 5, 5)], lens)
    with pytest.raises(ValueError):
        rm.normalise([(2, 0, 5)], lens)
    with pytest.raises(ValueError):
        rm.normalise([(0, -1, 5)], lens)
    assert rm.normalise([(0, 50, 60)], lens) == []           # left empty by the clipping


def test_the_cli_bed_keeps_between_a_third_and_two_thirds():
    import coordsort_inputs as ci
    import markdup_cli_inputs as CI
    import pairdup_cli_inputs as PI
    bed = ri.cli_bed(PI.LENS)
    assert bed != sorted(bed) and len(rm.normalise(bed, list(PI.LENS))) < len(bed)          # unsorted as given, and some regions overlap
    recs = PI.sample()[1]
    kept = rm.keep(recs, bed)
    in_kept = set(kept)
    assert len(recs) / 3 < len(kept) < 2 * len(recs) / 3
    names = {recs[i]["qname"] for i in kept}
    # junction A's clipped reads stay with -L, junction B's and the pile with -X
    assert {"A0", "A1"} <= names and not any(n.startswith("B") or n.startswith("pile") for n in names)
    # pairs with one unmapped end on both sides of the list
    half = [i for i, r in enumerate(recs) if r["qname"].startswith("half")]
    assert 0 < sum(1 for i in half if i in in_kept) < len(half)
    # -D's flags come from the whole sample: marked records stay whose mate - without which no rule finds the pair - lies outside every region
    by_name = {}
    for i, r in enumerate(recs):
        by_name.setdefault(r["qname"], []).append(i)
    marked = [i for i, r in enumerate(PI.flagged(recs)) if r["flag"] & 0x400]
    assert any(i in in_kept and any(j not in in_kept for j in by_name[recs[i]["qname"]]) for i in marked)
    # ... and so do -M's, on the sample whose copies lie at one place
    plain = ci.cli_sample()[1]
    kept_m = set(rm.keep(plain, bed))
    assert len(plain) / 3 < len(kept_m) < 2 * len(plain) / 3
    assert any(r["flag"] & 0x400 and i in kept_m for i, r in enumerate(CI.flagged(plain)))
