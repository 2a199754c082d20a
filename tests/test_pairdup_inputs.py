"""The hand-made sets of tests/pairdup_inputs.py against the plain model of `seeksv run -D`'s rule (tests/pairdup_model.py): the model gives the answers written
by hand, every set has the property it is named for, and the sets without score ties are marked the same way in every order.  No GPU."""
import pytest

import markdup_model as mm
import pairdup_inputs as pi
import pairdup_model as pm

IDS = [s["name"] for s in pi.SETS]


def marked(records, flags):
    return [i for i, (r, f) in enumerate(zip(records, flags)) if f != r["flag"]]


def key_of(s, name):
    a, b = [r for r in s["records"] if r["qname"] == name]
    return pm.pair_key(a, b)


@pytest.mark.parametrize("s", pi.SETS, ids=IDS)
def test_the_model_gives_the_written_answers(s):
    recs = s["records"]
    flags = pm.mark(recs)
    assert marked(recs, flags) == s["dup"]
    assert all(f == r["flag"] | 0x400 for i, (r, f) in enumerate(zip(recs, flags)) if i in s["dup"])
    assert mm.sorted_ok(recs)                                     # `records` is the coordinate order
    assert all(0 <= r["tid"] < len(s["targets"]) or r["tid"] == -1 for r in recs)


@pytest.mark.parametrize("s", pi.SETS, ids=IDS)
def test_the_four_orders(s):
    orders = pi.orders(s)
    assert [o[0] for o in orders] == ["coordinate", "read_name", "reversed", "shuffle"]
    assert orders[0][1] == s["records"]
    for name, recs, where in orders:
        assert sorted(where) == list(range(len(recs)))
        got = {where[i] for i in marked(recs, pm.mark(recs))}
        if not pm.score_ties(s["records"]):
            assert got == set(s["dup"]), name                     # without score ties the marked set does not depend on the order
    if len(s["records"]) > 2:
        assert len({tuple(o[2]) for o in orders}) >= 3            # the orders really differ
    assert pm.score_ties(s["records"]) == bool(s["claim"].get("ties"))


def test_equal_scores_keep_the_earliest_in_every_order():
    s = pi.BY_NAME["equal_scores"]
    for name, recs, where in pi.orders(s):
        assert all(pm.takes_part(r) for r in recs)
        keeper = recs[0]["qname"]                                  # every pair scores the same: the pair of the record that comes first stays
        got = marked(recs, pm.mark(recs))
        assert sorted(got) == [i for i, r in enumerate(recs) if r["qname"] != keeper], name


def test_clip_forms_are_what_the_aligned_rule_misses():
    s = pi.BY_NAME["clip_forms"]
    recs = s["records"]
    assert [r["cigar"] for r in recs if r["flag"] & 0x40] == ["20M", "5S15M"] and [r["pos"] for r in recs if r["flag"] & 0x40] == [100, 105]
    assert marked(recs, mm.mark(recs)) == []                      # -M's rule: aligned positions differ
    assert key_of(s, "k") == key_of(s, "d") == (0, 100, 0, 0, 319, 1)
    for t in ("cigar7", "u_negative"):                             # (leading clips move pos; reverse_ends' trailing clips do not, -M finds those)
        r2 = pi.BY_NAME[t]["records"]
        assert marked(r2, mm.mark(r2)) == []


def test_reverse_ends():
    s = pi.BY_NAME["reverse_ends"]
    rev = [r for r in s["records"] if r["flag"] & 0x10]
    assert [r["cigar"] for r in rev] == ["20M"] + s["claim"]["cigars"] and {r["pos"] for r in rev} == {300}
    assert {pm.end_u(r) for r in rev} == {319}
    assert any(r["cigar"].endswith("S3H") for r in rev) and any("D" in r["cigar"] for r in rev) and any("N" in r["cigar"] for r in rev) and any("I" in r["cigar"] for r in rev)
    assert len({pm.read_score(a) + pm.read_score(b) for a, b in zip(s["records"][:6], s["records"][6:])}) == 6


def test_cigar7_and_negative_u():
    s = pi.BY_NAME["cigar7"]
    d = [r for r in s["records"] if r["qname"] == "d"]
    assert all(len(pm.cigar_ops(r)) == 7 for r in d) and (pm.end_u(d[0]), pm.end_u(d[1])) == s["claim"]["u"] == (100, 319)
    # the part of each CIGAR beyond five operations matters: cut to five the ends differ
    assert d[1]["cigar"] == "4M1D5M1I5M3S2H" and 300 + 4 + 1 + 5 + 5 - 1 != 319
    s = pi.BY_NAME["u_negative"]
    assert {pm.end_u(r) for r in s["records"] if not r["flag"] & 0x10} == {-3}


@pytest.mark.parametrize("field,at", [(v[0], v[1]) for v in pi._VARIANTS])
def test_key_sets_differ_in_one_field(field, at):
    s = pi.BY_NAME[f"key_{field}"]
    base, copy, var = key_of(s, "base"), key_of(s, "copy"), key_of(s, "var")
    assert base == copy == (1, 100, 0, 2, 319, 1)
    assert [k for k in range(6) if base[k] != var[k]] == [at] == [s["claim"]["differs_in"]]


def test_scores_and_name_groups():
    s = pi.BY_NAME["sum_not_read1"]
    x, y = ([r for r in s["records"] if r["qname"] == n] for n in "xy")
    assert (pm.read_score(x[0]), pm.read_score(y[0])) == s["claim"]["read1"] and x[0]["flag"] & 0x40 and y[0]["flag"] & 0x40
    assert (sum(map(pm.read_score, x)), sum(map(pm.read_score, y))) == s["claim"]["sums"]
    s = pi.BY_NAME["preset_0x400"]
    assert [i for i, r in enumerate(s["records"]) if r["flag"] & 0x400] == s["claim"]["preset"]
    found, unpaired = pm.pairs(s["records"])
    assert unpaired == s["claim"]["alone"] and len(found) == 2
    for name in ("group_of_one", "group_of_three", "two_first_of_pair", "mate_fields_disagree"):
        s = pi.BY_NAME[name]
        st = {}
        pm.mark(s["records"], stats=st)
        assert st["unpaired"] == s["claim"]["unpaired"] and st["pairs"] == (st["taking_part"] - st["unpaired"]) // 2, name
    s = pi.BY_NAME["two_first_of_pair"]
    assert sum(bool(r["flag"] & 0x40) for r in s["records"] if r["qname"] == "f") == 2
    s = pi.BY_NAME["group_of_three"]
    assert sum(r["qname"] == "t" for r in s["records"]) == 3
    # ... each of these would be marked if its name group were a pair: its key is k's and its score is lower
    for name, who in (("group_of_three", "t"), ("two_first_of_pair", "f"), ("mate_fields_disagree", "m"), ("mate_fields_disagree", "s")):
        s = pi.BY_NAME[name]
        a, b = [r for r in s["records"] if r["qname"] == who][:2]
        assert pm.pair_key(a, b) == key_of(s, "k") and pm.read_score(a) + pm.read_score(b) < 1200


def test_contigs_and_records_that_take_no_part():
    s = pi.BY_NAME["two_contigs"]
    assert key_of(s, "k")[0::3] == s["claim"]["contigs"]
    s = pi.BY_NAME["contig_ids"]
    assert max(r["tid"] for r in s["records"]) == s["claim"]["max_tid"] == 69999 and len(s["targets"]) == 70000
    assert key_of(s, "v")[0] == key_of(s, "k")[0] & 0xffff and key_of(s, "v")[1:] == key_of(s, "k")[1:]
    s = pi.BY_NAME["unmapped_between"]
    assert sum(not pm.takes_part(r) for r in s["records"]) == s["claim"]["no_part"]
    for name, recs, where in pi.orders(s)[1:]:
        part = [i for i, r in enumerate(recs) if pm.takes_part(r)]
        assert any(not pm.takes_part(recs[i]) for i in range(part[0], part[-1])), name     # in between


@pytest.mark.parametrize("n", [2, 63, 64, 65, 130])
def test_groups_of_one_key(n):
    s = pi.BY_NAME[f"group_{n}"]
    recs = s["records"]
    st = {}
    pm.mark(recs, stats=st)
    assert st == dict(records=2 * n, taking_part=2 * n, unpaired=0, pairs=n, groups_many=1, pairs_marked=n - 1)
    scores = [pm.read_score(recs[k]) + pm.read_score(recs[n + k]) for k in range(n)]
    assert sorted(scores) == list(range(1200, 1200 + n)) and scores[s["claim"]["best"]] == 1200 + n - 1
    assert 0 < s["claim"]["best"] < n - 1 or n == 2


@pytest.mark.parametrize("bits", [4, 1])
def test_300_distinct_keys_collide_under_narrow_hashes(bits):
    s = pi.BY_NAME["collide_300"]
    recs = s["records"]
    found, _ = pm.pairs(recs)
    assert len(found) == 300 and len({pm.pair_key(recs[a], recs[b]) for a, b in found}) == 300
    assert len({pm.name_hash(r) for r in recs}) == 300
    st = {}
    assert pm.mark(recs, bits, st) == [r["flag"] for r in recs]
    assert len({pm.name_hash(r, bits) for r in recs}) == 1 << bits and st["pairs"] == 0 and st["unpaired"] == 600


def test_rows_of_records_that_take_no_part_are_zero():
    s = pi.BY_NAME["unmapped_between"]
    assert [pm.row(r) == (0, 0, 0, 0) for r in s["records"]] == [not pm.takes_part(r) for r in s["records"]]
    r = pi.BY_NAME["clip_forms"]["records"][1]
    assert pm.row(r) == (mm.fnv1a(b"d"), 100, 400, 1)
