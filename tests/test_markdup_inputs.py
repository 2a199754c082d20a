"""Every hand-made input set of tests/markdup_inputs.py is what it claims to be (the claims are about the inputs, not about the rule's answers)."""
import pytest

import markdup_inputs as mi
import markdup_model as mm

IDS = [s["name"] for s in mi.SETS]


@pytest.mark.parametrize("s", mi.SETS, ids=IDS)
def test_sets_are_sorted_and_well_formed(s):
    recs = s["records"]
    assert mm.sorted_ok(recs)
    assert all(r["tid"] >= 0 for r in recs[:next((i for i, r in enumerate(recs) if r["tid"] < 0), len(recs))])  # unplaced records come last
    assert all(0 <= i < len(recs) for i in s["dup"]) and s["dup"] == sorted(set(s["dup"]))
    assert all(1 <= len(r["qname"]) <= 254 for r in recs)
    assert all(r["qual"] is None or len(r["qual"]) == len(r["seq"]) for r in recs)


def heads_of_run(recs, first):
    s, e = next((s, e) for s, e in mm.runs(recs) if s == first)
    return [i for i in range(s, e) if mm.takes_part(recs[i]) and mm.is_head(recs[i])], e - s


@pytest.mark.parametrize("name, field", [("key_mtid", "mtid"), ("key_mpos", "mpos"), ("key_rev", 0x10), ("key_mrev", 0x20)])
def test_key_sets_differ_in_exactly_one_field(name, field):
    s = mi.BY_NAME[name]
    heads, _ = heads_of_run(s["records"], 0)
    assert len(heads) == s["claim"]["heads_at_first_run"] == 3
    base, var, copy = (s["records"][i] for i in heads)
    assert mm.group_key(base) == mm.group_key(copy)
    kb, kv = mm.group_key(base), mm.group_key(var)
    differing = [k for k in range(6) if kb[k] != kv[k]]
    assert differing == [{"mtid": 2, "mpos": 3, 0x10: 4, 0x20: 5}[field]]


def test_tie_set_has_both_reads_at_one_position():
    s = mi.BY_NAME["tie_0x40"]
    assert all((r["tid"], r["pos"]) == (r["mtid"], r["mpos"]) for r in s["records"])
    assert [i for i, r in enumerate(s["records"]) if mm.is_head(r)] == s["claim"]["heads"] and [i for i, r in enumerate(s["records"]) if r["flag"] & 0x40] == s["claim"]["heads"]


@pytest.mark.parametrize("name", ["score_tie_earlier", "score_14_15", "score_ff", "score_lq0"])
def test_score_sets(name):
    s = mi.BY_NAME[name]
    heads, _ = heads_of_run(s["records"], 0)
    assert [mm.score(s["records"][i]) for i in heads] == s["claim"]["scores"]
    assert len({mm.group_key(s["records"][i]) for i in heads}) == 1
    if name == "score_14_15":
        assert set(mm.quals(s["records"][0])) == {14} and 15 in mm.quals(s["records"][1])
    if name == "score_ff":
        assert mm.quals(s["records"][0])[0] == 0xff
    if name == "score_lq0":
        assert s["records"][0]["seq"] == "" and mm.quals(s["records"][1])[0] == 0xff


def test_no_part_set():
    s = mi.BY_NAME["no_part"]
    recs = s["records"]
    assert [i for i, r in enumerate(recs) if not mm.takes_part(r)] == s["claim"]["no_part"]
    for bit in (0x4, 0x8, 0x100, 0x800, 0x400):
        assert any(r["flag"] & bit and r["tid"] == 0 for r in recs)
    assert [i for i, r in enumerate(recs) if r["flag"] & 0x400] == s["claim"]["preset"]
    assert recs[-1]["tid"] == -1 and recs[-1]["flag"] & 1 and not recs[-1]["flag"] & 0xc   # paired, nothing unmapped, yet unplaced
    # each of them would win its group if it took part: a higher score than the keeper's
    assert all(mm.score(recs[i]) > mm.score(recs[7]) for i in range(7))


def test_tail_sets():
    s = mi.BY_NAME["tail_before_head"]
    recs = s["records"]
    assert len(mm.runs(recs)) == 1 and [i for i, r in enumerate(recs) if mm.takes_part(r) and not mm.is_head(r)] == s["claim"]["tails"]
    assert recs[0]["qname"] == recs[2]["qname"] and not mm.is_head(recs[0]) and mm.is_head(recs[2])       # the tail lies before its head
    s = mi.BY_NAME["tail_kept_and_stray"]
    recs = s["records"]
    places = {(r["tid"], r["pos"]) for r in recs}
    assert all((recs[i]["mtid"], recs[i]["mpos"]) not in places for i in s["claim"]["stray"])


def test_name_sets():
    s = mi.BY_NAME["equal_names"]
    same = [r for r in s["records"] if r["qname"] == s["claim"]["shared_name"]]
    assert len(same) == 4 and len({mm.digest(r) for r in same}) == 2
    s = mi.BY_NAME["name_lengths"]
    assert sorted({len(r["qname"]) for r in s["records"]}) == s["claim"]["lengths"]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 1000])
def test_runs_of_n_heads(n):
    for kind, groups in (("one_key", 1), ("distinct", n)):
        s = mi.BY_NAME[f"run_{n}_{kind}"]
        heads, length = heads_of_run(s["records"], 0)
        assert len(heads) == length == n == s["claim"]["heads"]
        assert len({mm.group_key(s["records"][i]) for i in heads}) == groups == s["claim"]["groups"]
    s = mi.BY_NAME[f"run_{n}_one_key"]
    scores = [mm.score(r) for r in s["records"][:n]]
    assert scores.index(max(scores)) == s["claim"]["best"] and scores.count(max(scores)) == 1


def test_run_of_300_with_two_heads():
    s = mi.BY_NAME["run_300_two_heads"]
    heads, length = heads_of_run(s["records"], 0)
    assert length == s["claim"]["run"] == 300 and heads == s["claim"]["heads"]


def test_mixed_set_and_the_unsorted_one():
    s = mi.BY_NAME["mixed"]
    assert len({r["tid"] for r in s["records"] if r["tid"] >= 0}) == s["claim"]["contigs"]
    assert not mm.sorted_ok(mi.UNSORTED)


def test_sam_text_has_one_line_per_record():
    s = mi.BY_NAME["no_part"]
    lines = mi.sam_text(s["records"]).decode().splitlines()
    assert len(lines) == len(s["records"]) and all(len(x.split("\t")) == 11 for x in lines)
