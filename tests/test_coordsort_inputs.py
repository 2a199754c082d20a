"""The hand-made sets of tests/coordsort_inputs.py are what they claim to be, and tests/coordsort_model.py sorts them as Python's own stable sort does."""
import collections

import pytest

import bamio
import coordsort_inputs as ci
import coordsort_model as cm
import markdup_cli_inputs as CI

IDS = [s["name"] for s in ci.SETS]


def keys(s):
    return [cm.key(r, s["n_targets"]) for r in s["records"]]


@pytest.mark.parametrize("s", ci.SETS, ids=IDS)
def test_model_is_pythons_stable_sort(s):
    recs, nt = s["records"], s["n_targets"]
    got = cm.order(recs, nt)
    assert got == sorted(range(len(recs)), key=lambda i: cm.key(recs[i], nt))
    out = [recs[i] for i in got]
    assert cm.is_sorted(out, nt) and sorted(got) == list(range(len(recs)))
    assert cm.is_sorted(recs, nt) == (got == list(range(len(recs))))


@pytest.mark.parametrize("s", ci.SETS, ids=IDS)
def test_records_are_told_apart_and_fit_their_header(s):
    assert [r["isize"] for r in s["records"]] == list(range(len(s["records"])))
    assert all(-1 <= r["tid"] < s["n_targets"] and -1 <= r["pos"] <= ci.MAX_LEN - 1 for r in s["records"])
    names, lens = ci.targets_of(s)
    assert len(names) == len(lens) == s["n_targets"]
    for r in s["records"]:      # CIGAR and bases agree (both decoders check it)
        ops = bamio.parse_cigar(r["cigar"]) if r["cigar"] != "*" else []
        if ops and r["seq"]:
            assert sum(l for l, op in ops if op in (0, 1, 4, 7, 8)) == len(r["seq"])


def test_counts():
    for n in (0, 1, 2, 63, 64, 65, 2047, 2048, 2049):
        s = ci.BY_NAME[f"n{n}"]
        assert len(s["records"]) == s["claim"]["n"] == n
        if n >= 63:         # ties and disorder both
            assert len(set(keys(s))) < n and not cm.is_sorted(s["records"], 3)
    assert not cm.is_sorted(ci.BY_NAME["n2"]["records"], 3)
    for name in ("all_equal", "deep_tie"):
        s = ci.BY_NAME[name]
        assert len(s["records"]) == s["claim"]["n"] and len(set(keys(s))) == s["claim"]["distinct_keys"] == 1
    assert len(ci.BY_NAME["deep_tie"]["records"]) == 10 ** 5


def test_keys():
    s = ci.BY_NAME["pos_extremes"]
    assert {r["pos"] for r in s["records"]} >= set(s["claim"]["positions"]) == {-1, 2 ** 31 - 2}
    out = [s["records"][i] for i in cm.order(s["records"], 3)]
    assert [(r["tid"], r["pos"]) for r in out] == [(0, -1), (0, 2 ** 31 - 2), (1, -1), (1, -1), (1, 0), (1, 5), (1, 2 ** 31 - 2), (1, 2 ** 31 - 2)]
    assert [r["isize"] for r in out if (r["tid"], r["pos"]) == (1, -1)] == [2, 7]
    s = ci.BY_NAME["tid_bytes"]
    assert s["n_targets"] == 70000 and {r["tid"] for r in s["records"]} == set(s["claim"]["tids"]) == {0, 255, 256, 65535, 65536, 69999, -1}
    out = [s["records"][i]["tid"] for i in cm.order(s["records"], s["n_targets"])]
    assert out == [t for t in (0, 255, 256, 65535, 65536, 69999, -1) for _ in range(3)]        # the unplaced rank, 70000, behind every contig
    ranks = [cm.key(r, 70000)[0] for r in s["records"]]
    assert all(len({(t >> (8 * b)) & 255 for t in ranks}) > 1 for b in range(3))                 # every key byte of the rank differs somewhere
    s = ci.BY_NAME["one_target"]
    assert s["n_targets"] == 1 and {r["tid"] for r in s["records"]} == {0, -1}
    with pytest.raises(ValueError):
        cm.key(dict(tid=1, pos=0), 1)


def test_batches_and_ties():
    s = ci.BY_NAME["three_batches"]
    b = ci.batches_of(s, 1)
    assert len(b) == 3 and all(cm.is_sorted(x, 3) for x in b) and not cm.is_sorted(s["records"], 3)
    where = collections.defaultdict(set)
    for k, x in enumerate(b):
        for r in x:
            where[(r["tid"], r["pos"])].add(k)
    assert {k: len(v) for k, v in where.items() if len(v) > 1} == s["claim"]["ties_across"]
    out = [s["records"][i] for i in cm.order(s["records"], 3)]
    assert [r["isize"] for r in out if (r["tid"], r["pos"]) == (0, 100)] == [0, 3, 7]        # the earlier batch wins
    s = ci.BY_NAME["reversed"]
    k = keys(s)
    assert all(k[i] > k[i + 1] for i in range(len(k) - 1)) and len(k) > 128
    s = ci.BY_NAME["sorted"]
    assert cm.is_sorted(s["records"], 3) and len(set(keys(s))) < len(s["records"])
    s = ci.BY_NAME["sorted_but_last"]
    got, n = cm.order(s["records"], 3), len(s["records"])
    assert cm.is_sorted(s["records"][:-1], 3) and not cm.is_sorted(s["records"], 3)
    assert got.index(n - 1) < n - 100 and [i for i in got if i != n - 1] == list(range(n - 1))       # one record moves, far


def test_variable_parts():
    s = ci.BY_NAME["cigar_lengths"]
    n_ops = [0 if r["cigar"] == "*" else len(bamio.parse_cigar(r["cigar"])) for r in s["records"]]
    assert set(n_ops) >= set(s["claim"]["n_ops"]) == {0, 1, 5, 6, 70} and not cm.is_sorted(s["records"], 3)
    s = ci.BY_NAME["read_lengths"]
    assert {len(r["seq"]) for r in s["records"]} == set(s["claim"]["l_qseq"]) == {0, 7, 8}
    clipped = [r for r in s["records"] if 4 in (bamio.parse_cigar(r["cigar"])[0][1], bamio.parse_cigar(r["cigar"])[-1][1])]
    assert len(clipped) == s["claim"]["clipped"] and 0 < len(clipped) < len(s["records"])       # a decoder that ships clipped reads' bases only gives a mix
    s = ci.BY_NAME["unmapped_ends"]
    out = [s["records"][i] for i in cm.order(s["records"], 3)]
    assert sum(1 for r in out if r["flag"] & 12) == s["claim"]["skipped"]
    assert any(r["flag"] & 12 and r["tid"] == 1 for r in out)
    got, last = cm.changes(out)
    assert got == s["claim"]["changes"] and last == 2
    unfiltered, _ = cm.changes([dict(r, flag=0) for r in out])
    assert unfiltered != got                                                                     # the flag filter decides
    # across batches: the list goes on from the batch before, indices count inside the batch
    assert cm.batch_changes([out[:7], out[7:]]) == [[(6, 1)], [(0, 2)]]
    assert cm.batch_changes([out[:3], out[3:]]) == [[], [(3, 1), (4, 2)]]


def test_cut():
    assert cm.cut(0, 5) == [] and cm.cut(5, 5) == [(0, 5)] and cm.cut(6, 5) == [(0, 5), (5, 1)] and cm.cut(3, 1) == [(0, 1), (1, 1), (2, 1)]


def test_cli_sample():
    contigs, recs = ci.cli_sample()
    base = CI.sample()[1]
    assert len(recs) == len(base) + 2 * ci.N_HALF_MAPPED and ci.N_HALF_MAPPED >= 24
    half = [r for r in recs if r["flag"] & 12]
    assert len(half) == 2 * ci.N_HALF_MAPPED and sum(1 for r in half if r["flag"] & 4) == sum(1 for r in half if r["flag"] & 8) == ci.N_HALF_MAPPED
    assert not any(r["flag"] & 12 for r in base)
    names, nt = collections.Counter(r["qname"] for r in half), len(CI.NAMES)
    assert set(names.values()) == {2}
    assert cm.is_sorted(recs, nt)
    pile = max(collections.Counter(cm.key(r, nt) for r in recs).values())
    assert pile >= CI.PILE == 11000
    for other in (ci.shuffled(recs), ci.by_name(recs)):
        assert not cm.is_sorted(other, nt) and sorted(id(r) for r in other) == sorted(id(r) for r in recs)
        # ties: the expected file of an order is the stable sort OF THAT ORDER, and the orders disagree about it
        assert [id(other[i]) for i in cm.order(other, nt)] != [id(r) for r in recs]
    assert ci.by_name(recs) != ci.shuffled(recs)
