"""The split-read rule of `seeksv run -A` on the CPU: tests/splitread_model.py against the answers written out in tests/splitread_inputs.py, every set held to
the claim it was made for, and the agreement set - single-end, M I D S only, every record one-side soft-clipped or M..M - held to equality with
readthrough_model.find_junction, which tests/test_readthrough_model.py anchors on what the real reference printed."""
import numpy as np
import pytest

import readthrough_model as RM
import splitread_inputs as SI
import splitread_model as SM

SETS = SI.all_sets()


def run_model(records, min_mapq=1, cuts=()):
    b, names = SI.batch_of(records)
    batches, nm = RM.split(dict(batch=b, qnames=names), list(cuts))
    return SM.find_pairs(batches, nm, min_mapq, SI.CONTIGS)


@pytest.mark.parametrize("s", SETS, ids=[s["name"] for s in SETS])
def test_model_gives_the_written_answers(s):
    rows, counts = run_model(s["records"])
    assert len(rows) == len(s["rows"])
    for got, want in zip(rows, s["rows"]):
        assert got == want
    assert counts == s["counts"]
    # ... and the set as a file holds it
    records, want_rows = SI.file_set(s)
    rows, counts = run_model(records)
    assert rows == want_rows and counts == s.get("file_counts", s["counts"])
    # cut anywhere: the same
    for cut in range(1, len(s["records"])):
        assert run_model(s["records"], cuts=[cut]) == (s["rows"], s["counts"])


def test_combined_input_is_the_sets_side_by_side():
    records, rows, counts = SI.combined()
    got_rows, got_counts = run_model(records)
    assert got_rows == rows and got_counts == counts
    file_records, file_rows, file_counts = SI.combined(file_form=True)
    assert run_model(file_records) == (file_rows, file_counts) and not any(r.get("host_only") for r in file_records) and len(file_records) < len(records)
    assert len({r["qname"] for r in records}) == sum(len({r["qname"] for r in s["records"]}) for s in SETS)


def by_name(name):
    return next(s for s in SETS if s["name"] == name)


def test_worked_cases_are_the_issue_s():
    s = by_name("worked")
    r = s["rows"]
    assert r[0]["key"] == ("chrB", 1059, "+", "chrB", 5000, "+") and r[0]["kind"] == 0 and r[0]["microhomology"] == 0
    assert r[0]["up_seq"] == s["records"][0]["seq"][:60] and r[0]["down_seq"] == s["records"][0]["seq"][60:]          # bases 0..59 and 60..99 of the PRIMARY
    assert r[0]["up_cigar"] == [60 << 4] and r[0]["down_cigar"] == [40 << 4] and r[0]["edits"] == (1, 0)
    assert r[1]["microhomology"] == 2 and r[1]["key"][1] == 1059 and r[1]["up_cigar"] == [62 << 4]
    up, _ = RM.seq_infos(r[1])
    assert up["cigar"] == [(60, "M")]                                                                                   # 60M after the edit
    assert r[2]["key"] == ("chrB", 1059, "+", "chrB", 5039, "-") and r[2]["kind"] == 4 and r[2]["microhomology"] == 0
    assert r[2]["up_seq"] == s["records"][4]["seq"][:60] and r[2]["down_seq"] == s["records"][4]["seq"][60:]          # the primary's bases as stored


def test_each_set_makes_its_point():
    hard, soft = by_name("kinds_hard"), by_name("kinds_soft")
    assert [r["kind"] for r in hard["rows"]] == [0, 1, 2, 3, 4, 5] and hard["rows"] == soft["rows"]                    # borrowed or not: the same rows
    assert sum("H" in r["cigar"] for r in hard["records"]) == 6 and not any("H" in r["cigar"] for r in soft["records"])
    assert {(r["flag"] & 16) != 0 for r in hard["records"]} == {True, False}
    mh = by_name("microhomology")
    assert sorted((r["kind"], r["microhomology"]) for r in mh["rows"]) == [(0, 1), (0, 25), (1, 0), (2, 1), (2, 25), (3, 0), (4, 1), (4, 25), (5, 0)]
    assert [sum(r["clipped"]) for r in mh["rows"] if r["kind"] in (1, 3, 5)] == [1, 1, 1]                              # the < branches, missed by one
    bh = by_name("both_hard")
    assert all("H" in r["cigar"] for r in bh["records"][:2]) and bh["rows"][0]["records"] == (0, 2) and bh["counts"]["dropped_no_carrier"] == 1
    ul = by_name("unequal_lengths")
    assert ul["rows"] == [] and ul["counts"]["dropped_length"] == 1
    # the mate bits matter: the name alone pairs read 1 with read 2
    m = by_name("mates")
    b, names = SI.batch_of(m["records"])
    blind, _ = SM.find_pairs_by_name_only([b], [names], 1, SI.CONTIGS)
    assert [r["records"] for r in blind] == m["by_name_only"] and [r["records"] for r in m["rows"]] != m["by_name_only"]
    assert len({r["qname"] for r in m["records"]}) == 1 and {r["flag"] & 0xC0 for r in m["records"]} == {0x40, 0x80}
    assert sorted(len(r["qname"]) for r in by_name("name_lengths")["records"]) == [1, 1, 254, 254, 254]
    nt = by_name("not_taken")
    assert nt["rows"] == [] and nt["counts"]["candidates"] * 2 == len(nt["records"])
    assert {r["cigar"] for r in nt["records"]} >= {"", "50S40M10S", "50H40M10S", "100M", "10I90M", "100="}
    # ... each of them would pair if it were an ordinary supplementary record
    for k in range(1, len(nt["records"]), 2):
        good = dict(nt["records"][k], flag=SI.SUPP, mapq=60, tid=0, cigar="60S40M", seq=SI.S)
        assert run_model([nt["records"][k - 1], good])[1]["pairs"] == 1
    cr = by_name("clip_run")
    assert cr["records"][1]["cigar"] == "5H10S85M" and cr["rows"][0]["microhomology"] == 85 - 15
    rl = by_name("read_lengths")
    lens = sorted({len(r["up_seq"]) + len(r["down_seq"]) for r in rl["rows"]})
    assert lens == [1, 2, 63, 64, 65, 77, 129]
    assert all(len(r["down_seq"]) % 2 == 1 for r in rl["rows"] if r["kind"] == 2)                                       # the up record's clip is odd: its seqs start at odd offsets
    assert [r["kind"] for r in by_name("five")["rows"]] == [0, 2] and len(by_name("five")["records"]) == 5
    nb = by_name("no_bases")
    assert nb["counts"]["hard_clipped"] == 0 and nb["counts"]["pairs_borrowed"] == 2 and nb["counts"]["dropped_no_carrier"] == 1
    tc = by_name("two_contigs")["rows"][0]
    assert tc["key"][0] == "chrA" and tc["key"][3] == "chrB" and SI.CONTIGS.index("chrA") > SI.CONTIGS.index("chrB")


def fnv(name, mate):
    h = 1469598103934665603
    for ch in name.encode() + bytes([mate]):
        h = ((h ^ ch) * 1099511628211) & ((1 << 64) - 1)
    return h


def test_colliding_set_collides_under_four_bits():
    s = by_name("colliding")
    keys = {(r["qname"], r["flag"] & 0xC0) for r in s["records"]}
    buckets = {}
    for name, mate in keys:
        buckets.setdefault(fnv(name, mate) & 15, []).append(name)
    assert len(keys) == SI.N_COLLIDING and max(len(v) for v in buckets.values()) >= 3
    assert len({fnv(*k) for k in keys}) == len(keys)                                                                    # ... and not under 64


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("min_mapq", [0, 1, 31])
def test_agreement_set_equals_find_junction(seed, min_mapq):
    """where both rules apply they say the same: pairs, seqs, CIGAR sources"""
    s = SI.agreement(seed)
    for r in s["records"]:
        ops = RM.parse_cigar_text(r["cigar"])
        assert set(op for _, op in ops) <= set("MIDS") and not r["flag"] & (0x100 | 0xC0 | 1)
        assert (ops[0][1] == "S") != (ops[-1][1] == "S") or (ops[0][1] == "M" and ops[-1][1] == "M")
    b, names = SI.batch_of(s["records"] + SI.filler(20, seed))
    want, n_cand = RM.find_junction([b], [names], min_mapq, SI.CONTIGS)
    got, counts = SM.find_pairs([b], [names], min_mapq, SI.CONTIGS)
    assert got == want and counts["candidates"] == n_cand and counts["pairs"] == len(want)
    assert counts["hard_clipped"] == counts["pairs_borrowed"] == counts["dropped_no_carrier"] == counts["dropped_length"] == 0
    if min_mapq <= 1:
        assert len(want) >= 10 and {p["kind"] for p in want} == {0, 1, 2, 3, 4, 5}
    srt = SI.coordinate_sorted(s["records"] + SI.filler(20, seed))                                                     # ... and in coordinate order
    b, names = SI.batch_of(srt)
    assert SM.find_pairs([b], [names], min_mapq, SI.CONTIGS)[0] == RM.find_junction([b], [names], min_mapq, SI.CONTIGS)[0]


def test_cli_sample_is_what_it_claims():
    recs = SI.coordinate_sorted(SI.cli_sample())
    b, names = SI.batch_of(recs)
    rows, counts = SM.find_pairs([b], [names], 1, SI.CONTIGS)
    n_split = SI.N_FRAGMENTS + len([k for k in range(SI.N_FRAGMENTS) if k % 4 == 1])
    assert counts == dict(candidates=2 * n_split, hard_clipped=n_split, pairs=n_split, pairs_borrowed=n_split, dropped_no_carrier=0, dropped_length=0)
    assert {r["kind"] for r in rows} == {0, 1, 2, 3, 4, 5}
    for r in rows:                                                   # none across mates
        a, c = recs[r["records"][0]], recs[r["records"][1]]
        assert a["qname"] == c["qname"] and a["flag"] & 0xC0 == c["flag"] & 0xC0
    blind, _ = SM.find_pairs_by_name_only([b], [names], 1, SI.CONTIGS)
    assert sorted(r["records"] for r in blind) != sorted(r["records"] for r in rows)
    keys = [r["key"] for r in rows]                                   # every junction alone in its neighbourhood
    assert len(set(keys)) == len(keys)
    for x in keys:
        assert not [y for y in keys if y != x and (y[0], y[2], y[3], y[5]) == (x[0], x[2], x[3], x[5]) and abs(y[1] - x[1]) <= 50 and abs(y[4] - x[4]) <= 50]
    sh, _ = SI.batch_of(SI.shuffled(recs))
    assert SM.find_pairs([sh], [[r["qname"] for r in SI.shuffled(recs)]], 1, SI.CONTIGS)[1] == counts
