"""The inputs of the device row builder and of `seeksv run -P` (tests/run_split_inputs.py), held to the properties they were built for with the models
alone - realign_split_model for the alignments, readthrough_model for the -F pass; no GPU, no library."""
import functools

import pytest

import realign_split_inputs as SI
import run_split_inputs as RI


@functools.lru_cache(maxsize=None)
def results(name):
    return RI.model_results(RI.SETS[name]())


def test_every_length_occurs_and_aligns_where_it_can():
    s = RI.length_set()
    assert sorted({len(e[1]) for e in s}) == sorted(RI.LENGTHS) and all(sum(len(e[1]) == n for e in s) == 3 for n in RI.LENGTHS)
    res = results("length")
    for (_, q, _), r in zip(s, res):
        assert (r["primary"]["tid"] >= 0) == (30 <= len(q) <= 1024), (len(q), r["primary"])   # (20 and 21 bases score below 30)
    rev = {len(q) for (_, q, _), r in zip(s, res) if r["primary"]["tid"] >= 0 and r["primary"]["reverse"]}
    fwd = {len(q) for (_, q, _), r in zip(s, res) if r["primary"]["tid"] >= 0 and not r["primary"]["reverse"]}
    assert {n for n in RI.LENGTHS if 30 <= n <= 1024 and n % 2} & rev and {n for n in RI.LENGTHS if 30 <= n <= 1024 and n % 2} & fwd   # odd lengths on both strands
    assert rev & {511, 512, 513, 1024} and {63, 64, 65} & rev
    assert any(r["mate"]["tid"] >= 0 for (_, q, _), r in zip(s, res) if len(q) == 1024)


@pytest.mark.parametrize("name", [k for k in RI.SETS if k != "empty"])
def test_no_set_holds_a_query_the_hash_index_leaves_open(name):
    """`overflow` and `tie` are not functions of the input on the hash index: none here, so no record is exempt on the GPU"""
    assert not any(r["overflow"] or r["tie"] for r in results(name))


def test_names_and_offsets():
    every = [e for fn in RI.SETS.values() for e in fn()]
    lens = {len(e[0].encode()) for e in every}
    assert 1 in lens and RI.LONG_NAME in lens and max(lens) == 254 and min(lens) == 1
    for name in ("length", "alphabet", "no_mate", "all_mate"):
        so, no = RI.offsets_mod8(RI.SETS[name]())
        assert no == set(range(8)), (name, no)
        if name in ("length", "alphabet", "no_mate"):
            assert so == set(range(8)), (name, so)
    assert len(RI.one_set()) == 1 and len(RI.empty_set()) == 0
    for fn in RI.SETS.values():
        assert all(len(q) == len(s) for _, s, q in fn())


def test_alphabet_set_has_other_letters_on_both_strands():
    s, res = RI.alphabet_set(), results("alphabet")
    assert any(ch in q for _, q, _ in s for ch in "Nn") and any(q != q.upper() for _, q, _ in s) and any(ch in q for _, q, _ in s for ch in "R.")
    odd = [(q, r) for (_, q, _), r in zip(s, res) if set(q) - set("ACGT")]
    assert any(r["primary"]["tid"] >= 0 and r["primary"]["reverse"] for q, r in odd) and any(r["mate"]["tid"] >= 0 and r["mate"]["reverse"] for q, r in odd)
    assert any(r["mate"]["tid"] >= 0 and not r["primary"]["reverse"] for q, r in odd)
    assert any(r["primary"]["tid"] < 0 for q, r in odd)


def test_strand_combinations_and_mate_sets():
    combos = {(r["primary"]["reverse"], r["mate"]["reverse"]) for r in results("strand") if r["mate"]["tid"] >= 0}
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(r["mate"]["tid"] < 0 for r in results("no_mate")) and any(r["primary"]["tid"] >= 0 for r in results("no_mate")) and any(r["primary"]["tid"] < 0 for r in results("no_mate"))
    assert all(r["mate"]["tid"] >= 0 for r in results("all_mate")) and len(results("all_mate")) >= 20
    assert results("one")[0]["mate"]["tid"] >= 0


def test_rows_of_a_set_pair_up_in_the_model():
    """the planted reads as -F rows: a pair per read with a mate (names are unique), none from the reads without"""
    s = RI.all_mate_set()
    rows = RI.model_rows(s, results("all_mate"))
    assert len(rows) == 2 * len(s) and [r["flag"] & 2048 for r in rows] == [0, 2048] * len(s)
    pairs, cand = RI.model_junctions(rows, SI.NAMES)
    assert cand > 0 and len(pairs) > len(s) // 2
    rows = RI.model_rows(RI.no_mate_set(), results("no_mate"))
    assert len(rows) == len(RI.no_mate_set()) and RI.model_junctions(rows, SI.NAMES)[0] == []


def _e2e_rows(contigs, entries):
    import realign_model as M
    ref = M.Reference(contigs)
    return RI.model_rows(entries, RI.model_results(entries, ref=ref))


def test_e2e_sample_in_cat_order():
    """prefix.unmapped_1.fq.gz then prefix.unmapped_2.fq.gz of e2e_sample(): the mapped mates of file 1 come back 100M and are dropped; the ten junction reads
    of file 2 give 20 candidates, 10 pairs and the one planted key"""
    contigs, recs = SI.e2e_sample()
    f1, f2 = RI.unmapped_fastq(recs)
    assert len(f1) == len(f2) == SI.E2E_READS and all(n.endswith("/1") for n, _, _ in f1) and all(n.endswith("/2") for n, _, _ in f2)
    rows = _e2e_rows(contigs, f1 + f2)
    assert all(r["cigar"] == [(100, 0)] for r in rows[:len(f1)]) and len(rows) == len(f1) + 2 * len(f2)
    pairs, cand = RI.model_junctions(rows, SI.E2E_NAMES)
    assert cand == 20 and len(pairs) == 10 and {p["key"] for p in pairs} == {RI.E2E_KEY}


def test_e2e_variant_has_junction_reads_in_both_files():
    contigs, recs = RI.e2e_variant()
    f1, f2 = RI.unmapped_fastq(recs)
    assert len(f1) == len(f2) == SI.E2E_READS
    for part, n in ((f1, SI.E2E_READS // 2), (f2, SI.E2E_READS - SI.E2E_READS // 2)):
        pairs, cand = RI.model_junctions(_e2e_rows(contigs, part), SI.E2E_NAMES)
        assert cand == 2 * n and len(pairs) == n and {p["key"] for p in pairs} == {RI.E2E_KEY}
    pairs, cand = RI.model_junctions(_e2e_rows(contigs, f1 + f2), SI.E2E_NAMES)
    assert cand == 20 and len(pairs) == 10 and {p["key"] for p in pairs} == {RI.E2E_KEY}
    assert [r["flag"] for r in recs if r["qname"] == "jn1"] == [137, 69] and [r["flag"] for r in recs if r["qname"] == "jn2"] == [73, 133]
