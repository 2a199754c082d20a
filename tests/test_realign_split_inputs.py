"""CPU: every query set of tests/realign_split_inputs.py holds the property it was built for, under the model alone (tests/realign_split_model.py).
The hash index's sets contain no `overflow` and no `tie` query: nothing is exempt in tests/test_realign_split_gpu.py."""
import functools

import pytest

import realign_model as M
import realign_sorted_model as SRT
import realign_split_inputs as SI
import realign_split_model as SM


@functools.lru_cache(maxsize=None)
def ref():
    return M.Reference(SI.reference())


@functools.lru_cache(maxsize=None)
def results(max_occ):
    return tuple(SM.align_split(ref(), s, max_occ) for s in SI.all_queries()[0])


def test_reference_is_small_and_named():
    assert len(SI.reference()) == len(SI.NAMES) and sum(len(c) for c in SI.reference()) < 12000
    assert SI.offsets()[-1] == len(ref().text)


def test_no_query_is_left_to_the_lanes():
    """hash index: no query with more seeds than slots, none tied between two contigs - in every set that runs on it"""
    assert not any(r["overflow"] or r["tie"] for r in results(None))
    for contigs, queries, _ in (SI.sweep_set(), SI.tandem_set()):
        rf = M.Reference(contigs)
        assert not any(r["overflow"] or r["tie"] for r in (SM.align_split(rf, s) for s in queries))


@pytest.mark.parametrize("max_occ", [None, SI.CAP], ids=["hash", "sorted"])
def test_lengths(max_occ):
    q, lab = SI.length_set()
    assert sorted({len(s) for s in q}) == [40, 64, 65, 250, 1024]
    res = {l: SM.align_split(ref(), s, max_occ) for s, l in zip(q, lab)}
    for l, r in res.items():
        assert r["primary"]["tid"] >= 0 and (r["mate"]["tid"] >= 0) == (not l.startswith("len40")), l
    assert (res["len1024/fwd"]["primary"]["q_end"], res["len1024/fwd"]["mate"]["q_end"]) == (1024, 1024)   # (both in their own orientation)


def test_sweep_puts_the_mate_in_the_winners_lane():
    contigs, queries, labels = SI.sweep_set()
    rf = M.Reference(contigs)
    fwd = {}
    for s, l in zip(queries, labels):
        plain = M.align(rf, s)
        r = SM.align_split(rf, s)
        assert r["mate"]["tid"] == 1 and r["mate"]["reverse"] == 1 and r["mate"]["score"] >= 50 and r["primary"]["tid"] == 0 and r["primary"]["mapq"] == r["mate"]["mapq"] == 60, l
        assert plain["n_seeds"] <= M.MAX_CAND and plain["n_candidates"] == 2, l   # every strand-0 seed on the winner's diagonal, every strand-1 seed on the mate's
        fwd[len(s) - 51] = plain["n_seeds_fwd"]
        for max_occ in (SI.CAP,):
            assert SRT.align_sorted(rf, s, max_occ)["flags"] == 0
    assert [n for n, k in fwd.items() if k == 64] == [272, 273, 274, 275] and [n for n, k in fwd.items() if k == 128] == [528, 529, 530, 531]
    assert min(fwd.values()) < 64 < max(k for n, k in fwd.items() if n < 300) and min(k for n, k in fwd.items() if n > 500) < 128 < max(fwd.values())


def test_tandem_has_more_diagonals_than_lanes():
    contigs, queries, labels = SI.tandem_set()
    rf = M.Reference(contigs)
    assert len(queries) >= 12
    most = 0
    for s, l in zip(queries, labels):
        plain = M.align(rf, s)
        r = SM.align_split(rf, s)
        most = max(most, plain["n_candidates"])
        assert plain["n_seeds"] <= M.MAX_CAND and plain["mapq"] < 60, l
        assert r["primary"]["tid"] == 1 and r["primary"]["mapq"] == 60 and r["mate"]["tid"] == 0 and r["mate"]["mapq"] <= 6 and r["mate"]["second"] >= 30, l   # (6: the copy at the array's edge, one base longer by chance)
    assert most > 64


def test_mix_takes_turns():
    q, lab = SI.mix_set()
    n0 = len(SI.all_queries()[0]) - len(q)
    res = results(None)[n0:]
    assert 1900 < len(q) < 2100 and len(q) % 4
    kinds = []
    for s, r in zip(q, res):
        kinds.append("short" if len(s) < M.MIN_Q else "long" if len(s) > M.MAX_Q else "unaligned" if r["primary"]["tid"] < 0 else "split" if r["mate"]["tid"] >= 0 else "unsplit")
    count = {k: kinds.count(k) for k in set(kinds)}
    assert count["split"] > 500 and count["unsplit"] > 400 and count["unaligned"] > 100 and count["short"] > 100 and count["long"] > 100, count
    # early returns beside live wavefronts: workgroups (four queries in a row) that hold a short or long query AND a split one
    assert sum(1 for i in range(0, len(q) - 3, 4) if {"short", "long"} & set(kinds[i:i + 4]) and "split" in kinds[i:i + 4]) > 100
    # and the sorted index has the same primaries and mates on this reference
    assert [(r["primary"], r["mate"]) for r in results(SI.CAP)] == [(r["primary"], r["mate"]) for r in results(None)]


def test_flags_travel_with_the_mate():
    q, lab = SI.flags_set()
    res = [SM.align_split(ref(), s, SI.FLAGS_CAP) for s in q]
    for r, l in zip(res, lab):
        assert r["mate"]["tid"] >= 0 and r["mate"]["flags"] == r["primary"]["flags"] == (SRT.F_OVERFLOW if l.startswith("overflow") else SRT.F_MASKED), (l, r)
    assert res[2]["primary"]["q_end"] - res[2]["primary"]["q_beg"] == 60   # the masked read's primary still holds all 60 bases: the unmasked seeds behind base 30 found it


def test_cli_names():
    fq = SI.cli_set()
    assert len(fq) >= 200 and any(" " in n for n, _, _ in fq) and any("\t" in n for n, _, _ in fq) and any(n == SI.cli_name(n) for n, _, _ in fq)
    assert all(SI.cli_name(n).endswith(("/1", "/2")) and SI.cli_name(n) != s for n, s, _ in fq)
    assert len({SI.cli_name(n) for n, _, _ in fq}) == len(fq)


def test_e2e_goldens_hold_the_property():
    """tests/golden/realign_split (written by tests/golden/make_realign_split_reference.py from the real reference's getclip and getsv): with -F the SV
    table or stdout names both ends of the planted junction, without -F neither does; and the reads of the recorded prefix.unmapped_2.fq.gz are the
    sample's unmapped reads, whose model rows make that junction pair by pair with ten different split points"""
    import gzip
    import os

    import golden_util as G
    import readthrough_model as RT
    assert SI.e2e_names_both_ends(G.read_text("realign_split", "e2e.F.sv")) or SI.e2e_names_both_ends(G.read_text("realign_split", "e2e.F.stdout"))
    assert not SI.e2e_names_both_ends(G.read_text("realign_split", "e2e.sv")) and not SI.e2e_names_both_ends(G.read_text("realign_split", "e2e.stdout"))
    contigs, recs = SI.e2e_sample()
    assert not any("S" in r["cigar"] for r in recs)
    lines = gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "realign_split", "e2e.unmapped_2.fq.gz"), "rt").read().splitlines()
    unmapped = {r["qname"] + "/2": r["seq"] for r in recs if r["flag"] & 4}
    assert dict(zip((l[1:] for l in lines[0::4]), lines[1::4])) == unmapped and len(unmapped) == SI.E2E_READS
    rf = M.Reference(contigs)
    rows = [r for name, s in unmapped.items() for r in SM.bam_records(name, s, "I" * len(s), SM.align_split(rf, s))]
    batch, names = RT.batch_from_records([dict(qname=r["name"], flag=r["flag"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar="".join(f"{n}{op}" for n, op in r["cigar"]),
                                               seq=r["seq"]) for r in rows])
    pairs, n_cand = RT.find_junction([batch], [names], 1, list(SI.E2E_NAMES))
    assert n_cand == 2 * SI.E2E_READS and len(pairs) == SI.E2E_READS
    assert {p["key"] for p in pairs} == {("tA", SI.E2E_A + 1, "+", "tB", SI.E2E_B + 1, "+")}
    assert len({len(p["up_seq"]) for p in pairs}) == SI.E2E_READS
