"""Every query set of tests/realign_alts_inputs.py held to the property it was built for, through the model alone (tests/realign_alts_model.py).  CPU only.
What the GPU test compares with the model is therefore known to contain the cases: an input that drifts from its rule fails here, not silently there."""
import functools

import pytest

import realign_alts_inputs as AI
import realign_alts_model as AM
import realign_gapped_model as GM
import realign_inputs as I
import realign_model as M
import realign_sorted_model as SM

INDEXES = [None, AI.CAP]
IDS = ["hash", "sorted"]


@functools.lru_cache(maxsize=None)
def ref():
    return M.Reference(AI.reference())


def run(fn, max_alt=16, max_occ=None, gapped=False):
    q, lab = fn()
    return {k: AM.align_alts(ref(), s, max_alt, max_occ, gapped) for s, k in zip(q, lab)}


def at(name):
    """(tid, pos) of a planted piece"""
    p = AI.where(name)
    t = ref().contig_of(p)
    return t, p - ref().off[t]


def loci(r):
    return [(a["tid"], a["pos"]) for a in r["alts"]]


def test_reference_is_small_and_named():
    assert len(AI.reference()) == len(AI.NAMES) and 4000 < sum(len(c) for c in AI.reference()) < 9000


@pytest.mark.parametrize("max_occ", INDEXES, ids=IDS)
def test_ratio_and_its_equality(max_occ):
    by = run(AI.ratio_set, 16, max_occ)
    for st, rev in (("fwd", 0), ("rev", 1)):
        r = by[f"ratio/{st}"]
        assert (r["primary"]["tid"], r["primary"]["pos"], r["primary"]["score"], r["primary"]["reverse"]) == at("ratio0") + (60, rev)
        assert loci(r) == [at("ratio2")] and r["alts"][0]["score"] == 50 and r["alts"][0]["second"] == 60 and r["alts"][0]["mapq"] == 0
        r = by[f"equality/{st}"]
        assert (r["primary"]["tid"], r["primary"]["pos"], r["primary"]["score"]) == at("eq0") + (50,)
        assert loci(r) == [at("eq40")] and r["alts"][0]["score"] == 40
    scores = sorted(c[0] for c in AM.scored_candidates(ref(), AI.element("ratio"), max_occ))
    assert scores == [45, 50, 60]      # the copy with three substitutions is scored: the ratio keeps it out
    scores = sorted(c[0] for c in AM.scored_candidates(ref(), AI.element("eq"), max_occ))
    assert scores == [39, 40, 50]      # 5 * 40 == 4 * 50 is in, 39 is out


@pytest.mark.parametrize("max_occ", INDEXES, ids=IDS)
def test_floor(max_occ):
    by = run(AI.floor_set, 16, max_occ)
    for st in ("fwd", "rev"):
        r = by[f"floor/{st}"]
        assert r["primary"]["score"] == 36 and loci(r) == [at("floor30")] and r["alts"][0]["score"] == 30
    assert 5 * 29 >= 4 * 36            # the locus with 29 bases would pass the ratio: it is the floor that keeps it out
    assert sorted(c[0] for c in AM.scored_candidates(ref(), AI.element("floor"), max_occ)) == [30, 36]


@pytest.mark.parametrize("max_occ", INDEXES, ids=IDS)
def test_order(max_occ):
    by = run(AI.order_set, 16, max_occ)
    r = by["order/fwd"]
    assert (r["primary"]["tid"], r["primary"]["pos"]) == at("order0")
    assert loci(r) == [at("order_f2"), at("order_f1"), at("order_r")] and [a["score"] for a in r["alts"]] == [55, 55, 55]
    assert [a["reverse"] for a in r["alts"]] == [0, 0, 1]
    assert AI.where("order_r") < AI.where("order_f2") < AI.where("order_f1")   # the reverse copy has the smallest diagonal and still comes last
    r = by["contig/fwd"]
    assert (r["primary"]["tid"], r["primary"]["pos"], r["primary"]["score"]) == at("span36") + (36,)
    assert loci(r) == [at("span_a"), at("span_b")] and [a["score"] for a in r["alts"]] == [30, 30]
    a, b = r["alts"]
    assert a["tid"] + 1 == b["tid"] and (a["q_beg"], a["q_end"], b["q_beg"], b["q_end"]) == (0, 30, 30, 60)
    assert ref().off[a["tid"]] + a["pos"] - a["q_beg"] == ref().off[b["tid"]] + b["pos"] - b["q_beg"]   # one diagonal, two contigs
    assert not r["tie"]


@pytest.mark.parametrize("max_occ", INDEXES, ids=IDS)
def test_both_strands(max_occ):
    by = run(AI.strand_set, 16, max_occ)
    r = by["both/fwd"]
    assert (r["primary"]["tid"], r["primary"]["pos"], r["primary"]["reverse"], r["primary"]["mapq"]) == at("both_f") + (0, 0)
    assert loci(r) == [at("both_r")] and r["alts"][0]["reverse"] == 1 and r["alts"][0]["score"] == 60
    r = by["both/rev"]
    assert (r["primary"]["tid"], r["primary"]["pos"], r["primary"]["reverse"]) == at("both_r") + (0,)
    assert loci(r) == [at("both_f")] and r["alts"][0]["reverse"] == 1


@pytest.mark.parametrize("max_occ", INDEXES, ids=IDS)
def test_tandem_32_and_33(max_occ):
    by = run(AI.tandem_set, 16, max_occ)
    for st in ("fwd", "rev"):
        r = by[f"tandem32/{st}"]
        assert r["alts"] == [] and r["primary"]["second"] == 0 and r["primary"]["score"] == 40
        cands = AM.scored_candidates(ref(), AI.tandem_set()[0][0], max_occ)
        assert sorted(c[2] for c in cands)[1] - sorted(c[2] for c in cands)[0] == 32 and all(5 * c[0] >= 4 * 40 for c in cands)   # qualifies by score: one locus
        r = by[f"tandem33/{st}"]
        assert len(r["alts"]) == 1 and abs(r["alts"][0]["pos"] - r["primary"]["pos"]) == 33 and r["alts"][0]["tid"] == r["primary"]["tid"]


@pytest.mark.parametrize("max_occ", INDEXES, ids=IDS)
def test_suppressed_by_an_alternate(max_occ):
    for max_alt in (1, 16):
        by = run(AI.suppress_set, max_alt, max_occ)
        r = by["suppress/fwd"]
        assert (r["primary"]["tid"], r["primary"]["pos"], r["primary"]["score"]) == at("supp0") + (48,)
        prim = (0, r["primary"]["tid"], AI.where("supp0"))
        cands = [c for c in AM.scored_candidates(ref(), AI.element("supp"), max_occ) if c[0] >= 30 and 5 * c[0] >= 4 * 48 and not AM.same_locus((c[1], c[3], c[2]), prim)]
        assert len(cands) == 2 and abs(cands[0][2] - cands[1][2]) == 5 and {c[3] for c in cands} == {at("supp_del")[0]}
        assert len(r["alts"]) == 1 and r["primary"]["flags"] == 0    # the second diagonal went with the first: not an alternate, and not cut either


@pytest.mark.parametrize("max_occ", INDEXES, ids=IDS)
def test_family_and_max_alt(max_occ):
    want = [at(f"family{i}") for i in range(1, AI.N_FAMILY)]
    for max_alt in (1, 2, 16):
        by = run(AI.family_set, max_alt, max_occ)
        for st in ("fwd", "rev"):
            r = by[f"family/{st}"]
            assert (r["primary"]["tid"], r["primary"]["pos"]) == at("family0")
            assert loci(r) == want[:max_alt] and r["primary"]["flags"] & AM.F_ALT_CUT and all(a["flags"] == r["primary"]["flags"] for a in r["alts"])
            assert not r["overflow"]
    assert len(want) == 17


@pytest.mark.parametrize("max_occ", INDEXES, ids=IDS)
def test_partial_copy(max_occ):
    by = run(AI.hang_set, 16, max_occ)
    r = by["hang/fwd"]
    a = r["alts"][0]
    assert loci(r) == [at("hang46")] and (a["q_beg"], a["q_end"], a["score"]) == (0, 46, 46)
    a = by["hang/rev"]["alts"][0]
    assert (a["q_beg"], a["q_end"], a["reverse"]) == (0, 46, 1)


def test_alternates_hang_over_a_contigs_end():
    """the order set's "contig" query: its first alternate ends exactly with its contig and its diagonal runs 30 bases on into the next one; the second
    begins exactly with that contig and its diagonal starts 30 bases before it"""
    t, p = at("span_a")
    assert p + 30 == len(AI.reference()[t]) and at("span_b") == (t + 1, 0)


@pytest.mark.parametrize("max_occ", INDEXES, ids=IDS)
def test_gapped(max_occ):
    by = run(AI.gapped_set, 16, max_occ, gapped=True)
    for st in ("fwd", "rev"):
        r = by[f"gain/{st}"]
        assert r["primary"]["gap_len"] == -2 and r["primary"]["score"] == 70 - 2 - 8 and (r["primary"]["tid"], r["primary"]["pos"]) == at("gap_locus")
        assert loci(r) == [at("gap32")] and r["alts"][0]["score"] == 32
        first = GM.first_stage(ref(), AI.gapped_set()[0][0 if st == "fwd" else 1], max_occ)[0]["score"]
        assert 35 <= first < 40 and r["alts"][0]["second"] == first and r["primary"]["second"] == 32   # the first stage's best, not the refined 60
        r = by[f"late/{st}"]
        assert r["primary"]["tid"] == -1 and r["alts"] == []
        assert max(c[0] for c in AM.scored_candidates(ref(), AI.gapped_set()[0][2], max_occ, gapped=True)) == 26   # through the floor, unaligned behind it
        assert by[f"rescue/{st}"]["primary"]["gap_len"] != 0 and by[f"rescue/{st}"]["alts"] == []
        assert by[f"stays/{st}"]["primary"]["tid"] == -1


def test_flags_on_the_sorted_index():
    by = run(AI.flags_set, 16, AI.FLAGS_CAP)
    for st in ("fwd", "rev"):
        r = by[f"overflow/{st}"]
        assert r["primary"]["flags"] == SM.F_OVERFLOW and loci(r) == [at("long1"), at("long2")] and all(a["flags"] == SM.F_OVERFLOW for a in r["alts"])
        r = by[f"masked/{st}"]
        assert r["primary"]["flags"] == SM.F_MASKED and loci(r) == [at("mask1")] and r["alts"][0]["flags"] == SM.F_MASKED
        r = by[f"family/{st}"]
        assert r["primary"]["flags"] & SM.F_MASKED and 0 < len(r["alts"]) < 17


def test_mix_interleaves():
    q, lab = AI.mix_set()
    res = [AM.align_alts(ref(), s, 8) for s in q]
    has = [len(r["alts"]) > 0 for r in res]
    assert len(q) == AI.N_MIX > 2048 and len(q) % 4
    assert 300 < sum(has) < len(q) - 300 and sum(a != b for a, b in zip(has, has[1:])) > 400   # with and without, in turn
    assert sum(r["primary"]["tid"] < 0 for r in res) > 50 and {len(s) for s in q} >= {19, 1025}
    assert any(r["primary"]["flags"] & AM.F_ALT_CUT for r in res)                                 # the family at max_alt 8
    assert has[2048:].count(True) >= 1                                                            # an alternate behind the scan's first tile


@pytest.mark.parametrize("max_occ", INDEXES, ids=IDS)
def test_nothing_is_left_to_the_kernels_order(max_occ):
    """no query of the sets that run on the hash index has more seeds than slots or a primary tied between two contigs"""
    q, lab = AI.all_queries()
    bad = [l for s, l in zip(q, lab) for r in [AM.align_alts(ref(), s, 8, max_occ, gapped=l.startswith("gapped:"))] if r["overflow"] or r["tie"]]
    assert not bad, bad
    n_below = 0
    for s in q:   # the primary is the plain model's, `second` included where it is a candidate that its end extension took below 30
        want = M.align(ref(), s) if max_occ is None else SM.align_sorted(ref(), s, max_occ)
        got = AM.align_alts(ref(), s, 8, max_occ)["primary"]
        assert {k: got[k] for k in M.FIELDS} == {k: want[k] for k in M.FIELDS}, s
        n_below += 0 < want["second"] < 30
    assert n_below >= 3
    n_gap = 0
    for s in q[:len(q) - AI.N_MIX + 400]:   # gapped: the primary is realign_gapped_model.align_gapped's (every set and 400 of the mix)
        want = GM.align_gapped(ref(), s, max_occ)
        got = AM.align_alts(ref(), s, 8, max_occ, gapped=True)["primary"]
        got["flags"] &= ~AM.F_ALT_CUT   # (the one bit that is the alternates' own)
        assert {k: got[k] for k in M.FIELDS + GM.GAP_FIELDS + ("flags",)} == {k: want[k] for k in M.FIELDS + GM.GAP_FIELDS + ("flags",)}, s
        n_gap += want["gap_len"] != 0
    assert n_gap >= 4
    for name, fn in (("sweep", I.sweep_set), ("tandem", I.tandem_set), ("two-locus", I.two_locus_set)):
        contigs, queries, labels = fn()
        r2 = M.Reference(contigs)
        bad = [l for s, l in zip(queries, labels) for r in [AM.align_alts(r2, s, 16, max_occ)] if r["overflow"] or r["tie"]]
        assert not bad, (name, bad)


def test_an_alternate_from_the_winners_lane():
    """more than 64 candidate slots: realign_inputs.sweep_set() on the sorted index, where the slot of every seed is the model's.  For some query the
    alternate's first slot is the winner's first slot + 64: the winner's lane scored it in another round"""
    contigs, queries, _ = I.sweep_set()
    r2 = M.Reference(contigs)
    found = 0
    for s in queries:
        ori = M.orientations(s)
        seeds = sorted((SM.occ_class(len(r2.index[ori[st][o:o + M.K]])), st, o, p) for st in (0, 1) for o in range(len(s) - M.K + 1)
                       for p in r2.index.get(ori[st][o:o + M.K], ()))[:M.MAX_CAND]
        first = {}
        for slot, (_, st, o, p) in enumerate(seeds):
            first.setdefault((st, r2.contig_of(p), p - o), slot)
        r = AM.align_alts(r2, s, 16, AI.CAP)
        assert len(r["alts"]) == 1
        prim, alt = r["primary"], r["alts"][0]
        key = lambda h: (h["reverse"], h["tid"], r2.off[h["tid"]] + h["pos"] - h["q_beg"])  # noqa: E731
        found += first[key(alt)] == first[key(prim)] + 64
    assert found >= 2


def test_tandem_array_cuts_at_sixteen():
    """realign_inputs.tandem_set(): up to 90 diagonals 36 apart - more loci than 16 alternates"""
    contigs, queries, _ = I.tandem_set()
    r2 = M.Reference(contigs)
    res = [AM.align_alts(r2, s, 16) for s in queries[::9]]
    assert sum(len(r["alts"]) == 16 and bool(r["primary"]["flags"] & AM.F_ALT_CUT) for r in res) > len(res) // 2


def test_cli_set():
    fq = AI.cli_set()
    assert len(fq) > 150 and all(len(s) == len(q) <= 254 for s, q in fq) and len({s for s, _ in fq}) == len(fq)


def test_golden_tables_hold_the_samples_property():
    """tests/golden/realign_alts (the real reference's getsv over the model's records, written by tests/golden/make_realign_alts_reference.py, which asserts
    the same): with the secondary records the planted junction's two ends are named in the table or among the filtered junctions on stdout, with the
    primaries alone in neither; and the sample is what the generator saw: five copies, the clip inside copy 3"""
    import golden_util as G
    a, b = ("tA", str(AI.E2E_A + 1)), ("tB", str(AI.E2E_B + 1))

    def named(text):
        return any(a in set(zip(f, f[1:])) and b in set(zip(f, f[1:])) for f in (l.split("\t") for l in text.splitlines()))
    assert named(G.read_text("realign_alts", "e2e.sv")) or named(G.read_text("realign_alts", "e2e.stdout"))
    assert not named(G.read_text("realign_alts", "e2e.primary.sv")) and not named(G.read_text("realign_alts", "e2e.primary.stdout"))
    contigs, recs = AI.e2e_sample()
    clip = contigs[1][AI.E2E_B:AI.E2E_B + AI.E2E_CLIP]
    assert [i for i in range(len(contigs[1])) if contigs[1].startswith(clip, i)] == [p + 10 for p in AI.E2E_COPIES] and AI.E2E_B == AI.E2E_COPIES[2] + 10
    r = AM.align_alts(M.Reference(contigs), clip, 8, AI.CAP)
    assert (r["primary"]["pos"], r["primary"]["mapq"]) == (AI.E2E_COPIES[0] + 10, 0) and [x["pos"] for x in r["alts"]] == [p + 10 for p in AI.E2E_COPIES[1:]]
    assert sum(1 for x in recs if x["mapq"] == 0) == 5   # the repeat side's own clipped reads, which getclip drops
