"""tests/realign_gapped_inputs.py held to what each set was built for, with the models alone (CPU): the GPU comparison of
tests/test_realign_gapped_gpu.py means what its sets' names say only while these hold.  A set that misses its property is changed, not excused."""
import functools

import realign_gapped_inputs as GI
import realign_gapped_model as GM
import realign_model as M


@functools.lru_cache(maxsize=None)
def ref():
    return M.Reference(GI.reference())


@functools.lru_cache(maxsize=None)
def results(name):
    """[(label, query, gapped hit on the hash index, the same on the sorted index, ungapped hit)]"""
    q, lab = GI.SETS[name]()
    return [(l, s, GM.align_gapped(ref(), s), GM.align_gapped(ref(), s, 500), M.align(ref(), s)) for s, l in zip(q, lab)]


def test_reference_shape():
    c = GI.reference()
    off = GI.offsets(c)
    assert len(c) == 10 and all(1000 <= len(x) <= 2000 for x in c)
    assert all(o % 4 and o % 32 for o in off[1:-1])
    t = c[GI.TANDEM_CONTIG]
    run = GI.TANDEM_UNIT * GI.TANDEM_COPIES
    assert t[GI.TANDEM_AT:GI.TANDEM_AT + len(run)] == run and t[GI.TANDEM_AT - 1] != "G" and t[GI.TANDEM_AT + len(run)] != "C"
    h = c[GI.HOMO_CONTIG]
    assert h[GI.HOMO_AT:GI.HOMO_AT + GI.HOMO_LEN] == "A" * GI.HOMO_LEN and "A" not in h[GI.HOMO_AT - 1] + h[GI.HOMO_AT + GI.HOMO_LEN]
    assert max(len(v) for v in ref().index.values()) == 1   # no repeated 20-mer: nothing is masked, the sorted index sees the hash index's seeds


def test_no_query_is_left_to_the_kernel():
    """no `overflow`, no `tie` (the hash model's undetermined classes), and both kinds of index give one answer - but for the flags"""
    n = 0
    for name in GI.SETS:
        for l, s, g, gs, u in results(name):
            assert not g["overflow"] and not g["tie"] and not u["overflow"] and not u["tie"], (name, l)
            assert {k: g[k] for k in M.FIELDS + GM.GAP_FIELDS} == {k: gs[k] for k in M.FIELDS + GM.GAP_FIELDS}, (name, l)
            assert gs["flags"] in (0, GM.F_OVERFLOW) and (gs["flags"] == 0 or len(s) > 700), (name, l)
            assert g["score"] >= u["score"], (name, l)
            assert (g["gap_len"] != 0) == (g["score"] > u["score"]) or u["tid"] < 0, (name, l)
            n += 1
    assert n == len(GI.all_queries()[0]) > 600


def test_both_strands_give_one_alignment():
    for name in GI.SETS:
        r = results(name)
        for (l0, _, g0, _, _), (l1, _, g1, _, _) in zip(r[0::2], r[1::2]):
            assert l0.endswith("/fwd") and l1.endswith("/rev") and l0[:-4] == l1[:-4]
            if g0["tid"] >= 0:
                assert (g0["reverse"], g1["reverse"]) == (0, 1), l0
                assert {k: g0[k] for k in M.FIELDS + GM.GAP_FIELDS if k != "reverse"} == {k: g1[k] for k in M.FIELDS + GM.GAP_FIELDS if k != "reverse"}, l0


def test_length_set():
    for l, s, g, _, u in results("length"):
        kind, L = l[0], int(l[1:l.index("-")])
        if L == 17:
            assert g["gap_len"] == 0 and {k: g[k] for k in M.FIELDS} == {k: u[k] for k in M.FIELDS}, l
            assert 50 <= g["score"] <= 53 and g["q_end"] - g["q_beg"] < 60, l
        else:
            assert g["gap_len"] == (L if kind == "D" else -L), l
            assert (g["q_beg"], g["q_end"], g["n_mismatch"]) == (0, 100, 0) and g["score"] == (100 if kind == "D" else 100 - L) - 6 - L, l
            assert 50 - 3 <= g["gap_at"] <= 50, l   # (left-aligned: a few bases earlier where the bases allow it)


def test_place_set():
    for l, s, g, _, u in results("place"):
        kind, place = l[0], l[2:l.rindex("-")]
        whole = 60 - 7 if kind == "D" else 60 - 1 - 7
        if place.startswith("7-"):
            assert g["gap_len"] == 0 and g["score"] == whole == u["score"] and g["q_end"] - g["q_beg"] == whole, l   # 7 matches pay for the gap exactly: no gap
        else:
            assert g["gap_len"] == (1 if kind == "D" else -1) and g["score"] == whole and (g["q_beg"], g["q_end"]) == (0, 60), l
            short = 30 if place == "middle" else int(place.split("-")[0])
            at = short if place.endswith("start") or place == "middle" else 60 - short - (kind == "I")
            assert at - 2 <= g["gap_at"] <= at, l
            if place.startswith("8-"):
                assert u["score"] == whole - 1, l   # the other side of the break-even: one point won
            assert g["side"] == ("right" if place.endswith("start") else "left"), l


def test_side_set():
    for l, s, g, _, _ in results("side"):
        assert g["gap_len"] == (2 if l[0] == "D" else -2) and g["side"] == l.split("-")[2] and (g["q_beg"], g["q_end"]) == (0, 100), l
    assert {g["side"] for _, _, g, _, _ in results("side")} == {"left", "right"}


def test_rescue_set():
    for l, s, g, _, u in results("rescue"):
        assert u["tid"] == -1, l
        if l.startswith("rescue"):
            L = int(l[8])
            assert g["tid"] >= 0 and abs(g["gap_len"]) == L and g["score"] == 50 - 6 - L and g["n_mismatch"] == 0 and g["q_end"] - g["q_beg"] == len(s), l
        else:
            assert {k: g[k] for k in M.FIELDS} == M.UNALIGNED and g["gap_len"] == 0, l
            w = GM.first_stage(ref(), s)[0]
            assert w is not None and 20 <= w["score"] < 30, l   # the floor let it through (25, or 21 with the mismatch at the query's end); the refinement found nothing


def test_edge_set():
    off = GI.offsets(GI.reference())
    for l, s, g, _, _ in results("edge"):
        t, over = int(l[l.index("-D-") - 1] if "-D-" in l else l[l.index("-I-") - 1]), int(l[l.rindex("-") + 1:l.index("/")])
        assert g["tid"] == t and abs(g["gap_len"]) == 2, l
        clen = off[t + 1] - off[t]
        if l.startswith("over-end"):
            assert g["q_end"] == len(s) - over and g["side"] == "left", l   # the right piece is the free one and stops at the contig's last base
            assert g["pos"] + (g["q_end"] - g["q_beg"]) + g["gap_len"] == clen, l
        else:
            assert g["q_beg"] == over and g["pos"] == 0 and g["side"] == "right", l


def test_repeat_set():
    for l, s, g, _, _ in results("repeat"):
        left = int(l[l.rindex("-") + 1:l.index("/")])
        want = dict([("tandem-unit-less", 3), ("tandem-unit-more", -3), ("homopolymer-2-less", 2), ("homopolymer-1-more", -1)])[l[:l.rindex("-")]]
        assert (g["gap_at"], g["gap_len"]) == (left, want), l   # the repeat's first base: the smallest k
        assert (g["q_beg"], g["q_end"], g["n_mismatch"]) == (0, len(s), 0), l
    assert {g["side"] for _, _, g, _, _ in results("repeat")} == {"left", "right"}


def test_substitution_set():
    for l, s, g, _, u in results("substitution"):
        assert u["tid"] >= 0 and u["n_mismatch"] >= 1, l
        assert g["gap_len"] == 0 and {k: g[k] for k in M.FIELDS} == {k: u[k] for k in M.FIELDS}, l


def test_limit_set():
    by = {l: (s, g, gs) for l, s, g, gs, _ in results("limit")}
    for strand in ("/fwd", "/rev"):
        assert len(by["exact-20" + strand][0]) == 20 and by["exact-20" + strand][1]["tid"] == -1
        assert len(by["long-1025" + strand][0]) == 1025 and by["long-1025" + strand][1]["tid"] == -1
        assert by["exact-1024" + strand][1]["score"] == 1024 and by["exact-1024" + strand][1]["gap_len"] == 0
        for kind, L in (("D", 1), ("I", -1)):
            for end in ("end", "start"):
                s, g, gs = by[f"long-{kind}-19-from-{end}{strand}"]
                assert len(s) == 1024 and g["gap_len"] == L and (g["q_beg"], g["q_end"]) == (0, 1024) and g["score"] == 1024 - (kind == "I") - 7, (kind, end)
                assert gs["flags"] == GM.F_OVERFLOW and len(M.seeds(ref(), s)) > M.MAX_CAND


def test_junk_set():
    n_counted = 0
    for l, s, g, _, _ in results("junk"):
        assert not set(s) <= set("ACGTacgt"), l
        assert abs(g["gap_len"]) == 3 and (g["q_beg"], g["q_end"]) == (0, 80), l
        where = l.split("-")[2]
        assert g["n_mismatch"] == dict(before=1, behind=1, both=2, inserted=0)[where], l   # a byte that is no base costs a mismatch, an inserted one nothing
        assert g["score"] == 80 - (3 if g["gap_len"] < 0 else 0) - 9 - 5 * g["n_mismatch"], l
        n_counted += g["n_mismatch"] > 0
    assert n_counted >= 12


def test_many_set():
    r = results("many")
    assert len(r) > 256 and len(r) % 4
    with_gap = [g for _, _, g, _, _ in r if g["gap_len"]]
    assert len(with_gap) >= len(r) // 2
    assert {abs(g["gap_len"]) for g in with_gap} == set(range(1, 17)) and {g["gap_len"] > 0 for g in with_gap} == {True, False}
    assert {g["side"] for g in with_gap} == {"left", "right"} and any(g["n_mismatch"] for g in with_gap) and any(g["q_end"] - g["q_beg"] < len(s) for _, s, g, _, _ in r if g["gap_len"])


def test_cli_set():
    fq = GI.cli_set()
    assert len(fq) > 500 and all(0 < len(s) == len(q) <= 254 for s, q in fq) and len({s for s, _ in fq}) == len(fq)


def test_golden_table_holds_the_planted_junction():
    """tests/golden/realign_gapped/e2e.sv (the real reference's getsv on the model's gapped records, tests/golden/make_realign_gapped_reference.py): one
    row, from tA's last base before the breakpoint to tB's first base behind it, the clip's CIGAR with the planted deletion"""
    import golden_util as G
    rows = [l.split("\t") for l in G.read_text("realign_gapped", "e2e.sv").splitlines() if not l.startswith("@")]
    assert len(rows) == 1
    r = rows[0]
    assert (r[0], int(r[1]), r[2], r[4], int(r[5]), r[6]) == ("tA", GI.E2E_A + 1, "+", "tB", GI.E2E_B + 1, "+")
    assert int(r[3]) == 10 and r[20] == f"{GI.E2E_DEL_AT}M{GI.E2E_DEL}D{GI.E2E_CLIP - GI.E2E_DEL_AT}M"
    contigs, recs = GI.e2e_sample()
    assert [len(c) for c in contigs] == list(GI.E2E_LENS)
    clips = [x for x in recs if x["qname"].startswith("jn") and x["flag"] == 97]
    assert len(clips) == 10 and all(x["cigar"].endswith(f"M{GI.E2E_CLIP}S") and x["pos"] + int(x["cigar"].split("M")[0]) == GI.E2E_A + 1 for x in clips)
    clip = clips[0]["seq"][-GI.E2E_CLIP:]
    g = GM.align_gapped(M.Reference(contigs), clip)
    assert (g["tid"], g["pos"], g["gap_at"], g["gap_len"], g["q_beg"], g["q_end"]) == (1, GI.E2E_B, GI.E2E_DEL_AT, GI.E2E_DEL, 0, GI.E2E_CLIP)
    u = M.align(M.Reference(contigs), clip)
    assert (u["pos"], u["q_beg"]) == (GI.E2E_B + GI.E2E_DEL_AT + GI.E2E_DEL, GI.E2E_DEL_AT)   # without the gap: behind the deletion, 26 bases clipped towards the breakpoint
