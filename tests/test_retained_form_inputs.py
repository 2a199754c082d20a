"""The record sets of tests/retained_form_inputs.py are what tests/test_retained_form_gpu.py takes them for: the plain models accept them, neither duplicate rule
marks a record of FORM, and SEAM needs its sort and its marks across the cut.  No GPU."""
import coordsort_model as cm
import markdup_inputs as mi
import markdup_model as mm
import pairdup_model as pm
import retained_form_inputs as rf

NT = len(rf.TARGETS)


def test_form_has_every_shape_and_no_duplicates():
    recs = rf.FORM
    assert 18 <= len(recs) <= 22 and mm.sorted_ok(recs) and cm.is_sorted(recs, NT)
    assert cm.order(recs, NT) == list(range(len(recs)))
    ops = [pm.cigar_ops(r) for r in recs]
    assert recs[-1]["tid"] == -1 and ops[-1] == [] and all(r["tid"] >= 0 for r in recs[:-1])       # the unplaced record without operations, last
    assert sum(len(o) == 17 for o in ops) == 1
    clipped = [bool(o) and "S" in (o[0][1], o[-1][1]) for o in ops]
    assert any(c and len(r["seq"]) == 40 for c, r in zip(clipped, recs)) and 0 < sum(clipped) < len(recs)
    assert {r["tid"] for r in recs if r["tid"] >= 0} == {0, 1}
    assert len({(r["tid"], r["pos"]) for r in recs}) == len(recs)
    assert all(len(r["qual"]) == len(r["seq"]) > 0 for r in recs)
    # neither rule marks anything, with whole digests and with digests of one bit (every name collides) - and both rules have records that take part
    flags = [r["flag"] for r in recs]
    for bits in (64, 1):
        assert mm.mark(recs, bits) == flags and pm.mark(recs, bits) == flags
    assert sum(mm.takes_part(r) for r in recs) == 8 and sum(pm.takes_part(r) for r in recs) == 8
    st = {}
    pm.mark(recs, 64, st)
    assert st["pairs"] == 4 and st["groups_many"] == 0 and st["pairs_marked"] == 0
    # in any other order too (the sort's producer is handed the reverse)
    assert pm.mark(recs[::-1]) == flags[::-1] and cm.order(recs[::-1], NT) == list(range(len(recs) - 1, -1, -1))
    assert mi.sam_text(recs, rf.TARGETS).count(b"\n") == len(recs)


def test_one_and_none():
    assert len(rf.ONE) == 1 and rf.NONE == [] and rf.ONE[0]["tid"] >= 0
    assert pm.mark(rf.ONE) == [rf.ONE[0]["flag"]] and mm.mark(rf.ONE) == [rf.ONE[0]["flag"]] and cm.order(rf.ONE, NT) == [0] and cm.order(rf.NONE, NT) == []


def test_seam_needs_the_other_side():
    recs, cut = rf.SEAM, rf.SEAM_CUT
    assert 0 < cut < len(recs) and not cm.is_sorted(recs, NT)
    order = cm.order(recs, NT)
    assert all(i >= cut for i in order[:len(recs) - cut]) and all(i < cut for i in order[len(recs) - cut:])   # the second batch in front of the first
    found, unpaired = pm.pairs(recs)
    assert not unpaired and len(found) == cut and all(a < cut <= b for a, b in found)                          # every pair's mates on either side
    flags = pm.mark(recs)
    marked = [i for i, (r, f) in enumerate(zip(recs, flags)) if f != r["flag"]]
    assert any(i < cut for i in marked) and any(i >= cut for i in marked) and len(marked) == 10
    assert not pm.score_ties(recs)
