"""The sample of tests/test_pairdup_cli_gpu.py (tests/pairdup_cli_inputs.py) has the properties the CLI test relies on.  No GPU."""
import coordsort_inputs as ci
import markdup_cli_inputs as CI
import markdup_model as mm
import pairdup_cli_inputs as PI
import pairdup_model as pm


def test_the_pair_rule_marks_what_the_aligned_rule_misses():
    contigs, recs = PI.sample()
    recs = list(recs)
    assert len(recs) == len(ci.cli_sample()[1]) and mm.sorted_ok(recs) and all(not r["flag"] & 0x400 for r in recs)
    st = {}
    by_pair = pm.mark(recs, stats=st)
    by_m = mm.mark(recs)
    plain = [r["flag"] for r in recs]
    marked = sorted(r["qname"] for r, f in zip(recs, by_pair) if f != r["flag"])
    assert marked == sorted(2 * [f"A{j}copy{k}" for j in range(2) for k in range(CI.COPIES)])      # both reads of every copy, nothing else
    assert by_pair != plain and by_pair != by_m and by_m == plain                                  # -M's rule finds none of them
    assert st["pairs_marked"] == 2 * CI.COPIES and st["groups_many"] == 2 and st["unpaired"] == 0
    assert st["taking_part"] == 2 * st["pairs"] < st["records"]
    # the copies of an original: four aligned positions, one unclipped 5' end, and lower qualities than the original's
    for j in range(2):
        firsts = [r for r in recs if r["qname"].startswith(f"A{j}") and r["tid"] == 0]
        assert len({r["pos"] for r in firsts}) == 1 + CI.COPIES and len({pm.end_u(r) for r in firsts}) == 1
        assert max(firsts, key=pm.read_score)["qname"] == f"A{j}"
    # the marks do not depend on the order (no score ties inside a group)
    assert not pm.score_ties(recs)
    for order in (ci.shuffled(recs), ci.by_name(recs)):
        assert sorted(r["qname"] for r, f in zip(order, pm.mark(order)) if f != r["flag"]) == marked
