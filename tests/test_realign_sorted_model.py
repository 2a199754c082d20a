"""The model of the re-aligner's sorted index (tests/realign_sorted_model.py) on the CPU: where no repeat is in play it is the plain model of
tests/realign_model.py, and on the repeat reference of tests/realign_sorted_inputs.py the hand cases come out as they were built.  The GPU
comparison (tests/test_realign_sorted_gpu.py) holds the kernels against this model in every field and flag."""
import pytest

import realign_inputs as I
import realign_model as M
import realign_sorted_inputs as SI
import realign_sorted_model as SM

E_TID, F_TID, POLY_TID, C35_TID = (SI.NAMES.index(x) for x in ("E", "F", "polyA", "c35"))


@pytest.mark.parametrize("shape", list(I.SHAPES))
@pytest.mark.parametrize("which", ["random", "threshold"])
def test_equals_the_plain_model_without_repeats(shape, which):
    """random references, cap 500: every field of every query the plain model determines (neither `overflow` nor `tie`); flags 0 - but for the
    1024-base substrings, whose 251 seeds lie on one diagonal: the plain model does not call that `overflow`, the admission rule leaves 59 seeds
    out and says so (OVERFLOW), and the hit is the same"""
    contigs, queries = (I.random_set(shape) if which == "random" else I.threshold_set(shape))[:2]
    ref = M.Reference(contigs)
    n = n_over = 0
    for q in queries:
        w = M.align(ref, q)
        if w["overflow"] or w["tie"]:
            continue
        s = SM.align_sorted(ref, q, 500)
        assert {k: s[k] for k in M.FIELDS} == {k: w[k] for k in M.FIELDS}, q
        assert s["n_masked_kmers"] == 0 and s["n_admitted"] == min(w["n_seeds"], M.MAX_CAND), q
        assert s["flags"] == (SM.F_OVERFLOW if w["n_seeds"] > M.MAX_CAND else 0), q
        n_over += w["n_seeds"] > M.MAX_CAND
        n += 1
    assert n >= len(queries) - 4 and n_over == (2 if which == "random" else 0)


def test_index_stats_of_the_repeat_reference():
    ref = SI.repeat_model()
    n_e = sum(1 for v in ref.index.values() if len(v) == SI.E_COPIES)   # the element's sampled 20-mers
    assert n_e >= (SI.E_LEN - M.K + 1) // M.SAMPLE
    for cap in SI.CAPS:
        st = SM.index_stats(ref, cap)
        assert st["n_indexed"] == ref.n_sampled and st["occ_max"] == SI.poly_a_sampled() > 500
        assert st["n_distinct"] == len(ref.index)
    assert SM.index_stats(ref, 500)["n_over_cap"] == 1 and SM.index_stats(ref, 300)["n_over_cap"] == 1
    assert SM.index_stats(ref, 299)["n_over_cap"] == 1 + n_e and SM.index_stats(ref, 65535)["n_over_cap"] == 0
    assert SM.index_stats(ref, 1)["n_over_cap"] == sum(1 for v in ref.index.values() if len(v) > 1)


def hit(label, cap=500):
    return SI.repeat_expected(cap)[SI.repeat_queries()[1].index(label)]


def placed(h):
    return h["tid"], h["pos"], h["q_beg"], h["q_end"], h["score"], h["reverse"]


@pytest.mark.parametrize("strand", ["fwd", "rev"])
def test_hand_cases(strand):
    rev = int(strand == "rev")
    for a in (0, 30, 60):   # inside the element: the first copy, as good as any other, seeds left out
        h = hit(f"E60@{a}/{strand}")
        assert placed(h) == (E_TID, a, 0, 60, 60, rev) and (h["second"], h["mapq"], h["flags"], h["n_admitted"]) == (60, 0, SM.F_OVERFLOW, M.MAX_CAND)
    # part repeat, part unique, the repeat first in offset order or last: the unique seeds are admitted first and place the query at its own copy
    k0 = SI.e_copy_start(SI.E_COPY)
    h = hit(f"E36+spacer24/{strand}")
    assert placed(h) == (E_TID, k0 + SI.E_LEN - 36, 0, 60, 60, rev) and 36 <= h["second"] <= 50 and h["mapq"] == 60 and h["flags"] == SM.F_OVERFLOW
    h = hit(f"spacer24+E36/{strand}")
    assert placed(h) == (E_TID, k0 + SI.E_STRIDE - 24, 0, 60, 60, rev) and 36 <= h["second"] <= 50 and h["mapq"] == 60 and h["flags"] == SM.F_OVERFLOW
    h = hit(f"E20+spacer40/{strand}")   # the element's only whole 20-mer is not sampled: unique
    assert placed(h) == (E_TID, k0 + SI.E_LEN - 20, 0, 60, 60, rev) and (h["second"], h["flags"]) == (0, 0)
    # the diverged family: below the candidate limit, the MAPQ ladder is exact
    fam = [hit(f"F60-copy{k}/{strand}") for k in range(SI.F_COPIES)]
    assert all(h["tid"] == F_TID and h["score"] == 60 and h["flags"] == 0 and 0 < h["n_admitted"] < M.MAX_CAND for h in fam)
    assert {0, 30, 60} <= {h["mapq"] for h in fam}
    assert all(h["mapq"] == M.mapq_of(60, h["second"]) for h in fam)
    # poly-A: masked at 500
    h = hit(f"polyA60/{strand}")
    assert {k: h[k] for k in M.FIELDS} == M.UNALIGNED and h["flags"] == SM.F_MASKED and h["n_masked_kmers"] == 41
    h = hit(f"unique40+A20/{strand}")
    assert placed(h) == (0, 1000, 0, 40, 40, rev) and h["flags"] == SM.F_MASKED and h["mapq"] == 60
    h = hit(f"A20+unique40/{strand}")
    assert placed(h) == (2, 500, 20, 60, 40, rev) and h["flags"] == SM.F_MASKED
    for i in range(6):
        h = hit(f"random{i}/{strand}")
        assert {k: h[k] for k in M.FIELDS} == M.UNALIGNED and h["flags"] == 0
    # contig edges
    assert placed(hit(f"c35/{strand}")) == (C35_TID, 0, 0, 35, 35, rev)
    assert placed(hit(f"c35-and-neighbours/{strand}")) == (C35_TID, 0, 10, 45, 35, rev)
    assert hit(f"c19/{strand}")["tid"] == -1
    # lengths
    assert hit(f"len19/{strand}")["tid"] == -1 and hit(f"len1025/{strand}")["tid"] == -1 and hit(f"len20/{strand}")["tid"] == -1
    h = hit(f"len1024/{strand}")   # 251 seeds of one diagonal
    assert placed(h) == (SI.NAMES.index("r2"), 700, 0, 1024, 1024, rev) and h["flags"] == SM.F_OVERFLOW


def test_every_hit_is_a_true_alignment():
    ref = SI.repeat_model()
    for cap in (299, 500, 65535):
        for q, h in zip(SI.repeat_queries()[0], SI.repeat_expected(cap)):
            M.check_hit(ref.text, ref.off, q, h)


def test_cap_sweep():
    """the element has 300 copies: masked at 299, seeded at 300 and 500; poly-A is seeded only without a cap in its way"""
    for strand in ("fwd", "rev"):
        h = hit(f"E60@30/{strand}", 299)
        assert h["tid"] == -1 and h["flags"] == SM.F_MASKED
        assert {k: hit(f"E60@30/{strand}", 300)[k] for k in M.FIELDS + ("flags",)} == {k: hit(f"E60@30/{strand}", 500)[k] for k in M.FIELDS + ("flags",)}
        assert hit(f"E60@30/{strand}", 300)["tid"] == E_TID
        h = hit(f"E36+spacer24/{strand}", 299)   # still placed, by its unique seeds alone
        assert h["pos"] == SI.e_copy_start(SI.E_COPY) + SI.E_LEN - 36 and h["flags"] == SM.F_MASKED and h["second"] <= 50
        h = hit(f"polyA60/{strand}", 65535)
        assert (h["tid"], h["score"], h["second"], h["mapq"], h["flags"]) == (POLY_TID, 60, 60, 0, SM.F_OVERFLOW)
