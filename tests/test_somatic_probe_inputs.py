"""CPU: the hand-made samples of tests/somatic_probe_inputs.py.  Every pass's cluster table, built by the oracle from the sample's reads, is exactly the
listed clusters in the listed order; and the model (tests/somatic_probe_model.py) gives every probe the answer that is written out by hand beside it."""
import pytest

import oracle_lib
import somatic_probe_inputs as I
import somatic_probe_model as M

SAMPLES = I.samples()


@pytest.mark.parametrize("sample", SAMPLES, ids=[s.name for s in SAMPLES])
def test_oracle_tables_are_the_listed_clusters(sample):
    for clusters in sample.passes:
        got = M.table_clusters(oracle_lib.getclip([I.pass_batch(clusters)], 0.9, 1, False))
        assert got == [(c.tid, c.pos, c.side, c.left, c.right, c.support) for c in I.table_order(clusters)]


def test_oracle_cuts_the_passes_sample_where_the_contig_comes_back():
    s = I.passes_sample()
    recs = [r for clusters in s.passes for r in I.pass_records(clusters)]
    got = M.table_clusters(oracle_lib.getclip([I.records_to_batch(recs)], 0.9, 1, False))
    assert got == [(c.tid, c.pos, c.side, c.left, c.right, c.support) for clusters in s.passes for c in I.table_order(clusters)]


@pytest.mark.parametrize("sample", SAMPLES, ids=[s.name for s in SAMPLES])
def test_model_gives_the_hand_written_answers(sample):
    passes = [[(c.tid, c.pos, c.side, c.left, c.right, c.support) for c in I.table_order(clusters)] for clusters in sample.passes]
    names = [c.name for clusters in sample.passes for c in clusters]
    assert len(set(names)) == len(names)
    got = M.probe_passes([p for _, p, _ in sample.cases], passes, sample.rate, sample.min_len)
    for (label, _, want), g in zip(sample.cases, got):
        assert g == I.expected_hit(sample, want), (sample.name, label, g, want)
    assert any(want is None for _, _, want in sample.cases) and any(want is not None for _, _, want in sample.cases)


def test_anchor_offsets_are_what_the_labels_say():
    """the designed offsets: the ten bases are found where the label says, and nowhere before"""
    s = I.anchor_sample()
    by_name = {c.name: c for c in s.passes[0]}
    for label, p, want in s.cases:
        if " anchor at " not in label or "wrong" in label:
            continue
        word = label.split(" anchor at ")[1]
        c = by_name[want]
        s2, s4 = (p["b"], c.right) if p["mode"] == 2 else (c.right, p["b"])
        h = s4.find(s2[:10])
        assert h == (len(s4) - 10 if word == "the last offset" else int(word)), label
    e = by_name["E"].right
    assert e.find(e[:10]) == 0 and e.find(e[:10], 1) == 30


def test_every_listed_length_and_mode_is_there():
    s = I.lengths_sample()
    assert {len(c.left) for c in s.passes[0]} | {len(c.right) for c in s.passes[0]} >= set(I.LENGTHS)
    for n, k in I.MAX_MISMATCHES.items():  # the table's arithmetic: k substitutions reach 0.9, k + 1 do not
        assert (n - k) / n >= 0.9 > (n - k - 1) / n
    modes = {(p["mode"], want is not None) for smp in SAMPLES for _, p, want in smp.cases}
    assert modes == {(m, f) for m in (0, 1, 2) for f in (False, True)}
