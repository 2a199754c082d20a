"""GPU: the somatic look-ups on the device-side cluster table (k_somatic_probe behind ssv_clip_cluster; Context.clip_probe_set / clip_probe_get) against the
plain-Python model (tests/somatic_probe_model.py): the hand-made samples of tests/somatic_probe_inputs.py cut into passes as listed there - support, pos, pass
and cluster of every probe -, the argument errors, the probes' lifetime, and 2,000 probes derived from a synthetic sample's own clusters."""
import ctypes as C

import numpy as np
import pytest

import somatic_probe_inputs as I
import somatic_probe_model as M
from seeksv_amd import _abi, synth
from seeksv_amd.device import Context, SeeksvError

pytestmark = pytest.mark.gpu
SAMPLES = I.samples()
SYNTH_FULL = dict(genome_frac=1 / 8192, depth=40, n_sv=24)
TABLE_COLUMNS = ("tid", "pos", "side", "support", "left_len", "right_len", "str_off", "str", "cigar_off", "n_cigar", "cigar", "qual_missing")


def _hits(h):
    return [(int(x["support"]), int(x["pos"]), int(x["pass"]), int(x["cluster"])) for x in h]


def _run_passes(ctx, sample):
    """one clip pass per listed pass, with the sample's probes set -> (hits, passes, the passes' tables)"""
    ctx.clip_table_format(0)
    ctx.clip_probe_set([p for _, p, _ in sample.cases], sample.rate, sample.min_len)
    tables = []
    for clusters in sample.passes:
        ctx.clip_begin(0.9, 1, False)
        ctx.clip_scan(I.pass_batch(clusters))
        tables.append(ctx.clip_cluster())
    hits, passes = ctx.clip_probe_get()
    ctx.clip_probe_set([])
    return hits, passes, tables


@pytest.mark.parametrize("sample", SAMPLES, ids=[s.name for s in SAMPLES])
def test_hand_made_samples_equal_model_and_hand_written_answers(sample):
    with Context(0) as ctx:
        hits, passes, tables = _run_passes(ctx, sample)
    assert passes == len(sample.passes)
    listed = [M.table_clusters(t) for t in tables]
    assert listed == [[(c.tid, c.pos, c.side, c.left, c.right, c.support) for c in I.table_order(clusters)] for clusters in sample.passes]
    model = M.probe_passes([p for _, p, _ in sample.cases], listed, sample.rate, sample.min_len)
    got = _hits(hits)
    for (label, _, want), g, m in zip(sample.cases, got, model):
        assert g == m == I.expected_hit(sample, want), (sample.name, label, g, m, want)


def test_passes_cut_by_getclip_where_the_contig_comes_back():
    s = I.passes_sample()
    recs = [r for clusters in s.passes for r in I.pass_records(clusters)]
    with Context(0) as ctx:
        ctx.clip_table_format(0)
        ctx.clip_probe_set([p for _, p, _ in s.cases], s.rate, s.min_len)
        ctx.getclip([I.records_to_batch(recs)])
        hits, passes = ctx.clip_probe_get()
    assert passes == 2
    assert _hits(hits) == [I.expected_hit(s, want) for _, _, want in s.cases]


def test_argument_errors_change_nothing():
    s = I.rates_sample()
    lib = _abi.hip_lib()
    with Context(0) as ctx:
        ctx.clip_table_format(0)
        ctx.clip_probe_set([p for _, p, _ in s.cases], s.rate, s.min_len)
        text = (C.c_char * 8)(*b"ACGTACGT")
        one = np.zeros(1, dtype=_abi.CLIP_PROBE_DTYPE)

        def refused(**kw):
            p = one.copy()
            p[0] = (0, 10, 10, ord("5"), 0, (0, 0), 0, 4, 4, 4)
            for k, v in kw.items():
                p[k] = v
            return lib.ssv_clip_probe_set(ctx._h, p.ctypes.data, 1, C.addressof(text), 8, 0.9, 10)
        assert refused() == 0
        # (the accepted set above replaced the sample's probes: set them again, then every refusal must leave them alone)
        ctx.clip_probe_set([p for _, p, _ in s.cases], s.rate, s.min_len)
        bad = [refused(side=ord("4")), refused(side=0), refused(mode=3), refused(a_off=5), refused(b_len=5), refused(a_len=0xffffffff),
               lib.ssv_clip_probe_set(ctx._h, None, 1, C.addressof(text), 8, 0.9, 10), lib.ssv_clip_probe_set(ctx._h, one.ctypes.data, 1, None, 8, 0.9, 10)]
        assert all(rc != 0 for rc in bad), bad
        assert all(rc == bad[0] for rc in bad)
        with pytest.raises(SeeksvError):
            ctx.clip_probe_set([dict(tid=0, lo=1, hi=1, side="4", mode=0, a="A", b="C")])
        for clusters in s.passes:
            ctx.clip_begin(0.9, 1, False)
            ctx.clip_scan(I.pass_batch(clusters))
            ctx.clip_cluster()
        hits, passes = ctx.clip_probe_get()
        assert passes == 1 and _hits(hits) == [I.expected_hit(s, want) for _, _, want in s.cases]


def test_format_3_is_refused_while_probes_are_set():
    s = I.rates_sample()
    with Context(0) as ctx:
        ctx.clip_table_format(3)
        ctx.clip_probe_set([p for _, p, _ in s.cases], s.rate, s.min_len)
        ctx.clip_begin(0.9, 1, False)
        ctx.clip_scan(I.pass_batch(s.passes[0]))
        with pytest.raises(SeeksvError, match="format"):
            ctx.clip_cluster()
        ctx.clip_probe_set([])
        t = ctx.clip_cluster()  # without probes the compact table is built as ever
        assert t["n_clusters"] == 1


def test_empty_set_clears_and_tables_are_untouched():
    s = I.walk_sample()
    batch = I.pass_batch(s.passes[0])
    with Context(0) as plain:
        plain.clip_table_format(0)
        plain.clip_begin(0.9, 1, False)
        plain.clip_scan(batch)
        want = plain.clip_cluster()
    with Context(0) as ctx:
        hits, passes, tables = _run_passes(ctx, s)     # probes set, then cleared with an empty set
        assert passes == 1 and sum(1 for h in _hits(hits) if h[0]) > 5
        ctx.clip_begin(0.9, 1, False)
        ctx.clip_scan(batch)
        after = ctx.clip_cluster()
        hits2, passes2 = ctx.clip_probe_get()
        assert len(hits2) == 0 and passes2 == 0
    for t in (tables[0], after):                       # with probes set and with none: the table of a context that never had probes
        assert t["n_clusters"] == want["n_clusters"] > 10
        for k in TABLE_COLUMNS:
            assert np.array_equal(t[k], want[k]), k


def test_probes_survive_clip_begin_and_the_next_set_starts_over():
    s = I.passes_sample()
    with Context(0) as ctx:
        ctx.clip_table_format(0)
        ctx.clip_probe_set([p for _, p, _ in s.cases], s.rate, s.min_len)
        ctx.clip_begin(0.9, 1, False)
        ctx.clip_begin(0.9, 1, False)                  # two begins, no pass clustered yet
        hits, passes = ctx.clip_probe_get()
        assert passes == 0 and not any(h[0] for h in _hits(hits))
        for clusters in s.passes:
            ctx.clip_begin(0.9, 1, False)
            ctx.clip_scan(I.pass_batch(clusters))
            ctx.clip_cluster()
        hits, passes = ctx.clip_probe_get()
        assert passes == 2 and _hits(hits) == [I.expected_hit(s, want) for _, _, want in s.cases]
        # the next set zeroes the hits and the pass count: the later pass alone now
        ctx.clip_probe_set([p for _, p, _ in s.cases], s.rate, s.min_len)
        ctx.clip_begin(0.9, 1, False)
        ctx.clip_scan(I.pass_batch(s.passes[1]))
        ctx.clip_cluster()
        hits, passes = ctx.clip_probe_get()
        alone = M.probe_passes([p for _, p, _ in s.cases], [[(c.tid, c.pos, c.side, c.left, c.right, c.support) for c in I.table_order(s.passes[1])]], s.rate, s.min_len)
        assert passes == 1 and _hits(hits) == alone


def _derived_probes(clusters, rng, n):
    """probes made of a table's own clusters: the strings intact, with 1 .. 15 substitutions, truncated, on the neighbouring position, in all three modes"""
    out = []
    while len(out) < n:
        tid, pos, side, left, right, _ = clusters[rng.randint(len(clusters))]
        a, b = left, right
        kind = rng.randint(5)
        if kind == 1:
            for s_ in range(rng.randint(1, 16)):
                which = rng.randint(2)
                t = list(b if which else a)
                if t:
                    i = rng.randint(len(t))
                    t[i] = "ACGT"[("ACGT".find(t[i]) + 1 + rng.randint(3)) % 4]
                    if which:
                        b = "".join(t)
                    else:
                        a = "".join(t)
        elif kind == 2:
            a, b = a[rng.randint(len(a) + 1):], b[:rng.randint(len(b) + 1)]
        elif kind == 3:
            pos += int(rng.choice([-1, 1]))
        mode = rng.randint(3)
        if mode and kind == 4:  # the junction moved by a few bases, as the anchored modes exist for
            cut = rng.randint(0, 8)
            a, b = (left + right)[:max(0, len(left) - cut)], (left + right)[max(0, len(left) - cut):]
        w = int(rng.randint(0, 40))
        lo, hi = (pos, pos) if mode == 0 else (pos - int(rng.randint(0, w + 1)), pos + int(rng.randint(0, w + 1)))
        out.append(dict(tid=tid if rng.randint(50) else -1, lo=lo, hi=hi, side=side if rng.randint(20) else "35"[side == "3"], mode=int(mode), a=a, b=b))
    return out


@pytest.mark.parametrize("rate,min_len", [(0.9, 10), (0.5, 60)])
def test_randomised_probes_on_synthetic_sample(rate, min_len):
    w = synth.Workload(**SYNTH_FULL)
    b = w.generate_host(0, w.n_total)
    with Context(0) as ctx:
        ctx.clip_table_format(0)
        ctx.clip_begin(0.9, 1, False)
        ctx.clip_scan(b)
        clusters = M.table_clusters(ctx.clip_cluster())
        probes = _derived_probes(clusters, np.random.RandomState(11), 2000)
        ctx.clip_probe_set(probes, rate, min_len)
        ctx.clip_begin(0.9, 1, False)
        ctx.clip_scan(b)
        ctx.clip_cluster()
        hits, passes = ctx.clip_probe_get()
    model = M.probe_passes(probes, [clusters], rate, min_len)
    got = _hits(hits)
    assert passes == 1 and len(got) == 2000
    wrong = [(k, probes[k]["mode"], g, m) for k, (g, m) in enumerate(zip(got, model)) if g != m]
    assert not wrong, wrong[:5]
    found = [m for m in model if m[0]]
    assert 200 < len(found) < 1900 and {probes[k]["mode"] for k, m in enumerate(model) if m[0]} == {0, 1, 2}
