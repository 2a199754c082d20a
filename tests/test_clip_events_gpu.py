"""-m gpu: the event stage of getclip - ssv_clip_scan_range through cluster_sort: k_build_ends, k_clip_scan_ends, k_cand_place, k_clip_filter,
k_clip_place, k_event_max, k_last_tid, k_gather_sizes, k_clip_gather, k_check_sorted, k_key_max, the windowed rank pass and its radix
fallback, k_side_bounds, k_merge_sides, k_concat_sides, k_gather_lines - against the per-record model of tests/clip_events_model.py on the
designed inputs of tests/clip_events_inputs.py.  Every input's every event is a cluster of its own, so the cluster table IS the event list in
table order: all keys of the ASCII table bit for bit, the event count after the scans, and under the compact format the strings of every
cluster.  The model is pinned by the oracle and by the real reference, and what each input reaches is asserted, in
tests/test_clip_events_inputs.py."""
import functools

import pytest

import clip_events_inputs as I
import clip_events_model as M
from seeksv_amd import host
from test_batch_forms_gpu import to_device
from test_hip_golden import assert_tables_equal

pytestmark = pytest.mark.gpu

GETCLIP = [n for n in I.names() if I.inputs()[n]["kind"] == "getclip"]
PASSES = [n for n in I.names() if I.inputs()[n]["kind"] == "passes"]
SCANNED = [n for n in I.names() if I.inputs()[n].get("scan_variants")]


@pytest.fixture(scope="module")
def ctx():
    from seeksv_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def strings_of(t):
    return [host.cluster_strings(t, k) for k in range(t["n_clusters"])]


@functools.lru_cache(maxsize=4)
def wanted(name, tag):
    t, per_pass = I.modelled(name, tag)
    return t, strings_of(t)


def compact(ctx, call):
    ctx.clip_table_format(3)
    try:
        return call()
    finally:
        ctx.clip_table_format(0)


def same_strings(d, strings, what):
    assert d["n_clusters"] == len(strings), what
    for k in range(d["n_clusters"]):
        assert host.cluster_strings(d, k) == strings[k], (what, k)


def one_pass(ctx, batches, ranges, want_events, **kw):
    """clip_begin / clip_scan_range / clip_event_count / clip_cluster, called directly -> the pass's table"""
    ctx.clip_begin(**kw)
    for b, (r0, r1) in zip(batches, ranges):
        ctx.clip_scan_range(b, r0, r1)
    assert ctx.clip_event_count() == want_events
    return ctx.clip_cluster()


@pytest.mark.parametrize("name", GETCLIP)
def test_event_list_equals_model(ctx, name):
    x = I.inputs()[name]
    opts = dict(own=x["own"], initial_last_tid=x["initial_last_tid"])
    for tag in x["runs"]:
        kw = dict(I.RUN_KW[tag], **opts)
        want, strings = wanted(name, tag)
        for cuts in [[]] + x["cutsets"]:
            batches = I.host_batches(name, tuple(cuts))
            assert_tables_equal(ctx.getclip(batches, **kw), want)
            same_strings(compact(ctx, lambda: ctx.getclip(batches, **kw)), strings, (tag, cuts))
            got = one_pass(ctx, batches, [(0, len(b["tid"])) for b in batches], want["n_events"], **kw)
            assert_tables_equal(got, want)


@pytest.mark.parametrize("name", PASSES)
def test_ranges_called_directly(ctx, name):
    x = I.inputs()[name]
    opts = dict(ship_all=x.get("ship_all", False), pad=x.get("pad", True))
    for tag in x["runs"]:
        whole, per_pass = I.modelled(name, tag)
        tables = []
        for p, (ev, scans) in zip(I.passes_of(x), per_pass):
            want = M.table(ev, scans)
            batches = [I.batch_of(recs, **opts) for recs, _ in scans]
            ranges = [rng for _, rng in scans]
            kw = dict(I.RUN_KW[tag], initial_last_tid=p["initial_last_tid"])
            got = one_pass(ctx, batches, ranges, len(ev), **kw)
            assert_tables_equal(got, want)
            same_strings(compact(ctx, lambda: one_pass(ctx, batches, ranges, len(ev), **kw)), strings_of(want), (tag, ranges))
            tables.append(got)
        assert_tables_equal(host.concat_tables(tables) if len(tables) > 1 else tables[0], whole)


@pytest.mark.parametrize("variant", ["no-ends", "blocks-1", "blocks-2"])
@pytest.mark.parametrize("name", SCANNED)
def test_scan_variants(ctx, monkeypatch, name, variant):
    """tile_edges and candidate_counts again: without the cigar_ends column (k_build_ends writes it), and with one and two workgroups for the
    whole scan - with two, the five-tile input gives a workgroup three rounds: both LDS parities, and a prefetch that ends on the partial tile"""
    x = I.inputs()[name]
    if variant != "no-ends":
        monkeypatch.setenv("SSV_CLIP_SCAN_BLOCKS", variant[-1])
    for tag in x["runs"]:
        want, _ = I.modelled(name, tag)
        for cuts in [[]] + x["cutsets"]:
            batches = I.host_batches(name, tuple(cuts), variant != "no-ends")
            assert_tables_equal(ctx.getclip(batches, **I.RUN_KW[tag]), want)


@pytest.mark.parametrize("name", I.FORMS)
def test_batch_forms(ctx, name):
    """host arrays, device columns, and the retained copy (persistent: its events point into the batch, k_clip_gather does not run) give one table"""
    x = I.inputs()[name]
    opts = dict(own=x["own"], initial_last_tid=x["initial_last_tid"])
    for tag in x["runs"]:
        kw = dict(I.RUN_KW[tag], **opts)
        want, strings = wanted(name, tag)
        for cuts in [[]] + x["cutsets"][:1]:
            hosts = I.host_batches(name, tuple(cuts))
            runs, last = [], x["initial_last_tid"]
            for b in hosts:
                runs.append(host.host_tid_runs(b, last))
                last = runs[-1][-1][1] if runs[-1] else last
            assert_tables_equal(ctx.getclip(hosts, **kw), want)
            devs = [to_device(b) for b in hosts]
            assert_tables_equal(ctx.getclip([d for d, _ in devs], tid_runs=runs, **kw), want)
            kept = []
            try:
                for d, _ in devs:
                    kept.append(ctx.batch_retain(d))
                assert_tables_equal(ctx.getclip(kept, tid_runs=runs, **kw), want)
                same_strings(compact(ctx, lambda: ctx.getclip(kept, tid_runs=runs, **kw)), strings, (tag, "retained"))
            finally:
                for k in kept:
                    ctx.batch_release(k)
