"""-m gpu: the fused getsv pass on the hand-made geometry of tests/getsv_window_inputs.py - ssv_getsv_begin / _scan / _finish called directly, ALL FOUR
outputs (discordant counts, range sums, point depths, max_depth) against the oracle, which tests/test_getsv_window_inputs.py pins with a second plain
model on the CPU.  Integers: equal, no tolerance.  Every case with -q 20 and 0; as one batch and cut into three parts at random records; with the
reference span stated and with max_ref_span = 0 in every part (k_max_span measures it: the same answers); with the batch's tid runs and without
(SSV_NO_TID_RUNS: k_getsv_scan_runs / k_getsv_scan) where the batch is a scan tile or more; and the cases with ONE long read cut so that the first
parts state a short span and a later one the long one - the tile map is built again, over hand-made windows, while records are streaming."""
import zlib

import numpy as np
import pytest

import getsv_window_inputs as W
import oracle_lib as O
from test_oracle_golden import split_batch

pytestmark = pytest.mark.gpu
QS = (20, 0)
LABELS = ("counts", "range sums", "point depths", "max_depth")


@pytest.fixture(scope="module")
def ctx():
    from seeksv_amd.device import Context
    c = Context(0)
    yield c
    c.close()


_want = {}


def want(name, q):
    """what the oracle computes for the case: once, shared"""
    if (name, q) not in _want:
        names, lens, b, j, w, r, p, mean, sd = W.case(name)
        _want[name, q] = (O.discordant([b], j, mean, sd, 4, q),) + O.depth([b], w, r, p, q)
    return _want[name, q]


def cut(b, cuts, span):
    """the batch cut at the record indices `cuts`.  span: "whole" - every part states the whole stream's longest reference span (split_batch);
    "own" - its own, as a reader's batches do; "unknown" - 0, and the library measures it"""
    n = len(b["tid"])
    edges = [0] + sorted(set(k for k in cuts if 0 < k < n)) + [n]
    spans = W.ref_spans(b)
    parts = []
    for lo, hi in zip(edges, edges[1:]):
        part = split_batch(b, lo, hi)
        if span == "own": part["max_ref_span"] = int(spans[lo:hi].max())
        elif span == "unknown": part["max_ref_span"] = 0
        parts.append(part)
    return parts


def run(ctx, parts, case, q):
    names, lens, b, j, w, r, p, mean, sd = case
    ctx.getsv_begin(j, w, mean, sd, np.array(lens, np.int32), 4, q, q)
    for part in parts:
        ctx.getsv_scan(part)
    return ctx.getsv_finish(r, p)


def assert_four(got, wanted, what):
    assert len(got) == len(wanted) == 4
    for k, label in enumerate(LABELS):
        if k < 3:
            assert got[k].dtype == wanted[k].dtype and np.array_equal(got[k], wanted[k]), (what, label, np.flatnonzero(got[k] != wanted[k])[:8])
        else:
            assert got[k] == wanted[k], (what, label, got[k], wanted[k])


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("name", W.CASES)
def test_hand_made_windows_hip_equals_oracle(ctx, monkeypatch, name, q):
    case = W.case(name)
    b = case[2]
    n = len(b["tid"])
    wanted = want(name, q)
    rng = np.random.RandomState(zlib.crc32(name.encode()) + q)
    streams = [("one batch", [], "whole"), ("one batch", [], "unknown")]
    three = [int(x) for x in rng.randint(1, n, 2)]
    streams += [(f"cut at {three}", three, "whole"), (f"cut at {three}", three, "unknown")]
    if name in W.ONE_LONG:
        # the parts before the long read state a short span, the part that holds it the long one: the tile map is rebuilt mid-stream
        i = int(np.argmax(W.ref_spans(b)))
        at = [int(rng.randint(W.CS_TILE, i - 100)), i - int(rng.randint(0, 100))]
        parts = cut(b, at, "own")
        assert parts[0]["max_ref_span"] <= 450 and parts[1]["max_ref_span"] <= 450 and parts[2]["max_ref_span"] > 9000
        streams.append((f"a short span first, cut at {at}", at, "own"))
    for no_runs in ((False, True) if n >= W.CS_TILE else (False,)):
        if no_runs: monkeypatch.setenv("SSV_NO_TID_RUNS", "1")
        else: monkeypatch.delenv("SSV_NO_TID_RUNS", raising=False)
        for what, cuts, span in streams:
            got = run(ctx, cut(b, cuts, span), case, q)
            assert_four(got, wanted, (name, q, what, "span " + span, "no tid runs" if no_runs else "tid runs"))
    monkeypatch.delenv("SSV_NO_TID_RUNS", raising=False)
