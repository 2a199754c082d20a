"""CPU: the inputs of tests/pileup_cap_inputs.py through the oracle, against what the REAL reference wrote for them
(tests/golden/pileup_cap/reference.json, made by tests/golden/make_pileup_cap_reference.py) and against the plain per-read model of
tests/pileup_cap_model.py; and every input really has the property tests/test_pileup_cap_differential_gpu.py relies on - an input that
stopped reaching its branch would leave the GPU test green and empty."""
import json
import os

import numpy as np
import pytest

import golden_util as G
import oracle_lib as O
import pileup_cap_inputs as P
import pileup_cap_model as M
from seeksv_amd import host
from test_oracle_golden import OracleBackend

QS = (20, 0)
LOOKBACK, RING = 7998, 8192     # CAP_LOOKBACK, CAP_LDS_RING (getsv_kernels.h)


def reference_outputs():
    with open(os.path.join(G.GOLDEN, "pileup_cap", "reference.json")) as f:
        return json.load(f)


def stack_windows(c):
    """one window over each stack's columns and the 200 behind them (1-based, merged)"""
    iv = sorted((tid, max(1, pos - 150), min(c.lens[tid], pos + 300)) for tid, pos in c.stacks)
    out = []
    for t, a, b in iv:
        if out and out[-1][0] == t and a <= out[-1][2] + 1:
            out[-1] = (t, out[-1][1], max(b, out[-1][2]))
        else:
            out.append((t, a, b))
    return out


def deep_tiles(c, q=20):
    """the 4096-record tiles that hold a "deep" record when the file is one batch (k_cap_mark's rule)"""
    tid = np.array([r["tid"] for r in c.recs])
    pos = np.array([r["pos"] for r in c.recs])
    span = max(M.ref_span(r["cigar"]) for r in c.recs)
    deep = np.zeros(len(tid), bool)
    deep[LOOKBACK:] = (tid[LOOKBACK:] >= 0) & (tid[LOOKBACK:] == tid[:-LOOKBACK]) & (pos[LOOKBACK:] - pos[:-LOOKBACK] <= span)
    return sorted(set((np.flatnonzero(deep) // P.TILE).tolist()))


def test_case_list_is_stable():
    assert len(P.CASES) == len(set(P.CASES)) == 34 and sorted(reference_outputs()) == sorted(P.CASES)
    assert all(len(P.case(n).recs) <= 40000 for n in P.ALL_CASES)


@pytest.mark.parametrize("name", P.ALL_CASES)
def test_oracle_and_model_against_the_reference(tmp_path, name):
    c = P.case(name)
    want = reference_outputs().get(name)
    assert (want is None) == (name in P.UNPINNED)     # (a case that the reference cannot run: the model and the oracle only)
    bam = str(tmp_path / "c.bam")
    P.write_bam(bam, c)
    names, lens, batches = host.read_bam(bam)
    assert names == c.names and sum(len(b["tid"]) for b in batches) == len(c.recs)
    wins = stack_windows(c)
    windows = np.array(wins, dtype=[("tid", np.int32), ("beg", np.int32), ("end", np.int32)])
    points = np.array([(t, col, col) for t, a, b in wins for col in range(a, b + 1)], dtype=windows.dtype)
    n_dropped = {}
    for q in QS:
        # (a) the oracle's tables are the reference's, seven values per junction
        if want is not None:
            sv, so = str(tmp_path / f"{q}.sv"), str(tmp_path / f"{q}.stdout")
            with open(sv, "w") as f:
                f.write(want[str(q)]["sv"])
            with open(so, "w") as f:
                f.write(want[str(q)]["stdout"])
            stats, junctions, folded = G.run_getsv_case(bam, c.rows, OracleBackend(), min_mapq=q)
            golden = G.parse_sv_outputs(sv, so)
            assert sum(len(v) for v in golden.values()) == len(junctions)
            assert G.check_getsv_against_golden(junctions, folded, golden) == 7 * len(junctions)
        # (b) the model's dropped reads give the oracle's depth at every column over the stacks
        trace = []
        dropped = M.dropped_reads(c.recs, q, trace=trace)
        rs, pd, mx = O.depth(batches, windows, windows[:0], points, q)
        model = np.concatenate([M.depth(c.recs, dropped, q, t, a, b) for t, a, b in wins])
        assert np.array_equal(pd, model), (name, q, np.flatnonzero(pd != model)[:5])
        n_dropped[q] = len(dropped)
        # (c) the case has its property
        kind = P.KIND[name]
        assert (len(dropped) == 0) == (kind == "control")
        if kind == "spanless_first":
            assert M.dropped_reads(c.recs, q, parent_rule=True) != dropped
        elif not name.startswith("random") and not (name == "filtered_mapq" and q == 0):
            assert M.dropped_reads(c.recs, q, parent_rule=True) == dropped      # (the other named cases do not depend on that rule)
        live = dict(trace)
        if name.startswith("fill_"):
            s = c.first_index(0, 5001)
            assert live[s] + 0 == int(name[5:]) - sum(1 for r in c.recs[:s] if r["pos"] + M.ref_span(r["cigar"]) == 5000 and M.passes(r, q))
            before = [i for i, _ in trace if i < s][-1]
            assert live[before] + 1 == int(name[5:])            # the stack's last read made it `target`, and it was taken
            assert before not in dropped
    if name == "jump_in_sweep":
        keep = [i for i, r in enumerate(c.recs) if M.passes(r, 20)]
        gaps = [(c.recs[b]["pos"] - c.recs[a]["pos"], b) for a, b in zip(keep, keep[1:])]
        gap, at = max(gaps)
        tiles = deep_tiles(c)
        assert gap > RING and any(abs(at // P.TILE - t) <= 2 for t in tiles) and min(tiles) <= at // P.TILE <= max(tiles)
    if name.startswith("ring_"):
        i = next(i for i, r in enumerate(c.recs) if r.get("tag") == "long")
        assert M.ref_span(c.recs[i]["cigar"]) > RING
        s = c.first_index(*c.stacks[-1])
        assert (i < 1000) == (name == "ring_global_first_batch") and i < s and c.recs[i]["pos"] + M.ref_span(c.recs[i]["cigar"]) > c.stacks[-1][1] + 100
        if name == "ring_regrow_later_batch":
            assert i > 8192 and i // P.TILE in deep_tiles(c) or any(abs(i // P.TILE - t) <= 2 for t in deep_tiles(c))
    if name.startswith("filtered_"):
        tags = {}
        for i, r in enumerate(c.recs):
            if "tag" in r:
                assert not M.passes(r, 20)
                tags.setdefault(r["tag"], []).append(i)
        assert len(tags["first_at_start"]) == 6 and len(tags["chunk"]) >= 5 and len(tags["tile"]) >= 2
        place = lambda r: r.get("place", (r["tid"], r["pos"]))
        assert all(place(c.recs[i - 1]) != place(c.recs[i]) == place(c.recs[i + 1]) for i in tags["first_at_start"])
        assert all(i % P.CHUNK == 0 for i in tags["chunk"]) and all(i % P.TILE == 0 for i in tags["tile"])
    if name.startswith("two_stacks"):
        tiles = deep_tiles(c)
        first = [t for t in tiles if t * P.TILE < c.first_index(0, 14000)]
        second = [t for t in tiles if t not in first]
        # three apart: the sweep reaches the second stack's tile with since_deep == 2; six apart: it ends, and a new one starts from the tail
        assert (second[0] - first[-1] == 3) if name.endswith("three_tiles") else (second[0] - first[-1] >= 6)
    if name == "spanless_in_group_of_130":
        i = next(i for i, r in enumerate(c.recs) if r["pos"] == 5001 and r["cigar"] == "100S")
        a = c.first_index(0, 5001)
        assert a // P.CHUNK < i // P.CHUNK or (a + 129) // P.CHUNK > i // P.CHUNK      # the group crosses a chunk
        assert a // P.CHUNK != (a + 129) // P.CHUNK
    if name == "contig_change":
        assert c.recs[c.first_index(1, 0) - 1]["pos"] == max(r["pos"] for r in c.recs if r["tid"] == 0)
    if name == "filtered_mapq":
        assert n_dropped[0] != n_dropped[20]
