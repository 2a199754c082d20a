"""CPU: the plain-Python model of the clustering walk (tests/cluster_bins_model.py) against the C oracle on every designed sample and every
match rate - all keys of the table, none exempt - and against the REAL reference on the part of the samples that it defines: the sha256 of
its clip / clip.fq texts lie in tests/golden/cluster_bins/reference.json (made by tests/golden/make_cluster_bins_reference.py with
oracle/_ref/seeksv_ref; no reference binary is needed here).  tests/test_cluster_bins_gpu.py then holds the kernels to this model."""
import hashlib
import json
import os

import pytest

import cluster_bins_inputs as I
import golden_util as G
import oracle_lib as O
from seeksv_amd import host
from test_hip_golden import assert_tables_equal

IDS = [f"{f}-{c}" for f, c in I.SAMPLE_IDS]


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


@pytest.fixture(scope="module")
def reference():
    with open(os.path.join(G.GOLDEN, "cluster_bins", "reference.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("family,cls", I.SAMPLE_IDS, ids=IDS)
def test_model_equals_oracle(family, cls):
    s = I.sample(family, cls)
    for tag, _, kw in I.runs_of(family):
        t, bins, recs = I.modelled(family, cls, tag)
        assert_tables_equal(t, O.getclip([s["batch"]], **kw))
        assert sum(b["n_events"] for b in bins) == t["n_events"] and sum(b["n_clusters"] for b in bins) == t["n_clusters"]
        assert all(max(b["assign"]) == b["n_clusters"] - 1 for b in bins)


@pytest.mark.parametrize("family,cls", I.SAMPLE_IDS, ids=IDS)
def test_model_equals_reference(reference, family, cls):
    """everything but the records marked ref=False: no qualities, and lone soft clips inside bins of several reads (the reference reads outside
    its strings there)"""
    s = I.sample(family, cls)
    want = reference[s["name"]]
    assert sorted(want) == sorted(r[0] for r in I.runs_of(family))
    for tag, _, kw in I.runs_of(family):
        t, bins, recs = I.modelled(family, cls, tag, True)
        clip, fq = host.format_clip_outputs(t, s["names"])
        assert sha(clip) == want[tag]["clip"], tag
        assert sha(fq) == want[tag]["fq"], tag
        assert t["n_clusters"] == want[tag]["rows"]
