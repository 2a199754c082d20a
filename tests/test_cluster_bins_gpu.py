"""-m gpu: the consensus clustering walk (k_cluster_bins4 / k_cluster_bins, the bin lists before them, the multi-event side of the pack
kernels behind them) against the plain-Python model of tests/cluster_bins_model.py on the designed samples of tests/cluster_bins_inputs.py:
every match rate of a sample's family, the whole sample and the sample cut inside a deep bin and inside a many-cluster bin, the ASCII table
with all its keys, and the compact table's strings of every cluster.  The model itself is pinned by the oracle and by the real reference in
tests/test_cluster_bins_model.py; what each sample reaches is asserted in tests/test_cluster_bins_inputs.py."""
import pytest

import cluster_bins_inputs as I
from seeksv_amd import host
from test_hip_golden import assert_tables_equal
from test_oracle_golden import split_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from seeksv_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("family,cls", I.SAMPLE_IDS, ids=[f"{f}-{c}" for f, c in I.SAMPLE_IDS])
def test_clustering_walk_equals_model(ctx, family, cls):
    s = I.sample(family, cls)
    b = s["batch"]
    cuts = I.cuts_of(family, cls)
    parts = [split_batch(b, cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]
    for tag, _, kw in I.runs_of(family):
        want, bins, recs = I.modelled(family, cls, tag)
        strings = [host.cluster_strings(want, k) for k in range(want["n_clusters"])]
        for how, batches in (("whole", [b]), ("parts", parts)):
            assert_tables_equal(ctx.getclip(batches, **kw), want)
            ctx.clip_table_format(3)
            try:
                d = ctx.getclip(batches, **kw)
            finally:
                ctx.clip_table_format(0)
            assert d["n_clusters"] == want["n_clusters"], (tag, how)
            for k in range(d["n_clusters"]):
                assert host.cluster_strings(d, k) == strings[k], (tag, how, k)
