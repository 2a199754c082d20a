"""CPU: the plain-Python model of `somatic`'s look-ups (tests/somatic_probe_model.py) against the REAL reference's output - the counts in columns 24-25 of
tests/golden/somatic/somatic*.sv (the 227-row branch-coverage table on the synthetic normal) and of tests/golden/example/cancer.somatic.temp.sv - with the
normal's clusters from the oracle's getclip, as tests/test_somatic_stage.py builds them.  And the host half of the same case analysis: the -J dump with the
look-ups sent through build_cluster_probes (SSV_SOMATIC_PROBES=host) equals the plain dump."""
import gzip
import os
import subprocess

import pytest

import golden_util as G
import oracle_lib
import somatic_probe_model as M
from seeksv_amd import host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
SYNTH_FULL = dict(genome_frac=1 / 8192, depth=40, n_sv=24)
VARIANTS = (("", {}), (".l0", dict(offset=0)), (".l60", dict(offset=60)), (".t05", dict(rate=0.5)), (".m60", dict(min_clipped_len=60)))
FLAGS = {"": [], ".l0": ["-l", "0"], ".l60": ["-l", "60"], ".t05": ["-t", "0.5"], ".m60": ["-m", "60"]}


@pytest.fixture(scope="module")
def synth_normal():
    w = synth.Workload(**SYNTH_FULL)
    b = w.generate_host(0, w.n_total)
    table = oracle_lib.getclip([b], 0.9, 1, False)
    return w, table


def _expected_counts(text):
    return [(int(c[23]), int(c[24])) for c in (l.split("\t") for l in text.splitlines()[1:])]


@pytest.mark.parametrize("tag,kw", VARIANTS, ids=[v[0] or "default" for v in VARIANTS])
def test_model_counts_equal_reference_on_branch_table(synth_normal, tag, kw):
    w, table = synth_normal
    rows = M.parse_tumor_rows(G.read_text("somatic", "tumor.sv"))
    got = M.somatic_counts(rows, list(w.names), [M.table_clusters(table)], **kw)
    exp = _expected_counts(G.read_text("somatic", f"somatic{tag}.sv"))
    assert len(got) == len(exp) == 198
    assert got == exp
    assert sum(1 for a, b in exp if a or b) > 20, "the table's look-ups never found anything"


def test_model_counts_equal_reference_on_example():
    names, lens, batches = host.read_bam(os.path.join(G.GOLDEN, "example", "normal.sort.bam"))
    table = oracle_lib.getclip(batches, 0.9, 1, False)
    rows = M.parse_tumor_rows(G.read_text("example", "cancer.sv"))
    got = M.somatic_counts(rows, list(names), [M.table_clusters(table)])
    exp = _expected_counts(G.read_text("example", "cancer.somatic.temp.sv"))
    assert len(exp) > 0 and got == exp


def test_dump_through_host_probes_equals_plain_dump(synth_normal, tmp_path):
    if not os.path.exists(SEEKSV):
        subprocess.check_call(["make", "-C", ROOT, "cli"], stdout=subprocess.DEVNULL)
    w, table = synth_normal
    rows, _ = host.format_clip_outputs(table, w.names)
    clip = str(tmp_path / "normal.clip.gz")
    with gzip.open(clip, "wt") as f:
        f.write(rows)
    tumor = os.path.join(G.GOLDEN, "somatic", "tumor.sv")
    for tag, flags in FLAGS.items():
        out = {}
        for how in ("plain", "host"):
            dump = str(tmp_path / f"dump{tag}.{how}")
            env = dict(os.environ)
            env.pop("SSV_SOMATIC_PROBES", None)
            if how == "host":
                env["SSV_SOMATIC_PROBES"] = "host"
            r = subprocess.run([SEEKSV, "somatic", "-J", dump] + flags + ["unused.bam", clip, tumor, "unused.out"], capture_output=True, text=True, env=env)
            assert r.returncode == 0, r.stderr
            out[how] = (open(dump).read(), r.stderr)
        assert out["host"] == out["plain"], tag
        assert len(out["plain"][0].splitlines()) == 199
