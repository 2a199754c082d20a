"""-m gpu: `seeksv somatic -N n` - the discordant tally over the normal BAM cut into n runs of records, one rank per run (the ranks share the GPU of a
one-GPU box and exchange through host memory; between different GPUs it is one RCCL all-gather), the insert-size pass on rank 0: table and stderr must
be what `seeksv somatic` on one GPU writes, i.e. the reference's."""
import os
import subprocess
import sys

import pytest

import golden_util as G
import test_cli_gpu as T

pytestmark = pytest.mark.gpu

SEEKSV = T.SEEKSV


@pytest.fixture(autouse=True, params=["host-inflate", "device-inflate"])
def inflate(request):
    """every case twice: the ranks' runs inflated and decoded by the host threads, and on the ranks' GPUs (-Z)"""
    return [] if request.param == "host-inflate" else ["-Z"]


def _somatic(args, env=None):
    return subprocess.run([SEEKSV, "somatic"] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("tag,flags", [("", []), (".q0", ["-q", "0"]), (".n0", ["-n", "0"])], ids=["default", "q0", "n0"])
def test_somatic_ranks_virus_integration(tmp_path_factory, tmp_path, inflate, tag, flags, n):
    """BASELINE config 5 in small: the tumor's table against the patient's normal sample, the normal's BAM pass over n ranks"""
    bam, clip_gz, _ = T._synth_sample(tmp_path_factory, "hbvnormal", T.HBV_NORMAL)
    out = str(tmp_path / "somatic.sv")
    r = _somatic(inflate + ["-N", str(n)] + flags + [bam, clip_gz, os.path.join(G.GOLDEN, "synth", "hbvfull.loose.sv"), out])
    assert r.returncode == 0, r.stderr
    assert open(out).read() == G.read_text("somatic", f"hbv.somatic{tag}.sv")
    assert T._somatic_stderr(r.stderr) == T._somatic_stderr(G.read_text("somatic", f"hbv.somatic{tag}.stderr"))


def test_somatic_ranks_example(tmp_path, inflate):
    ex = os.path.join(G.GOLDEN, "example")
    pre = str(tmp_path / "normal")
    r = subprocess.run([SEEKSV, "getclip", "-o", pre, os.path.join(ex, "normal.sort.bam")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = str(tmp_path / "somatic.sv")
    r = _somatic(inflate + ["-N", "2", os.path.join(ex, "normal.sort.bam"), pre + ".clip.gz", os.path.join(ex, "cancer.sv"), out])
    assert r.returncode == 0, r.stderr
    assert open(out).read() == G.read_text("example", "cancer.somatic.temp.sv")


def test_somatic_ranks_every_branch_of_the_table(tmp_path_factory, tmp_path, inflate):
    """the 227 tumor rows that take every branch of ReadTumorFileAndOutputSomaticInfo, the normal's tally over five ranks"""
    bam, clip_gz, _ = T._synth_sample(tmp_path_factory, "synthfull", T.SYNTH_FULL["synthfull"])
    out = str(tmp_path / "somatic.sv")
    r = _somatic(inflate + ["-N", "5", bam, clip_gz, os.path.join(G.GOLDEN, "somatic", "tumor.sv"), out])
    assert r.returncode == 0, r.stderr
    assert open(out).read() == G.read_text("somatic", "somatic.sv")
    assert T._somatic_stderr(r.stderr) == T._somatic_stderr(G.read_text("somatic", "somatic.stderr"))


def _rccl_loads():
    """the names the group's loader tries (csrc/group_api.inc), in a process of its own"""
    code = "import ctypes, sys\nfor n in sys.argv[1:]:\n    try:\n        ctypes.CDLL(n)\n        sys.exit(0)\n    except OSError:\n        pass\nsys.exit(1)\n"
    return subprocess.run([sys.executable, "-c", code, "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"]).returncode == 0


def test_somatic_one_rank_through_rccl(tmp_path_factory, tmp_path, inflate):
    """SSV_GROUP_RCCL_ONE=1: `-N 1` takes the ranks' path, its vector through a one-rank RCCL communicator - what a one-GPU box can run of the exchange"""
    if not _rccl_loads():
        pytest.skip("librccl does not load here")
    bam, clip_gz, _ = T._synth_sample(tmp_path_factory, "hbvnormal", T.HBV_NORMAL)
    out = str(tmp_path / "somatic.sv")
    r = _somatic(inflate + ["-N", "1", bam, clip_gz, os.path.join(G.GOLDEN, "synth", "hbvfull.loose.sv"), out], {"SSV_GROUP_RCCL_ONE": "1", "SSV_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    assert open(out).read() == G.read_text("somatic", "hbv.somatic.sv")
    assert "exchange over RCCL" in r.stderr


@pytest.mark.parametrize("n", ["0", "-2"])
def test_somatic_ranks_usage(tmp_path, n):
    r = _somatic(["-N", n, "a.bam", "a.clip.gz", "t.sv", str(tmp_path / "o.sv")])
    assert r.returncode == 1 and "Usage: seeksv somatic" in r.stderr and " -N " in r.stderr
    assert os.listdir(str(tmp_path)) == []
