"""CPU: the surface of `seeksv run -P` and of ssv_realign_split_batch is there - the usage text, the exported symbol, its binding.  What they compute
needs a GPU: tests/test_realign_split_batch_gpu.py, tests/test_run_split_gpu.py."""
import ctypes as C
import os
import subprocess

from seeksv_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")


def test_usage_of_run_names_P():
    r = subprocess.run([SEEKSV, "run"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Usage: seeksv run")
    line = [l for l in r.stderr.splitlines() if l.lstrip().startswith("-P ")]
    assert len(line) == 1 and "unmapped" in line[0]
    assert "no prefix.F.bam is written" in r.stderr and "-F in -v" in r.stderr and "-N in -c" in r.stderr


def test_library_exports_and_abi_binds_the_call():
    lib = _abi.hip_lib()
    assert hasattr(lib, "ssv_realign_split_batch") and lib.ssv_abi_version() == 9
    fn = lib.ssv_realign_split_batch
    assert len(fn.argtypes) == 11 and fn.argtypes[3] is C.c_int64
    assert fn.argtypes[9]._type_ is _abi.Batch and fn.argtypes[10]._type_ is _abi.Names
    assert "realign_rows" in lib.ssv_prof_names().decode().split("\n")
    from seeksv_amd.device import Context
    assert callable(Context.realign_split_batch)
