"""CPU: the host end of `getsv -F` (seeksv_amd/host/readthrough_stage.cpp) through tests/native/readthrough_check.cpp - MinusCigarRight /
AddCigarLeft as the reference has them (clip_reads.cpp:507-558) and the insert-or-count rule of FindJunction (process_bwasw.cpp:198-216)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = """minus 40M3I7M2D 0 -> 40M3I7M 1
minus 40M3I7M2D 5 -> 40M3I2M 1
minus 70M 30 -> 40M 1
minus 30M 30 -> 30M 0
minus 10M5D20M10X 12 -> 10M5D8M 1
minus 5=50M 50 -> 5=50M 0
add 70M 10 -> 80M
add 5I65M 10 -> 10M5I65M
add 3=40M 2 -> 2M3=40M
chrA 1040 + chrA 5001 + | 0 0 | ACGT  0 0 3 0 | ACGT  0 0 3 0 | 1
chrA 100 - chrB 200 + | 4 0 | ACG 70M 0 0 0 2 | TGCA 4M5I60M 0 0 1 2 | 1
chrB 6050 + chrA 20001 + | 0 0 | AAAA 70M 0 0 0 2 | CCCCCC 60M 0 0 2 2 | 1
"""


def test_readthrough_host_stage(tmp_path):
    from seeksv_amd import _abi
    exe = str(tmp_path / "readthrough_check")
    flags = os.environ.get("SSV_TEST_CXXFLAGS", "-O2").split()  # (make asan: the sanitizer flags)
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "readthrough_check.cpp"),
                           os.path.join(ROOT, "seeksv_amd", "host", "readthrough_stage.cpp"), os.path.join(ROOT, "seeksv_amd", "host", "junction_stage.cpp"), "-o", exe,
                           "-L" + _abi.LIBDIR, "-lseeksv_host", "-lz", "-lpthread", "-Wl,-rpath," + _abi.LIBDIR])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    assert out == WANT
