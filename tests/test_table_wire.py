"""CPU: the host rebuild of the cluster table's narrow wire form (seeksv_amd/csrc/table_wire.h - rows of 6 bytes, position escapes, the kind-0
CIGAR stream) against an encoder of the test program's own (tests/native/table_wire_check.cpp), built with ASan + UBSan as a program with its own
main and run as a child process: seeded random tables, steps of 65534 / 65535 / 65536 bases, lengths of 255, supports of 254, every CIGAR kind,
over 1, 3 and 16 thread ranges and over ranges that start on an escape or just behind one; a wire form that contradicts itself is refused."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wire_rebuild_against_independent_encoder(tmp_path):
    exe = str(tmp_path / "table_wire_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "seeksv_amd", "csrc"), os.path.join(ROOT, "tests", "native", "table_wire_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout and "BAD" not in r.stdout
    assert int(r.stdout.split()[-4]) > 500   # tables
