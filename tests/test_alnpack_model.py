"""CPU: the plain-Python name hash of tests/clip_sam.py - the model tests/test_alnpack_gpu.py holds ssv_aln_pack's hashes against - gives the numbers of the
host's own clip_text_hash (junction_stage.cpp:42-50, through tests/native/alnpack_check.cpp), at every length around the 8-byte words it reads."""
import os
import subprocess

import numpy as np
import pytest

import clip_sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 254)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from seeksv_amd import _abi
    out = str(tmp_path_factory.mktemp("ap") / "alnpack_check")
    flags = os.environ.get("SSV_TEST_CXXFLAGS", "-O2").split()  # (make asan: the sanitizer flags)
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "alnpack_check.cpp"),
                           os.path.join(ROOT, "seeksv_amd", "host", "junction_stage.cpp"), "-o", out, "-L" + _abi.LIBDIR, "-lseeksv_host", "-lz", "-lpthread", "-Wl,-rpath," + _abi.LIBDIR])
    return out


def test_python_text_hash_equals_the_hosts(exe):
    rng = np.random.RandomState(3)
    names = []
    for n in LENGTHS:
        names.append(bytes(rng.choice(list(b"ACGTN"), n).tolist()))
        names.append(bytes(rng.randint(33, 127, n).astype(np.uint8).tolist()))  # every printable byte
        names.append(bytes(x for x in rng.randint(128, 256, n).astype(np.uint8).tolist()))  # bytes with the top bit set (no sign extension)
    r = subprocess.run([exe], input=b"".join(x + b"\n" for x in names), capture_output=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(names)
    assert got == [clip_sam.text_hash(x) for x in names]
    assert sorted({len(x) for x in names}) == list(LENGTHS)
    assert len(set(got)) == len(set(names))  # (the empty name comes three times)
    assert clip_sam.text_hash("ACGT") == clip_sam.text_hash(b"ACGT") != clip_sam.text_hash(b"ACGT\0")
