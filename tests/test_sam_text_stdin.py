"""CPU: SamTextReader (seeksv_amd/host/sam_text.cpp) through tests/native/sam_text_check.cpp: "-" is standard input, read sequentially - through a pipe, plain
and gzip-compressed (told apart by the stream's first bytes, none of which is lost) - and hands out what the file of the same bytes hands out."""
import gzip
import os
import subprocess

import pytest

import readthrough_inputs as RT
import sam_text as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stc") / "sam_text_check")
    flags = os.environ.get("SSV_TEST_CXXFLAGS", "-O2").split()  # (make asan: the sanitizer flags)
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "native", "sam_text_check.cpp"),
                           os.path.join(ROOT, "seeksv_amd", "host", "sam_text.cpp"), "-o", out, "-lz", "-lpthread"])
    return out


def piped(exe, data, chunk):
    """the bytes through a pipe (not a file on the descriptor: no pread, no seek)"""
    p = subprocess.Popen([exe, "-", str(chunk)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.communicate(data)
    assert p.returncode == 0, err
    return out, err


@pytest.mark.parametrize("chunk", [1 << 20, 700])
def test_standard_input_plain_and_gzip_equal_the_file(exe, tmp_path, chunk):
    recs = ST.clip_positions(RT.small_records(), RT.LENS)
    data = ST.text(recs, RT.NAMES, RT.LENS).encode("latin-1")
    body = ST.text(recs, RT.NAMES, RT.LENS, with_header=False).encode("latin-1")
    head = "".join(f"{n} {l}\n" for n, l in zip(RT.NAMES, RT.LENS)).encode()
    n_hdr = data.count(b"\n") - body.count(b"\n")
    outs = {}
    for name, raw in (("plain", data), ("gzip", gzip.compress(data))):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(raw)
        r = subprocess.run([exe, p, str(chunk)], capture_output=True)
        assert r.returncode == 0, r.stderr
        is_gz = int(name == "gzip")
        assert r.stdout == f"targets 3 first_line {n_hdr + 1} gzip {is_gz}\n".encode() + head + body, name
        out, err = piped(exe, raw, chunk)
        assert out == r.stdout, name
        with open(p, "rb") as f:  # ... and a file on the descriptor
            r2 = subprocess.run([exe, "-", str(chunk)], stdin=f, capture_output=True)
        assert r2.returncode == 0 and r2.stdout == r.stdout, name
        outs[name] = err
    if chunk == 700:
        assert int(outs["plain"].split()[1]) > 10  # (several chunks)


def test_empty_standard_input(exe):
    out, err = piped(exe, b"", 1 << 20)
    assert out == b"targets 0 first_line 1 gzip 0\n"
