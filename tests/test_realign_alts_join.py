"""CPU: the records `seeksv realign -S` writes, through the host join of `seeksv getsv` (assemble_junctions of seeksv_amd/host/junction_stage.cpp, driven by
tests/native/junction_check.cpp).  The sample is tests/realign_alts_inputs.e2e_sample(): its clip.gz and clip.fq.gz are the real reference's getclip output
(tests/golden/realign_alts, kept by tests/golden/make_realign_alts_reference.py), clip.bam holds the MODEL's records (tests/realign_alts_model.py) for the one
clipped sequence - with its secondary records and without.  Every flag-256 record of the read name has to make a junction of its own."""
import gzip
import os
import subprocess

import pytest

import bamio
import realign_alts_inputs as AI
import realign_alts_model as AM
import realign_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "realign_alts")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from seeksv_amd import _abi
    out = str(tmp_path_factory.mktemp("jc") / "junction_check")
    flags = os.environ.get("SSV_TEST_CXXFLAGS", "-O2").split()  # (make asan: the sanitizer flags)
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "junction_check.cpp"),
                           os.path.join(ROOT, "seeksv_amd", "host", "junction_stage.cpp"), "-o", out, "-L" + _abi.LIBDIR, "-lseeksv_host", "-lz", "-lpthread", "-Wl,-rpath," + _abi.LIBDIR])
    return out


def clip_bam(path, max_alt):
    """clip.bam as `seeksv realign -c 500 [-S max_alt]` writes it for the sample's clip.fq.gz -> the records"""
    ref = M.Reference(AI.e2e_sample()[0])
    lines = gzip.open(os.path.join(GOLDEN, "e2e.clip.fq.gz"), "rt").read().splitlines()
    recs = []
    for s, q in zip(lines[1::4], lines[3::4]):
        res = AM.align_alts(ref, s, max_alt or 1, AI.CAP)
        if not max_alt:
            res["alts"] = []
        for r in AM.bam_records(s, q, res):
            recs.append(dict(qname=s, flag=r["flag"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar="".join(f"{n}{op}" for n, op in r["cigar"]), seq=r["seq"], qual=r["qual"]))
    bamio.write_bam(path, list(AI.E2E_NAMES), list(AI.E2E_LENS), recs)
    return recs


def junctions(exe, bam, *merge):
    r = subprocess.run([exe, "join", os.path.join(GOLDEN, "e2e.clip.gz"), bam] + list(merge), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [l.split("\t") for l in r.stdout.splitlines()]


@pytest.mark.parametrize("merge", [(), ("20",)], ids=["join", "join+merge"])
def test_every_secondary_record_makes_a_junction(exe, tmp_path, merge):
    """with the alternates: five junctions from tA 1001, one to each copy of the element on tB, the planted one (tB 921, copy 3) among them, all from the same
    clipped sequence with the same support; with the primary alone: one junction, to copy 1"""
    want = [("tA", str(AI.E2E_A + 1), "tB", str(p + 10 + 1)) for p in AI.E2E_COPIES]
    planted = ("tA", str(AI.E2E_A + 1), "tB", str(AI.E2E_B + 1))
    assert planted == want[2]
    recs = clip_bam(str(tmp_path / "alts.clip.bam"), 8)
    assert [r["flag"] for r in recs] == [0, 256, 256, 256, 256] and len({r["qname"] for r in recs}) == 1
    rows = junctions(exe, str(tmp_path / "alts.clip.bam"), *merge)
    assert sorted((x[0], x[1], x[3], x[4]) for x in rows) == sorted(want)
    assert all((x[2], x[5]) == ("+", "+") for x in rows)
    assert len({tuple(x[6:]) for x in rows}) == 1
    recs = clip_bam(str(tmp_path / "primary.clip.bam"), 0)
    assert [r["flag"] for r in recs] == [0]
    rows = junctions(exe, str(tmp_path / "primary.clip.bam"), *merge)
    assert [(x[0], x[1], x[3], x[4]) for x in rows] == [want[0]]
