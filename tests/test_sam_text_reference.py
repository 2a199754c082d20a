"""-m "not gpu", skipped where the real reference is not built (oracle/_ref, `make -C oracle ref`): the SAM text tests/sam_text.py writes decodes - through
libbam 0.1.16's own text reader (oracle/_ref/sam2bam) - to the records tests/bamio.write_bam writes, in every variant; and the committed goldens of the
SAM-text tests (tests/golden/samdec/, tests/golden/readthrough/sam.json) are what the reference writes today."""
import json
import os
import subprocess
import sys

import pytest

import bamio
import readthrough_inputs as RT
import sam_text as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAM2BAM = os.path.join(ROOT, "oracle", "_ref", "sam2bam")
SEEKSV_REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
pytestmark = pytest.mark.skipif(not (os.path.exists(SAM2BAM) and os.path.exists(SEEKSV_REF)), reason="the real reference is not built (make -C oracle ref)")

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

VARIANTS = [{}, dict(lower=True), dict(dot_n=True), dict(hex_flags=True), dict(tags=True), dict(crlf=True), dict(final_newline=False),
            dict(lower=True, dot_n=True, hex_flags=True, tags=True, crlf=True, final_newline=False)]


def through_libbam(tmp_path, recs, **kw):
    sam, bam = str(tmp_path / "t.sam"), str(tmp_path / "t.bam")
    ST.write(sam, recs, RT.NAMES, RT.LENS, **kw)
    r = subprocess.run([SAM2BAM, sam, bam], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return ST.read_bam_full(bam)


@pytest.mark.parametrize("variant", VARIANTS, ids=["+".join(v) or "plain" for v in VARIANTS])
def test_helper_text_decodes_to_the_bam_records(tmp_path, variant):
    """small file and a random seed, with qualities, mate fields and XC tags (no '=' / 'X' CIGARs: libbam's text reader aborts on them)"""
    for base in (RT.small_records(), RT.random_records(0, n_names=300)):
        recs = ST.with_extras(ST.without_eq_x(ST.clip_positions(base, RT.LENS)), 5)
        for r in recs:
            r["aux"] = ST.bam_aux(r)
        ref = str(tmp_path / "ref.bam")
        bamio.write_bam(ref, RT.NAMES, RT.LENS, recs)
        names, got = through_libbam(tmp_path, recs, **variant)
        wnames, want = ST.read_bam_full(ref)
        assert names == wnames == RT.NAMES
        assert got == want
        assert got == [ST.expected(r) for r in recs]
        simple = [dict(qname=r["qname"], flag=r["flag"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar=[(l, "MIDNSHP=X"[op]) for l, op in r["cigar"]], l_qseq=r["l_qseq"]) for r in got]
        assert bamio.read_bam_records(ref)[1] == simple


def test_forms_golden_is_what_libbam_decodes(tmp_path):
    import make_samdec_reference as M
    want = json.load(open(os.path.join(M.OUT, "forms.json")))
    L, ends = M.forms()
    data = ST.header(M.NAMES, M.LENS).encode() + b"".join(a + e for a, e in zip(L, ends))
    assert data == open(os.path.join(M.OUT, "forms.sam"), "rb").read()
    bam = str(tmp_path / "forms.bam")
    r = subprocess.run([SAM2BAM, os.path.join(M.OUT, "forms.sam"), bam], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names, recs = ST.read_bam_full(bam)
    assert names == want["names"] and recs == want["records"]


def test_readthrough_sam_golden_is_what_the_reference_writes(tmp_path):
    """the small file under every run, and the first random seed"""
    import make_readthrough_sam_reference as M
    want = json.load(open(os.path.join(RT.GOLDEN, "readthrough", "sam.json")))
    d = str(tmp_path / "small")
    os.makedirs(d)
    assert M.small(d) == want["small"]
    saved = RT.RANDOM_SEEDS
    try:
        RT.RANDOM_SEEDS = (0,)
        d = str(tmp_path / "random")
        os.makedirs(d)
        assert M.random(d)["0"] == want["random"]["0"]
    finally:
        RT.RANDOM_SEEDS = saved
