"""-m "not gpu", skipped where the real reference is not built (oracle/_ref, `make -C oracle ref`): the reference writes the same SV table and the same
stdout from the SAM text tests/clip_sam.py makes of a clip.bam as from the .bam itself - as a plain file, gzip-compressed and on standard input
(getsv.h:437-446 opens every name without ".bam" as text).  This holds the helper's text, not this repository's code: with it, the committed outputs of
the .bam runs are the expected outputs of tests/test_getsv_clip_sam_gpu.py."""
import gzip
import os
import subprocess

import pytest

import clip_sam
import golden_util as G
import test_random_cli_vs_reference_gpu as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV_REF = os.path.join(ROOT, "oracle", "_ref", "seeksv_ref")
EX = os.path.join(G.GOLDEN, "example")
pytestmark = pytest.mark.skipif(not os.path.exists(SEEKSV_REF), reason="the real reference is not built (make -C oracle ref)")


def ref_getsv(args, stdin=None):
    r = subprocess.run([SEEKSV_REF, "getsv"] + args, capture_output=True, text=True, stdin=stdin if stdin is not None else subprocess.DEVNULL)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r


def all_forms(d, flags, clip_bam, bam, clip_gz):
    """-> [(sv, stdout, stderr lines)] of the reference for the .bam, the plain text, the gzip text and the text on standard input"""
    sam, samgz = os.path.join(d, "c.sam"), os.path.join(d, "c.sam.gz")
    clip_sam.write(sam, clip_bam)
    clip_sam.write(samgz, clip_bam)
    outs = []
    for tag, clip in (("bam", clip_bam), ("sam", sam), ("gz", samgz), ("stdin", "-")):
        sv = os.path.join(d, f"ref.{tag}.sv")
        if clip == "-":
            with open(sam, "rb") as f:
                r = ref_getsv(flags + ["-", bam, clip_gz, sv, os.path.join(d, "r.fq")], stdin=f)
        else:
            r = ref_getsv(flags + [clip, bam, clip_gz, sv, os.path.join(d, "r.fq")])
        outs.append((open(sv).read(), r.stdout, r.stderr.splitlines()))
    return outs


def check_forms(outs, n_targets):
    line = f"[samopen] SAM header is present: {n_targets} sequences."
    for sv, stdout, err in outs[1:]:
        assert sv == outs[0][0] and stdout == outs[0][1]
        assert err.count(line) == 1 and err.index(line) < err.index("'InputSoftInfoStoreBreakpoint' finished")
        assert [l for l in err if l != line] == outs[0][2]
    assert line not in outs[0][2]


@pytest.mark.parametrize("sample", ["cancer", "normal"])
def test_reference_reads_the_example_as_sam_text(tmp_path, sample):
    clip_gz = str(tmp_path / "s.clip.gz")
    with gzip.open(clip_gz, "wb") as f:
        f.write(open(os.path.join(EX, sample + ".clip.txt"), "rb").read())
    clip_bam = os.path.join(EX, sample + ".clip.bam")
    outs = all_forms(str(tmp_path), [], clip_bam, os.path.join(EX, sample + ".sort.bam"), clip_gz)
    assert outs[0][0] == G.read_text("example", f"{sample}.sv") and outs[0][1] == G.read_text("example", f"{sample}.getsv.stdout")
    check_forms(outs, len(clip_sam.bam_header(clip_bam)[0]))


@pytest.mark.parametrize("tag,flags", RC.GETSV_RUNS, ids=[t for t, _ in RC.GETSV_RUNS])
def test_reference_reads_random_inputs_as_sam_text(tmp_path, tag, flags):
    ref = RC.reference_outputs()["getsv"]["0"][tag]
    bg, clip_bam, clip_gz = RC.make_inputs(0, str(tmp_path))
    outs = all_forms(str(tmp_path), list(flags), clip_bam, bg, clip_gz)
    assert RC.sha(outs[0][0]) == ref["sv"] and RC.sha(outs[0][1]) == ref["stdout"]
    check_forms(outs, 3)
