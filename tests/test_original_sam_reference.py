"""-m "not gpu": the real reference's getclip on the SAM text tests/original_sam.py makes of the bundled samples - a plain file, gzip, standard input
(clip_reads.h:363-384 opens every name without ".bam" as text) - writes the four outputs it writes for the .bam, and the same stderr behind libbam's
[samopen] line.  This holds the helper's text, not this repository's code: with it the committed goldens of the .bam runs are the expected outputs of
tests/test_getclip_sam_gpu.py.  The reference runs are skipped where oracle/_ref is not built; their result is recorded once as sha256 sums in
tests/golden/original_sam/reference.json (tests/golden/make_original_sam_reference.py), which the last test holds against the goldens without any binary."""
import json
import os

import pytest

import golden_util as G
import original_sam_reference as R

needs_reference = pytest.mark.skipif(not os.path.exists(R.SEEKSV_REF), reason="the real reference is not built (make -C oracle ref)")


@needs_reference
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("sample", R.SAMPLES)
def test_reference_reads_the_example_as_sam_text(tmp_path, sample, form):
    out, stderr, n_names = R.reference_getclip(str(tmp_path), sample, form)
    for ext in R.OUTPUTS:
        assert out[ext] == R.golden_bytes(sample, ext), ext
    assert stderr == f"[samopen] SAM header is present: {n_names} sequences.\n" + G.read_text("example", sample + ".getclip.stderr")


def test_recorded_reference_run_equals_the_goldens():
    """what the reference wrote for the text, as recorded, is what the goldens hold: every sample, form and output"""
    with open(R.RECORDED) as f:
        rec = json.load(f)
    assert sorted(rec) == sorted(R.SAMPLES)
    for sample in R.SAMPLES:
        assert sorted(rec[sample]) == sorted(R.FORMS)
        for form in R.FORMS:
            assert rec[sample][form] == {ext: R.sha(R.golden_bytes(sample, ext)) for ext in R.OUTPUTS}, (sample, form)
