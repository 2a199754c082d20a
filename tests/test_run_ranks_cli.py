"""CPU: the surface of `seeksv run -N` and `seeksv somatic -N` is there - the usage texts and the refusals that need no GPU.  What the commands compute
needs one: tests/test_run_ranks_gpu.py, tests/test_somatic_ranks_gpu.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")


def _option_lines(text, opt):
    return [l for l in text.splitlines() if l.lstrip().startswith(opt + " ")]


def test_usage_of_run_names_N():
    r = subprocess.run([SEEKSV, "run"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Usage: seeksv run [options] <input.sorted.bam> <reference fasta(.gz)> <output prefix>\n")
    n = _option_lines(r.stderr, "-N")
    assert len(n) == 1 and "one per GPU" in n[0]
    g = _option_lines(r.stderr, "-G")
    assert len(g) == 1 and "-N" in g[0]
    # the -P paragraph as `tests/test_run_split_cli.py` reads it
    p = _option_lines(r.stderr, "-P")
    assert len(p) == 1 and "unmapped" in p[0]
    assert "no prefix.F.bam is written" in r.stderr and "-F in -v" in r.stderr and "-N in -c" in r.stderr


def test_usage_of_somatic_names_N():
    r = subprocess.run([SEEKSV, "somatic"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Usage: seeksv somatic")
    n = _option_lines(r.stderr, "-N")
    assert len(n) == 1 and "all-gather" in n[0]
    assert len(_option_lines(r.stderr, "-G")) == 1


def test_zero_ranks_print_the_usage_text(tmp_path):
    for cmd, operands in (("run", ["a.bam", "ref.fa", str(tmp_path / "p")]), ("somatic", ["a.bam", "a.clip.gz", "t.sv", str(tmp_path / "o.sv")])):
        for n in ("0", "-1"):
            r = subprocess.run([SEEKSV, cmd, "-N", n] + operands, capture_output=True, text=True)
            assert r.returncode == 1 and f"Usage: seeksv {cmd}" in r.stderr, (cmd, n)
    assert os.listdir(str(tmp_path)) == []
