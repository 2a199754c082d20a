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


def _run(tmp_path, *options):
    """`seeksv run <options> a.bam ref.fa <tmp>/p` from inside the empty directory; no input exists: the command line is judged before anything is opened."""
    return subprocess.run([SEEKSV, "run", *options, "a.bam", "ref.fa", str(tmp_path / "p")], capture_output=True, text=True, cwd=str(tmp_path))


def _one_line(r):
    lines = r.stderr.splitlines()
    assert r.returncode == 1 and len(lines) == 1 and lines[0].startswith("seeksv run: "), r.stderr
    return lines[0]


def test_ranks_or_devices_inside_c_without_runs_own_N_are_refused(tmp_path):
    # (getclip's ranks would bypass what the aligner step and the junction stage take from the single pass; -v "-N n" stays `getsv -N` over the file)
    for words in ("-N 2", "-G 1"):
        assert "-c" in _one_line(_run(tmp_path, "-c", words)), words
    assert os.listdir(str(tmp_path)) == []


def test_errors_inside_the_step_options_end_the_run_before_anything_is_written(tmp_path):
    r = _run(tmp_path, "-v", "-l 95")  # getsv's range check
    assert r.returncode == 1 and r.stderr.startswith("Usage: seeksv getsv"), r.stderr
    r = _run(tmp_path, "-c", "-x")
    assert r.returncode == 1 and "Usage: seeksv getclip" in r.stderr and "invalid option" in r.stderr, r.stderr
    for words in ("-m -1", "-N 0"):
        r = _run(tmp_path, "-v", words)
        assert r.returncode == 1 and r.stderr.startswith("Usage: seeksv getsv"), (words, r.stderr)
    r = _run(tmp_path, "-a", "-c 0")  # as `seeksv realign -c 0`
    alone = subprocess.run([SEEKSV, "realign", "-c", "0", "ref.fa", "p.clip.fq.gz", "p.clip.bam"], capture_output=True, text=True, cwd=str(tmp_path))
    assert alone.returncode == 1 and alone.stderr.startswith("Usage: seeksv realign")
    assert (r.returncode, r.stdout, r.stderr) == (alone.returncode, alone.stdout, alone.stderr)
    assert os.listdir(str(tmp_path)) == []


def test_the_refusals_of_P_and_N_need_no_gpu(tmp_path):
    assert "-P" in _one_line(_run(tmp_path, "-N", "2", "-P"))
    assert "-N or -G inside -c or -v" in _one_line(_run(tmp_path, "-N", "2", "-c", "-N 2"))
    assert "-N or -G inside -c or -v" in _one_line(_run(tmp_path, "-N", "2", "-v", "-G 1"))
    assert os.listdir(str(tmp_path)) == []
