"""CPU: what `seeksv run -A` adds to the surfaces that need no GPU - the usage text, the two exported calls and their bindings, the header as C99 - and the
refusals, which come before the GPU is asked for and before any file exists."""
import ctypes as C
import glob
import os
import subprocess

from seeksv_amd import _abi, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")

C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "seeksv_hip.h"

int main(void)
{
	ssv_rt_original_counts st;
	ssv_rt_params p;
	memset(&st, 0, sizeof(st));
	memset(&p, 0, sizeof(p));
	/* without a context both calls refuse their arguments: nothing here needs a GPU */
	if (ssv_rt_begin_original(NULL, &p) != SSV_E_ARG) return 1;
	if (ssv_rt_original_stats(NULL, &st) != SSV_E_ARG) return 2;
	if (sizeof(st) != 7 * sizeof(int64_t)) return 3;
	printf("%d %d\n", SSV_ABI_VERSION, (int)(st.candidates + st.hard_clipped + st.pairs + st.pairs_borrowed + st.dropped_no_carrier + st.dropped_length + st.store_bytes));
	return 0;
}
"""


def test_usage_text_names_the_option_and_its_limits():
    r = subprocess.run([SEEKSV, "run"], capture_output=True, text=True)
    assert r.returncode == 1
    lines = r.stderr.splitlines()
    assert lines[0] == "Usage: seeksv run [options] <input.sorted.bam> <reference fasta(.gz)> <output prefix>"
    text = " ".join(" ".join(lines).split())
    assert "         -A  " in r.stderr
    for words in ("supplementary alignments", "flag 2048", "hard clips count", "mates never meet", "not the marks -M / -D make", "not restricted by -L / -X", "with -u it runs in input order",
                  "no chaining", "Not with -P, -F in -v or -N above 1, not inside -c, -v or -a"):
        assert words in text, words
    for opt in ("-P", "-M", "-D", "-u", "-L <file>", "-X <file>", "-N <int>"):                          # the others are still there
        assert f"         {opt} " in r.stderr, opt
    for cmd in ("getclip", "getsv", "realign", "somatic"):                                             # no other command has it
        r = subprocess.run([SEEKSV, cmd], capture_output=True, text=True)
        assert " -A " not in r.stderr, cmd


def test_refusals_leave_no_file(tmp_path):
    cases = [(["-A", "-P"], "-P is not supported with -A"), (["-A", "-v", "-F other.bam"], "-F inside -v names another source"), (["-A", "-N", "2"], "-N above 1 is not supported"),
             (["-c", "-A"], "-A inside -c, -v or -a is not supported"), (["-v", "-b 3 -A"], "-A inside -c, -v or -a is not supported"),
             (["-A", "-a", "-A"], "-A inside -c, -v or -a is not supported")]
    for k, (opts, words) in enumerate(cases):
        pre = str(tmp_path / f"refused{k}")
        r = subprocess.run([SEEKSV, "run"] + opts + ["in.bam", "ref.fa", pre], capture_output=True, text=True, cwd=str(tmp_path))
        lines = [l for l in r.stderr.splitlines() if not l.startswith("[stamp]")]
        assert r.returncode == 1 and len(lines) == 1 and lines[0].startswith("seeksv run: -A") and words in lines[0], (opts, r.stderr)
        assert r.stdout == "" and not glob.glob(pre + "*") and os.listdir(tmp_path) == []
    for cmd in ("getclip", "getsv"):                                                                    # `getsv -A` is no command of its own
        r = subprocess.run([SEEKSV, cmd, "-A", "in.bam"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and f"Usage: seeksv {cmd}" in r.stderr


def test_library_exports_the_two_calls_and_the_version_stays():
    lib = _abi.hip_lib()
    assert lib.ssv_abi_version() == 9
    for name in ("ssv_rt_begin_original", "ssv_rt_original_stats", "ssv_rt_begin", "ssv_rt_scan", "ssv_rt_finish"):
        assert hasattr(lib, name), name
    assert lib.ssv_rt_begin_original.argtypes == lib.ssv_rt_begin.argtypes
    assert lib.ssv_rt_original_stats.argtypes[1]._type_ is _abi.RtOriginalCounts
    assert [k for k, _ in _abi.RtOriginalCounts._fields_] == ["candidates", "hard_clipped", "pairs", "pairs_borrowed", "dropped_no_carrier", "dropped_length", "store_bytes"]
    assert C.sizeof(_abi.RtOriginalCounts) == 56
    names = lib.ssv_prof_names().decode().split("\n")
    assert names[-2:] == ["splitread_scan", "splitread_finish"] and "rt_scan" in names and len(names) == len(set(names))
    # without a context both refuse
    assert lib.ssv_rt_begin_original(None, None) == -3 and lib.ssv_rt_original_stats(None, None) == -3


def test_bindings():
    for name in ("rt_begin_original", "rt_original_stats", "readthrough_original", "rt_begin", "readthrough"):
        assert callable(getattr(device.Context, name)), name


def test_header_states_the_rule_as_the_model_does():
    """the rule stands once in the header, and the model's head says the same"""
    header = " ".join(open(os.path.join(ROOT, "include", "seeksv_hip.h")).read().replace("\n *", " ").split())
    model = " ".join(open(os.path.join(ROOT, "tests", "splitread_model.py")).read().split())
    for sentence in ("exactly one of its two ends is clipped. An end is clipped when its outermost operation is S or H.", "R is the sum of M I S = X H;",
                     "the clip length of the clipped end is the sum of the run of S / H operations at that end (5H10S85M: 15);",
                     "A record carries the read when it has no H, its bases are present (seq_off != SSV_NO_SEQ) and l_qseq == R.",
                     "The key is (read name, flag & 0xC0) in the place of the read name alone: mates never meet; single-end reads have 0 there.",
                     "R_A == R_B (else B counts as dropped_length);", "at least one of the two carries the read (else B counts as dropped_no_carrier).",
                     "(begin, len, rc) on the same strand, (R - begin - len, len, !rc) on opposite strands."):
        assert sentence in header, sentence
        assert sentence in model, sentence


def test_header_compiles_as_c99_with_the_two_calls(tmp_path):
    src, exe = str(tmp_path / "splitread_abi.c"), str(tmp_path / "splitread_abi")
    with open(src, "w") as f:
        f.write(C_PROGRAM)
    libdir = _abi.LIBDIR
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir, "-lseeksv_hip",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["9", "0"], (r.returncode, r.stdout, r.stderr)
