"""CPU: what `seeksv run -A -S` adds to the surfaces that need no GPU - the usage text, the exported calls and their bindings, the header as C99 and its
rule beside the model's - the refusals, which come before the GPU is asked for and before any file exists, and the CPU build of the byte work
(tests/native/sa_parse_check.cpp: a stand-alone program under ASan + UBSan)."""
import ctypes as C
import glob
import os
import subprocess

from seeksv_amd import _abi, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
SA_FIELDS = ["sa_tags", "sa_multi", "sa_refused", "virtuals", "sa_redundant", "pairs_from_sa", "sa_dropped_length"]

C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "seeksv_hip.h"

int main(void)
{
	ssv_rt_original_sa_counts st;
	ssv_rt_params p;
	ssv_aux_t aux;
	const char *names[1] = {"chr1"};
	memset(&st, 0, sizeof(st));
	memset(&p, 0, sizeof(p));
	memset(&aux, 0, sizeof(aux));
	aux.mem = SSV_MEM_HOST; aux.encoding = SSV_AUX_SAM;
	/* without a context every call refuses its arguments: nothing here needs a GPU */
	if (ssv_rt_begin_original_sa(NULL, &p, names) != SSV_E_ARG) return 1;
	if (ssv_rt_original_sa_stats(NULL, &st) != SSV_E_ARG) return 2;
	if (ssv_rt_scan_aux(NULL, NULL, NULL, &aux) != SSV_E_ARG) return 3;
	if (ssv_bamdec_aux(NULL, &aux) != SSV_E_ARG || ssv_samdec_aux(NULL, &aux) != SSV_E_ARG) return 4;
	if (sizeof(st) != 7 * sizeof(int64_t) || SSV_AUX_BAM != 0 || SSV_AUX_SAM != 1) return 5;
	printf("%d %d\n", SSV_ABI_VERSION, (int)(st.sa_tags + st.sa_multi + st.sa_refused + st.virtuals + st.sa_redundant + st.pairs_from_sa + st.sa_dropped_length));
	return 0;
}
"""


def test_usage_text_names_the_option_and_its_limits():
    r = subprocess.run([SEEKSV, "run"], capture_output=True, text=True)
    assert r.returncode == 1
    text = " ".join(" ".join(r.stderr.splitlines()).split())
    assert "         -S  " in r.stderr and "         -A  " in r.stderr
    for words in ("with -A:", "SA:Z:rname,pos,strand,CIGAR, mapQ,NM;", "samtools view -F 0x800", "only when the record found no real partner", "a complete input gives what -A gives",
                  "S stands for the record's H", "no chaining", "sa_tags, sa_multi, sa_refused, virtuals, sa_redundant, pairs_from_sa and sa_dropped_length",
                  "Only with -A; not inside -c, -v or -a"):
        assert words in text, words


def test_refusals_leave_no_file(tmp_path):
    cases = [(["-S"], "-S without -A is not supported"), (["-S", "-u", "-D"], "-S without -A is not supported"), (["-A", "-S", "-c", "-S"], "-S inside -c, -v or -a is not supported"),
             (["-A", "-S", "-v", "-b 3 -S"], "-S inside -c, -v or -a is not supported"), (["-A", "-S", "-a", "-S 8"], "-S inside -c, -v or -a is not supported"),
             (["-S", "-a", "-S 8"], "-S inside -c, -v or -a is not supported")]
    for k, (opts, words) in enumerate(cases):
        pre = str(tmp_path / f"refused{k}")
        r = subprocess.run([SEEKSV, "run"] + opts + ["in.bam", "ref.fa", pre], capture_output=True, text=True, cwd=str(tmp_path))
        lines = [l for l in r.stderr.splitlines() if not l.startswith("[stamp]")]
        assert r.returncode == 1 and len(lines) == 1 and lines[0].startswith("seeksv run: -S") and words in lines[0], (opts, r.stderr)
        assert r.stdout == "" and not glob.glob(pre + "*") and os.listdir(tmp_path) == []
    # -A's own refusals are unchanged, with -S beside it too
    r = subprocess.run([SEEKSV, "run", "-A", "-S", "-P", "in.bam", "ref.fa", str(tmp_path / "p")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "-P is not supported with -A" in r.stderr and os.listdir(tmp_path) == []


def test_library_exports_the_calls_and_the_version_stays():
    lib = _abi.hip_lib()
    assert lib.ssv_abi_version() == 9
    for name in ("ssv_rt_begin_original_sa", "ssv_rt_scan_aux", "ssv_rt_original_sa_stats", "ssv_bamdec_aux", "ssv_samdec_aux"):
        assert hasattr(lib, name), name
    assert lib.ssv_rt_original_sa_stats.argtypes[1]._type_ is _abi.RtOriginalSaCounts
    assert [k for k, _ in _abi.RtOriginalSaCounts._fields_] == SA_FIELDS and C.sizeof(_abi.RtOriginalSaCounts) == 56
    assert [k for k, _ in _abi.Aux._fields_] == ["mem", "encoding", "n", "base", "off", "len", "bytes"] and C.sizeof(_abi.Aux) == 48
    names = lib.ssv_prof_names().decode().split("\n")
    for group in ("splitread_sa_aux", "splitread_sa_scan", "splitread_sa_finish", "splitread_scan", "splitread_finish"):
        assert group in names, group
    assert len(names) == len(set(names))
    assert lib.ssv_rt_begin_original_sa(None, None, None) == -3 and lib.ssv_rt_original_sa_stats(None, None) == -3 and lib.ssv_rt_scan_aux(None, None, None, None) == -3


def test_bindings():
    for name in ("rt_begin_original_sa", "rt_scan_aux", "rt_original_sa_stats", "readthrough_original_sa", "bamdec_aux", "samdec_aux"):
        assert callable(getattr(device.Context, name)), name


def test_header_states_the_rule_as_the_model_does():
    header = " ".join(open(os.path.join(ROOT, "include", "seeksv_hip.h")).read().replace("\n *", " ").split())
    model = " ".join(open(os.path.join(ROOT, "tests", "splitread_sa_model.py")).read().replace("\\\\r", "\\r").split())
    for sentence in ("Only a source has its optional fields looked at.", "an unknown type ends the walk.", "The first field with tag SA and type Z is taken; SA with another type is passed over.",
                     "a Z or H value with no NUL before the record's end, or a B array that runs over it, ends the walk with no value.",
                     "A field matches only when it begins with \"SA:Z:\" directly behind a tab", "at the newline, or at the end of the last line.",
                     "a missing final ';' at the value's end is accepted.", "rname must be a contig of the header, by exact name: else sa_refused.",
                     "R_source == R_virtual (unequal: sa_dropped_length).", "A virtual candidate whose source found a real partner is sa_redundant."):
        assert sentence in header, sentence
        assert sentence in model, sentence


def test_header_compiles_as_c99_with_the_calls(tmp_path):
    src, exe = str(tmp_path / "splitread_sa_abi.c"), str(tmp_path / "splitread_sa_abi")
    with open(src, "w") as f:
        f.write(C_PROGRAM)
    libdir = _abi.LIBDIR
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir, "-lseeksv_hip",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["9", "0"], (r.returncode, r.stdout, r.stderr)


def test_byte_work_as_a_program_under_the_sanitizers(tmp_path):
    """the two walkers, the entry parser and the contig look-up over areas that end exactly where their heap buffer ends: a read beyond `end` stops the program"""
    exe = str(tmp_path / "sa_parse_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "native", "sa_parse_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")   # (the runtimes linked statically: nothing to preload)
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "sa_parse_check: every case passed", (r.returncode, r.stdout, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
