"""-m gpu: the device BGZF inflate on DEFLATE streams zlib never writes.  Every stream the other modules feed the inflate kernels was written by zlib; here the
payloads come from the catalogue of tests/deflate_cases.py (written bit by bit: codes longer than the look-up tables, distances up to 32,768, both encodings of
258, blocks at every bit phase, chains and literal runs at the resolve kernels' thresholds, empty blocks ...), carried as the seq + qual bytes of valid BAM
records.  The reference is the host reader (zlib underneath; tests/test_deflate_cases.py holds it and the catalogue against zlib on the CPU): the device decode
equals its batches column for column and byte for byte, under three chunkings, again with the decoder's own CRC32 pass over every inflated byte, and in all four
combinations of the kernels' forms (SSV_TOKENS = wave | lanes, SSV_RESOLVE = win | wave: read once per process, hence child processes).  Malformed streams are
refused in every form; the container's rarer forms (empty BGZF blocks, a second gzip extra subfield) decode like everything else."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import numpy as np
import pytest

import deflate_cases as D
import golden_util as G
from seeksv_amd import device
from test_bamdec_gpu import KEYS, _device_all, _flatten, _host_all

pytestmark = pytest.mark.gpu
DIR_ENV = "SSV_STREAMS_DIR"
FILES = tuple(D.carrier_plan())
CHUNKS = [(64 << 20, 1 << 16), (64 << 20, 1), (200_000, 7)]
FORM_CHUNKS = [(64 << 20, 1 << 16), (64 << 20, 1), (64 << 20, 3), (200_000, 7)]
MODES = [("wave", "win"), ("wave", "wave"), ("lanes", "win"), ("lanes", "wave")]


def _write_all(d):
    D.write_carriers(d)
    D.write_container_forms(os.path.join(d, "forms.bam"))
    for b in D.malformed():
        D.write_carrier(os.path.join(d, "bad_" + b.name + ".bam"), [(b.data, bytes(b.isize))])


@pytest.fixture(scope="session")
def stream_dir(tmp_path_factory):
    """the carrier files, written once per session; a child run gets the directory from its parent"""
    d = os.environ.get(DIR_ENV)
    if not d:
        d = str(tmp_path_factory.mktemp("streams"))
        _write_all(d)
    return d


@pytest.fixture(scope="module")
def ctx():
    with device.Context(0) as c:
        yield c


_HOST = {}


def _host(path):
    if path not in _HOST:
        hb, hunm = _host_all(path, True)
        _HOST[path] = (_flatten(hb), hunm)
    return _HOST[path]


def _same_as_host(ctx, path, chunk_bytes, max_blocks, verify_crc=False):
    h, hunm = _host(path)
    db, dunm, _, _ = _device_all(ctx, path, chunk_bytes, max_blocks, True, verify_crc=verify_crc)
    d = _flatten(db)
    for k in KEYS + ("shipped",):
        assert np.array_equal(h[k], d[k]), k
    assert h["cigars"] == d["cigars"]
    assert len(h["seqs"]) == len(d["seqs"])
    for i, (a, b) in enumerate(zip(h["seqs"], d["seqs"])):
        if a != b:
            at = next(j for j in range(min(len(a), len(b))) if a[j] != b[j]) if len(a) == len(b) else -1
            raise AssertionError(f"record {i}: seq + qual differ (first at byte {at} of {len(a)})")
    assert hunm == dunm
    h["unm"] = len(hunm)
    return h


@pytest.mark.parametrize("chunk_bytes,max_blocks", CHUNKS, ids=[f"{c}B-{m}blk" for c, m in CHUNKS])
@pytest.mark.parametrize("fname", FILES)
def test_catalogue_device_equals_host(ctx, stream_dir, fname, chunk_bytes, max_blocks):
    """every fixed column, the CIGARs, every shipped seq + qual byte (the catalogue's bytes) and the unmapped side channel"""
    h = _same_as_host(ctx, os.path.join(stream_dir, fname + ".bam"), chunk_bytes, max_blocks)
    n = len(D.carrier_plan()[fname])
    assert len(h["tid"]) == len(h["seqs"]) == n + (n + 1) // 4 and h["unm"] == (n + 1) // 4


@pytest.mark.parametrize("fname", FILES)
def test_catalogue_device_equals_host_with_crc(ctx, stream_dir, fname):
    """with the decoder's own CRC32 pass: every inflated byte - also those the record decoder does not hand out - against the trailer the carrier wrote from the expanded tokens"""
    _same_as_host(ctx, os.path.join(stream_dir, fname + ".bam"), 64 << 20, 1 << 16, verify_crc=True)


@pytest.mark.parametrize("chunk_bytes,max_blocks", FORM_CHUNKS, ids=[f"{c}B-{m}blk" for c, m in FORM_CHUNKS])
def test_container_forms_device_equals_host(ctx, stream_dir, chunk_bytes, max_blocks):
    """28-byte empty BGZF blocks between data blocks, several in a row, first behind the header, on chunk boundaries (max_blocks 1 and 3); extra fields with a second subfield before and after BC"""
    path = os.path.join(stream_dir, "forms.bam")
    h = _same_as_host(ctx, path, chunk_bytes, max_blocks)
    assert len(h["seqs"]) >= 20
    _same_as_host(ctx, path, chunk_bytes, max_blocks, verify_crc=True)


def test_malformed_streams_are_refused(ctx, stream_dir):
    """every malformed stream (zlib and the CPU build of the decoder refuse each: tests/test_deflate_cases.py) in a small file of its own: the device decoder raises,
    and afterwards a valid file still decodes to the host reader's batches"""
    bad = D.malformed()
    assert len(bad) == 21
    for b in bad:
        with pytest.raises((device.SeeksvError, IOError)):
            _device_all(ctx, os.path.join(stream_dir, "bad_" + b.name + ".bam"), 64 << 20, 1 << 16, True)
    _same_as_host(ctx, os.path.join(stream_dir, "structure.bam"), 64 << 20, 1 << 16)


@pytest.mark.parametrize("name", ["libdeflate.1.bam", "libdeflate.6.bam", "libdeflate.12.bam"])
def test_libdeflate_written_files(ctx, name):
    """files written by libdeflate (tests/golden/make_libdeflate_bam.py), as current htslib builds write them: distances up to 32,767, which zlib never emits"""
    path = os.path.join(G.GOLDEN, "bamdec", name)
    for chunk_bytes, max_blocks in CHUNKS:
        h = _same_as_host(ctx, path, chunk_bytes, max_blocks)
    _same_as_host(ctx, path, 64 << 20, 1 << 16, verify_crc=True)
    assert len(h["seqs"]) > 1000


def _child(args, env, timeout):
    return subprocess.run([sys.executable] + args, env=env, capture_output=True, text=True, cwd=ROOT, timeout=timeout)


@pytest.mark.parametrize("tokens,resolve", MODES, ids=[f"tokens_{t}-resolve_{r}" for t, r in MODES])
def test_kernel_forms(stream_dir, tokens, resolve):
    """pass 1 as a wavefront per block (inflate_wave.h) and as a lane per block (inflate_core.h), pass 2 with the LDS window and in global memory: all four
    combinations, forced, through every test above on the same files"""
    if os.environ.get(DIR_ENV):
        pytest.skip("already inside a mode run")
    env = dict(os.environ, SSV_TOKENS=tokens, SSV_RESOLVE=resolve)
    env[DIR_ENV] = stream_dir
    r = _child(["-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", "catalogue or container_forms or malformed or libdeflate"], env, 600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout and "deselected" in r.stdout


def _phase_lines(stream_dir, fname):
    """[tokens wave] / [resolve win] lines of one file's decode in a fresh process with SSV_INFLATE_PHASES=1 (the default forms: wavefront pass 1, window pass 2)"""
    env = dict(os.environ, SSV_INFLATE_PHASES="1", SSV_TOKENS="wave", SSV_RESOLVE="win")
    r = _child([os.path.abspath(__file__), os.path.join(stream_dir, fname + ".bam")], env, 300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    win = [tuple(float(x) for x in m) for m in re.findall(r"\[resolve win\] (\d+) BGZF blocks, ([\d.]+) rounds each; per round: ([\d.]+) tokens, ([\d.]+) phases, ([\d.]+) all-lanes matches, ([\d.]+) window moves", r.stderr)]
    rounds = [int(x) for x in re.findall(r"most rounds in one window (\d+)", r.stderr)]
    assert win and rounds, r.stderr[-3000:]
    return win, rounds


def test_the_slow_paths_are_reached(stream_dir):
    """evidence from the kernels' own counters that the catalogue gets where it aims: the window of pass 2 moves and all-lanes matches (long, overlapping, across
    the window's first byte) happen on the sweep and chain files; the chain of pass 1 needs all 64 rounds on codes of one length"""
    if os.environ.get(DIR_ENV):
        pytest.skip("already inside a mode run")
    for fname in ("sweep_a", "matches"):
        win, _ = _phase_lines(stream_dir, fname)
        assert sum(w[5] * w[1] * w[0] for w in win) > 0, f"{fname}: no window move"
        assert sum(w[4] * w[1] * w[0] for w in win) > 0, f"{fname}: no all-lanes match"
    _, rounds = _phase_lines(stream_dir, "uniform")
    assert max(rounds) >= 64


if __name__ == "__main__":   # one file through the device decoder (test_the_slow_paths_are_reached reads what the kernels' counters print)
    with device.Context(0) as c:
        db, _, _, _ = _device_all(c, sys.argv[1], 64 << 20, 1 << 16, True)
        print(sum(len(b["tid"]) for b in db), "records")
