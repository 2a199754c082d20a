"""-m gpu: the second attempts.  The hot path guesses - the compact table's quality alphabet from the first events, its column widths, a staging size
for the two streaming passes, where a record starts in a BGZF block, a copy engine - and takes another path where a guess was wrong.  The inputs of
tests/rare_inputs.py make every such guess fail (tests/test_rare_inputs.py holds them to that on the CPU); here the results are held against the oracle
on the same batches, and a compact table also against the ASCII table of the same context."""
import gzip
import itertools
import os
import subprocess

import numpy as np
import pytest

import bamio
import oracle_lib as O
import rare_inputs as R
from seeksv_amd import _abi, device, host
from test_bam_reader import NAMES, LENS
from test_bamdec_gpu import CHUNKS, KEYS, _device_all, _flatten, _host_all, _runs_reference
from test_hip_golden import TABLE_KEYS, _compact_checks, assert_tables_equal
from test_oracle_golden import split_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")


@pytest.fixture(scope="module")
def ctx():
    with device.Context(0) as c:
        yield c


_made = {}


def _ladder(name, **opts):
    """(batch, the oracle's table of it): built once per module, shared, never written to"""
    key = (name,) + tuple(sorted(opts.items()))
    if key not in _made:
        _, first, late, _ = R.TRANSITION[name]
        b = R.ladder_batch(first, late, **opts)
        _made[key] = (b, O.getclip([b]))
    return _made[key]


def _alphabet(d):
    return [c - 33 for c in d["qual_alphabet"] if c]


def _compact(ctx, batches):
    """the ASCII table and the compact table of the same batches from the same context -> (ref, t, d)"""
    ref = ctx.getclip(batches)
    ctx.clip_table_format(3)
    try:
        ctx.clip_begin()
        for b in batches:
            ctx.clip_scan(b)
        t = ctx.clip_cluster(as_dict=False)
        return ref, t, host.table_to_dict(t)
    finally:
        ctx.clip_table_format(0)


# ---- a. the quality alphabet learned late ----

NO_GROUPS_SHAPE = {6: (3, 1), 9: (4, 1), 12: (4, 1)}   # SSV_QUAL_GROUPS=0: one quality, one field (the rows of test_compact_table_quality_alphabets)
LATE_CASES = [(t[0], True) for t in R.TRANSITIONS] + [("5to6", False), ("8to9", False), ("9to12", False)]


@pytest.mark.parametrize("name,groups", LATE_CASES, ids=[n + ("" if g else "-nogroups") for n, g in LATE_CASES])
def test_quality_alphabet_learned_late(ctx, monkeypatch, name, groups):
    """a quality value that only reads behind the first 4096 events carry: the first pack reports it (lut_miss), a second one with the tracking forms of
    k_pack3_stream / k_pack3_slow collects the table's values, a third packs with them - through every change of the quality stream's shape.  The late
    value is in the table's alphabet and no sample short of all events can have seen it: that is the evidence that the tracking launch ran."""
    _, first, late, shape = R.TRANSITION[name]
    if not groups:
        monkeypatch.setenv("SSV_QUAL_GROUPS", "0")
        shape = NO_GROUPS_SHAPE[len(first) + len(late)]
    b, want = _ladder(name)
    ref, t, d = _compact(ctx, [b])
    assert_tables_equal(ref, want)
    _compact_checks(ctx, d, ref, t)
    assert (d["qual_bits"], d["qual_group"]) == shape
    if d["qual_bits"] == 8:   # bytes (more than 45 values): the table carries characters and no alphabet - the characters of its strings are the alphabet
        chars = set().union(*(set(s[1] + s[3]) for s in (host.cluster_strings(d, k) for k in range(d["n_clusters"]))))
        assert _alphabet(d) == [] and sorted(ord(c) - 33 for c in chars) == sorted(set(first) | set(late))
    else:
        assert _alphabet(d) == sorted(set(first) | set(late))


# ---- b. the pack ladder's rungs together ----

RUNGS = {"support": dict(big_bin=70000), "exceptions": dict(n_every=7), "cigar": dict(long_skip=True)}


def _check_rungs(ctx, monkeypatch, name, rungs):
    opts = {}
    for r in rungs:
        opts.update(RUNGS[r])
    if "exceptions" in rungs:
        monkeypatch.setenv("SSV_EXC_CAP", "64")
    b, want = _ladder(name, **opts)
    ref, t, d = _compact(ctx, [b])
    assert_tables_equal(ref, want)
    assert (d["base_bits"], d["support_bytes"], d["cigar_bytes"]) == (4 if "exceptions" in rungs else 2, 4 if "support" in rungs else 2, 4 if "cigar" in rungs else 2)
    assert len(d["base_exc"]) == 0   # (4-bit bases carry their N themselves; without the rung there is none)
    _compact_checks(ctx, d, ref, t, check_size=False)
    return d


@pytest.mark.parametrize("name", ["4to5", "8to9", "16to17"])
def test_every_rung_of_the_pack_ladder_at_once(ctx, monkeypatch, name):
    """a bin of 70,000 reads (support to 32 bits), more bases outside A/C/G/T than SSV_EXC_CAP takes (bases to 4 bits), a 4096-base N (CIGAR operations to
    32 bits) and a late quality value in one table: the one loop of cluster_pack climbs all four, base_bits == 4 packs with a tracked alphabet"""
    _, first, late, shape = R.TRANSITION[name]
    d = _check_rungs(ctx, monkeypatch, name, ("support", "exceptions", "cigar"))
    assert _alphabet(d) == sorted(set(first) | set(late)) and (d["qual_bits"], d["qual_group"]) == shape


@pytest.mark.parametrize("pair", list(itertools.combinations(("support", "exceptions", "cigar", "late"), 2)), ids="+".join)
def test_every_pair_of_rungs(ctx, monkeypatch, pair):
    name = "4to5" if "late" in pair else "five-values"
    d = _check_rungs(ctx, monkeypatch, name, tuple(r for r in pair if r != "late"))
    assert len(_alphabet(d)) == 5 and (d["qual_bits"], d["qual_group"]) == (7, 3)


def test_late_alphabet_across_batches(ctx):
    """the same events from batches cut at records 1, 4097 and 5001: the sample, the late value and the stacks at the end each in a batch of their own"""
    _, first, late, shape = R.TRANSITION["4to5"]
    b, want = _ladder("4to5")
    cuts = [0, 1, 4097, 5001, len(b["tid"])]
    ref, t, d = _compact(ctx, [split_batch(b, cuts[k], cuts[k + 1]) for k in range(4)])
    assert_tables_equal(ref, want)
    _compact_checks(ctx, d, ref, t)
    assert _alphabet(d) == sorted(set(first) | set(late)) and (d["qual_bits"], d["qual_group"]) == shape


# ---- c. staging overflow of the clip scan ----

@pytest.fixture(scope="module")
def clip_overflow():
    b = R.clip_overflow_batch()
    return b, O.getclip([b])


def _clip_table(c, batches, fmt):
    """one getclip pass over host batches of one contig -> (dict, the table itself where it is the compact one)"""
    if fmt == 0:
        return c.getclip(batches), None
    c.clip_table_format(3)
    try:
        c.clip_begin()
        for b in batches:
            c.clip_scan(b)
        t = c.clip_cluster(as_dict=False)
        return host.table_to_dict(t), t
    finally:
        c.clip_table_format(0)


@pytest.mark.parametrize("cut", [None, 50000], ids=["whole", "cut-at-50000"])
@pytest.mark.parametrize("fmt", [0, 3], ids=["ascii", "compact"])
def test_clip_scan_staging_overflow(clip_overflow, fmt, cut):
    """six tiles of 8192 candidates each where a workgroup's share of a fresh context's staging holds 5462: k_clip_scan_ends leaves their counts at zero and
    raises the flag, ssv_clip_scan_range launches it again with four times the staging; the context keeps what it grew to.  (Cut at record 50,000 each part
    has few enough tiles to fit: the two parts' own launches.)"""
    b, want = clip_overflow
    batches = [b] if cut is None else [split_batch(b, 0, cut), split_batch(b, cut, len(b["tid"]))]
    with device.Context(0) as c:
        c.prof_reset()
        c.prof_enable(1)
        d = _clip_table(c, batches, fmt)[0]
        launches = c.prof_get("clip_scan")["launches"]
        print("clip_scan launches:", launches)
        ref = c.getclip(batches)
        assert_tables_equal(ref, want)
        c.prof_reset()
        d2, t2 = _clip_table(c, batches, fmt)
        assert c.prof_get("clip_scan")["launches"] == len(batches)   # the grown staging is kept
        if fmt == 3:
            _compact_checks(c, d2, ref, t2)
        else:
            assert_tables_equal(d2, want)
        assert d["n_clusters"] == d2["n_clusters"] and d["n_events"] == d2["n_events"]
        for k in TABLE_KEYS + (("runs", "base_exc") if fmt == 3 else ()):
            assert np.array_equal(d[k], d2[k]), k
        assert launches >= 2


# ---- d. staging overflow of the getsv scan ----

@pytest.mark.parametrize("runs", [False, True], ids=["k_getsv_scan", "k_getsv_scan_runs"])
@pytest.mark.parametrize("q", [20, 0])
def test_getsv_scan_staging_overflow(q, runs):
    """twenty tiles of 4096 candidates each where a workgroup's share of a fresh context's staging holds 3277: the scan runs again with four times the
    staging - the kernel that reads the tid column, and the one that takes the column as runs (a second contig's records behind the first's: two runs)"""
    b = dict(R.getsv_overflow_batch(tail_contig=runs))
    if runs:
        b["tid_runs"] = _abi.runs_of_tid(b["tid"])
        assert len(b["tid_runs"]) == 2
    else:
        b["no_tid_runs"] = True
    hdr, plan = R.getsv_overflow_plan()
    mean, sd = R.GETSV_OVERFLOW_STATS
    oc = O.discordant([b], plan.junctions, mean, sd, 4, q)
    ors, opd, _ = O.depth([b], plan.windows, plan.ranges, plan.points, q)
    assert oc.min() > 0 and opd.max() > 0
    with device.Context(0) as c:
        c.prof_reset()
        c.prof_enable(1)
        got_c, got_r, got_p = c.discordant_and_depth([b], plan, mean, sd, q, hdr.target_lens)
        launches = c.prof_get("getsv_scan")["launches"]
        print("getsv_scan launches:", launches)
        assert np.array_equal(got_c, oc) and np.array_equal(got_r, ors) and np.array_equal(got_p, opd)
        assert launches >= 2
    plan.close()
    hdr.close()


# ---- e. record starts that are none ----

@pytest.fixture(scope="module")
def decoy(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("decoy") / "decoy.bam")
    bamio.write_bam(path, NAMES, LENS, R.decoy_records())
    return path, {keep: _host_all(path, keep) for keep in (False, True)}


@pytest.mark.parametrize("keep_all", [False, True], ids=["clipseq", "allseq"])
@pytest.mark.parametrize("chunk_bytes,max_blocks", CHUNKS, ids=[f"{c}B-{m}blk" for c, m in CHUNKS])
def test_decoy_record_starts_are_repaired(ctx, decoy, chunk_bytes, max_blocks, keep_all):
    """aux arrays full of bytes that pass for record headers: blocks inside them guess a start where none is (k_find_records), the stitch must not believe
    it - neither where the chain of fakes runs into the next true record, nor where it breaks off, nor at a chunk's first block"""
    path, hosts = decoy
    hb, hunm = hosts[keep_all]
    db, dunm, druns, repaired = _device_all(ctx, path, chunk_bytes, max_blocks, keep_all)
    h, d = _flatten(hb), _flatten(db)
    assert len(h["tid"]) == 604
    for k in KEYS + ("shipped",):
        assert np.array_equal(h[k], d[k]), k
    assert h["cigars"] == d["cigars"] and h["seqs"] == d["seqs"]
    assert hunm == dunm and len(hunm) > 0
    assert druns == _runs_reference(h["flag"], h["tid"])
    print("repaired blocks:", repaired)
    if (chunk_bytes, max_blocks) == CHUNKS[0]:
        assert repaired >= 1


# ---- f. the runtime's copy ----

COPY_KEYS = TABLE_KEYS + ("runs", "base_exc")


def test_table_copy_by_the_runtime(monkeypatch, clip_overflow):
    """SSV_LINK_COPY=hip: the table leaves through hipMemcpyAsync on the copy stream (what every box without the HSA symbols does) - byte for byte the
    table of a default context, on the table that climbs every rung and on one of 54,068 clusters"""
    monkeypatch.setenv("SSV_EXC_CAP", "64")
    ladder = _ladder("4to5", big_bin=70000, n_every=7, long_skip=True)[0]
    tables = {}
    for mode in ("hip", None):
        if mode:
            monkeypatch.setenv("SSV_LINK_COPY", mode)
        else:
            monkeypatch.delenv("SSV_LINK_COPY")
        with device.Context(0) as c:
            c.clip_table_format(3)
            tables[mode] = [c.getclip([b]) for b in (ladder, clip_overflow[0])]
    for a, b, want in zip(tables["hip"], tables[None], (_ladder("4to5", big_bin=70000, n_every=7, long_skip=True)[1], clip_overflow[1])):
        assert a["format"] == 3 and a["n_clusters"] == b["n_clusters"] == want["n_clusters"] and a["n_events"] == b["n_events"] == want["n_events"]
        for k in COPY_KEYS:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        assert a["qual_alphabet"] == b["qual_alphabet"]
        for k in ("tid", "pos", "side", "support", "left_len", "right_len", "qual_missing", "n_cigar", "cigar"):
            assert np.array_equal(a[k], want[k]), k
        assert all(host.cluster_strings(a, k) == host.cluster_strings(want, k) for k in range(0, a["n_clusters"], 9))


# ---- g. through the command line ----

@pytest.mark.parametrize("way", ["plain", "pass-per-contig", "device-inflate"])
@pytest.mark.parametrize("name", ["4to5", "16to17"])
def test_cli_getclip_with_a_late_alphabet(tmp_path, name, way):
    """the row formatter reads a table whose alphabet was found by the tracking pass: clip.gz and clip.fq.gz equal the oracle's rows"""
    b = _ladder(name, n_every=7)[0]
    bam = str(tmp_path / "ladder.bam")
    host.write_bam(bam, R.LADDER_NAMES, R.LADDER_LENS, [b])
    _, _, batches = host.read_bam(bam)
    rows, fq = host.format_clip_outputs(O.getclip(batches, 0.9, 1, False), R.LADDER_NAMES)
    out = str(tmp_path / "o")
    env = dict(os.environ, SSV_PASS_RECORDS="1") if way == "pass-per-contig" else dict(os.environ)
    env.pop("SSV_DEVICE_INFLATE", None)
    r = subprocess.run([SEEKSV, "getclip"] + (["-Z"] if way == "device-inflate" else []) + ["-o", out, bam], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert gzip.open(out + ".clip.gz", "rt").read() == rows
    assert gzip.open(out + ".clip.fq.gz", "rt").read() == fq
