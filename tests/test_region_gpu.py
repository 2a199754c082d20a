"""-m gpu: ssv_regions_set / ssv_region_retain / ssv_batch_select (seeksv_amd/csrc/region_kernels.h) against the plain model (tests/region_model.py) on the
hand-made sets of tests/region_inputs.py, each in both modes.  The records reach the stage through the two device decoders - SAM text and BAM (which ships the
bases of clipped records only) - with the stream cut into 1, 2 and 3 batches and last_tid carried across.  What is compared is what the decoders gave: every
input record is read back from a plain ssv_batch_retain of the same decoded batch (line, hot columns, operations, bases + qualities), the model says which
stay, and the output must be exactly those, with the model's change list, tid_runs and last contig."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import coordsort_model as cm
import markdup_inputs as mi
import pairdup_inputs as pi
import pairdup_model as pm
import region_inputs as ri
import region_model as rm
from seeksv_amd import _abi
from seeksv_amd.device import Context, SeeksvError
from test_pairdup_gpu import bounds_of, decoded, empty_batch, read_back, release

pytestmark = pytest.mark.gpu

GROUPS = ("region_select", "region_gather")
PARTS = ("pos", "n_cigar", "cigar_ends", "rec", "cigar", "seqqual")
IDS = [s["name"] for s in ri.SETS]


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def set_list(ctx, s, exclude):
    ctx.regions_set(rm.normalise(s["regions"], s["lens"]), len(s["lens"]), exclude)


def expected(part, regions, exclude, prev_tid):
    """what the model says of one input batch: (kept indices, the output's change list, the contig behind it, its tid_runs or None)"""
    kept = rm.keep(part, regions, exclude)
    out = [part[i] for i in kept]
    changes, last = rm.changes(out, prev_tid)
    runs = rm.tid_runs(out)
    return kept, changes, last, runs if 1 <= len(runs) <= 64 else None


def check_output(ctx, out, info, before, part, want, uncopied=False):
    kept, changes, last, runs = want
    assert info["n_in"] == len(part) and info["n_kept"] == len(kept) == out.n and info["uncopied"] == uncopied
    assert info["changes"] == changes and info["last_tid"] == last
    got, lines, _ = read_back(ctx, out)
    bad = [k for k, (g, i) in enumerate(zip(got, kept)) if g != before[i]]
    assert not bad, (bad[:5], [kept[k] for k in bad[:5]])
    assert lines["isize"].tolist() == [part[i]["isize"] for i in kept]
    if not uncopied:                                             # (a batch handed back keeps the list it came with)
        r = out.get_tid_runs()
        if runs is None:
            assert r is None
        else:
            assert r is not None and list(zip(r["first"].tolist(), r["tid"].tolist())) == runs


def run_set(ctx, s, decoder, n_batches, exclude, how, tmp_path, keep_all_seq=True, unknown_span=False):
    """the set through one decoder in n_batches batches, restricted by region_retain (how == "retain") or by batch_select behind batch_retain; -> total kept"""
    recs = s["records"]
    bounds = bounds_of(len(recs), max(1, min(n_batches, len(recs))))      # (no empty part: a batch of 0 records has a test of its own)
    set_list(ctx, s, exclude)
    prev, total = 0, 0
    stream = decoded(ctx, recs, s["targets"], decoder, bounds, tmp_path, keep_all_seq=keep_all_seq) if recs else [empty_batch()]
    for k, (b, _) in enumerate(stream):
        part = recs[bounds[k]:bounds[k + 1]]
        plain = ctx.batch_retain(b)
        before, lines, _ = read_back(ctx, plain)
        assert lines["tid"].tolist() == [r["tid"] for r in part] and lines["pos"].tolist() == [r["pos"] for r in part]      # the decoder handed over the set itself
        if unknown_span:
            b.max_ref_span = 0
            plain.max_ref_span = 0
        want = expected(part, s["regions"], exclude, prev)
        if how == "retain":
            out, info = ctx.region_retain(b, prev)
            assert read_back(ctx, plain)[0] == before and not info["uncopied"]
            check_output(ctx, out, info, before, part, want)
            ctx.batch_release(plain)
        else:
            at = plain.tid
            out, info = ctx.batch_select(plain, prev)
            assert not plain.tid and plain.n == 0                  # the call's: zeroed
            all_kept = len(want[0]) == len(part)
            assert (out.tid == at) == all_kept
            check_output(ctx, out, info, before, part, want, uncopied=all_kept)
        assert out.max_ref_span == (0 if unknown_span else b.max_ref_span) and out.mem == (_abi.MEM_DEVICE | _abi.MEM_PERSISTENT)
        prev = info["last_tid"]
        total += int(out.n)
        ctx.batch_release(out)
        assert not out.tid and out.n == 0
    assert total == len(rm.keep(recs, s["regions"], exclude))
    return total


@pytest.mark.parametrize("n_batches", [1, 2, 3])
@pytest.mark.parametrize("decoder", ["sam", "bam"])
@pytest.mark.parametrize("s", ri.SETS, ids=IDS)
def test_sets_through_both_decoders_and_both_calls(ctx, s, decoder, n_batches, tmp_path):
    if n_batches > 1 and len(s["records"]) > 1000 and decoder == "bam":
        n_batches = 2                                            # (the large sets: fewer read-backs of the same records)
    for exclude in (False, True):
        for how in ("retain", "select"):
            run_set(ctx, s, decoder, n_batches, exclude, how, tmp_path)


def test_hand_written_answers(ctx):
    """the keep sets written out in tests/region_inputs.py, without the model in between"""
    s = ri.BY_NAME["grid"]
    set_list(ctx, s, False)
    (b, _), = decoded(ctx, s["records"], s["targets"], "sam", [0, len(s["records"])])
    out, info = ctx.region_retain(b)
    kept = set(ctx.batch_lines(out)["isize"].tolist())
    ctx.batch_release(out)
    by = {(r["cigar"], r["flag"], r["pos"]): r["isize"] for r in s["records"]}
    for k, want in ri.GRID_EXPECT.items():
        assert (by[k] in kept) == want, k
    for name in ("unplaced", "contig_order", "changes_on_dropped", "n0_list", "one_kept", "one_dropped"):
        s = ri.BY_NAME[name]
        for exclude, key in ((False, "kept"), (True, "kept_x")):
            set_list(ctx, s, exclude)
            (b, _), = decoded(ctx, s["records"], s["targets"], "sam", [0, len(s["records"])])
            out, info = ctx.region_retain(b)
            assert ctx.batch_lines(out)["isize"].tolist() == s["claim"][key], (name, exclude)
            if name == "changes_on_dropped":
                assert info["changes"] == s["claim"]["changes_out_x" if exclude else "changes_out"]
            ctx.batch_release(out)


def test_the_long_list_is_above_the_staging_capacity(ctx):
    assert ctx.region_lds_capacity() == ri.LDS_CAPACITY and ri.MANY > ctx.region_lds_capacity()
    s = ri.BY_NAME["region_counts"]
    per = [sum(1 for x in rm.normalise(s["regions"], s["lens"]) if x[0] == t) for t in range(4)]
    assert max(per[:3]) <= ctx.region_lds_capacity() < per[3]


@pytest.mark.parametrize("name", ["grid", "region_counts", "blocks", "seq_repack"])
def test_unknown_span_and_mixed_bases(ctx, name, tmp_path):
    """max_ref_span == 0 (unknown): no record is skipped by its distance, the decision is the same; the BAM decoder's mix of records with and without bases"""
    s = ri.BY_NAME[name]
    for exclude in (False, True):
        run_set(ctx, s, "sam", 2, exclude, "retain", tmp_path, unknown_span=True)
        run_set(ctx, s, "bam", 2, exclude, "select", tmp_path, keep_all_seq=False)
    if name == "seq_repack":
        set_list(ctx, s, False)
        for b, _ in decoded(ctx, s["records"], s["targets"], "bam", [0, len(s["records"])], tmp_path, keep_all_seq=False):
            out, _ = ctx.region_retain(b)
            has = ctx.batch_lines(out)["seq_off"] != np.uint64(2 ** 64 - 1)
            assert 0 < int(has.sum()) < len(has)
            ctx.batch_release(out)


def test_all_kept(ctx, tmp_path):
    """ssv_region_retain gives ssv_batch_retain's parts; ssv_batch_select gives the input's own pointers, uncopied, and launches no gather"""
    for decoder in ("sam", "bam"):
        s = ri.BY_NAME["all_kept"]
        set_list(ctx, s, False)
        for b, _ in decoded(ctx, s["records"], s["targets"], decoder, [0, len(s["records"])], tmp_path):
            plain = ctx.batch_retain(b)
            mine, info = ctx.region_retain(b)
            assert info["n_kept"] == info["n_in"] == len(s["records"]) and not info["uncopied"]
            assert mine.n == plain.n and mine.n_cigar_total == plain.n_cigar_total and mine.seqqual_bytes == plain.seqqual_bytes and mine.max_ref_span == plain.max_ref_span
            assert {p: getattr(mine, p) - mine.tid for p in PARTS} == {p: getattr(plain, p) - plain.tid for p in PARTS}
            (t1, l1, w1), (t2, l2, w2) = read_back(ctx, mine), read_back(ctx, plain)
            assert l1.tobytes() == l2.tobytes() and w1 == w2 and t1 == t2
            ctx.prof_enable(1)
            ctx.prof_reset()
            at = (plain.tid, plain.rec, plain.cigar, plain.seqqual)
            out, info = ctx.batch_select(plain)
            prof = {g: ctx.prof_get(g)["launches"] for g in GROUPS}
            ctx.prof_enable(0)
            assert info["uncopied"] and (out.tid, out.rec, out.cigar, out.seqqual) == at and prof["region_gather"] == 0 and prof["region_select"] > 0
            assert info["changes"] == rm.changes(s["records"])[0]
            assert read_back(ctx, out)[0] == t2
            release(ctx, [mine, out])
    # exclude mode with an empty list keeps everything too
    s = ri.BY_NAME["n0_list"]
    set_list(ctx, s, True)
    (b, _), = decoded(ctx, s["records"], s["targets"], "sam", [0, 3])
    out, info = ctx.batch_select(ctx.batch_retain(b))
    assert info["uncopied"] and info["n_kept"] == 3
    ctx.batch_release(out)


def test_an_empty_output_is_still_a_batch(ctx):
    s = ri.BY_NAME["none_kept"]
    set_list(ctx, s, False)
    (b, _), = decoded(ctx, s["records"], s["targets"], "sam", [0, len(s["records"])])
    out, info = ctx.region_retain(b, 1)
    assert out.n == 0 and out.tid and info["n_kept"] == 0 and info["changes"] == [] and info["last_tid"] == 1 and out.get_tid_runs() is None
    ctx.batch_release(out)
    # a batch of 0 records, through both calls
    e, _ = empty_batch()
    out, info = ctx.region_retain(e, 2)
    assert out.n == 0 and info == dict(n_in=0, n_kept=0, uncopied=False, last_tid=2, changes=[])
    sel, info = ctx.batch_select(out, 2)
    assert sel.n == 0 and info["n_in"] == 0 and info["uncopied"] and info["last_tid"] == 2
    ctx.batch_release(sel)


# ---- behind the other producers of a retained batch --------------------------------------------------------------------------------------------------------------

PD_REGIONS = [(0, 50, 150), (3, 0, 10)]


def lines_as_records(lines, recs):
    """the model's view of retained records: the decoded (tid, pos, flag) with the set's CIGAR text, found by what the records carry"""
    return [dict(tid=int(t), pos=int(p), flag=int(f), isize=int(i), cigar=c)
            for t, p, f, i, c in zip(lines["tid"].tolist(), lines["pos"].tolist(), lines["flag"].tolist(), lines["isize"].tolist(), [r["cigar"] for r in recs])]


def select_all(ctx, batches, model_recs, regions, exclude=False):
    """batch_select over retained batches (consumed) whose records the model sees as model_recs -> (outputs, their read-back tuples in one list)"""
    outs, got, prev, at = [], [], 0, 0
    for b in batches:
        part = model_recs[at:at + int(b.n)]
        at += int(b.n)
        before = read_back(ctx, b)[0]
        want = expected(part, regions, exclude, prev)
        out, info = ctx.batch_select(b, prev)
        check_output(ctx, out, info, before, part, want, uncopied=len(want[0]) == len(part))
        prev = info["last_tid"]
        outs.append(out)
        got += read_back(ctx, out)[0]
    return outs, got


def test_select_behind_dup_retain(ctx):
    s = mi.BY_NAME[[x["name"] for x in mi.SETS if x["dup"]][0]]
    recs = s["records"]
    ctx.regions_set([(0, 0, 50000)], len(mi.TARGETS))
    ctx.dup_begin()
    kept = []
    for b, nm in decoded(ctx, recs, mi.TARGETS, "sam", bounds_of(len(recs), 2)):
        kept.append(ctx.dup_retain(b, nm)[0])
    kept.append(ctx.dup_retain(*empty_batch(), last=True)[0])
    ctx.dup_finish()
    lines = np.concatenate([ctx.batch_lines(b) for b in kept])
    assert int((lines["flag"] & 0x400 != 0).sum()) == len(s["dup"]) > 0
    model = lines_as_records(lines, recs)
    regions = [(0, 0, 50000)]
    outs, got = select_all(ctx, kept, model, regions)
    flags = [np.frombuffer(t[0], _abi.RECORD_DTYPE)["flag"][0] for t in got]
    assert [int(f) for f in flags] == [model[i]["flag"] for i in rm.keep(model, regions)]      # the marks are carried
    release(ctx, outs)


def test_select_behind_pairdup_mark_and_sort(ctx):
    s = pi.BY_NAME["reverse_ends"]
    recs = pi.orders(s)[3][1]
    regions = PD_REGIONS
    ctx.regions_set(rm.normalise(regions, [100000] * len(pi.TARGETS)), len(pi.TARGETS))
    batches = [ctx.pairdup_retain(b, nm) for b, nm in decoded(ctx, recs, pi.TARGETS, "sam", bounds_of(len(recs), 2))]
    # before the mark the rows would be orphaned: refused, the batch stays what it was
    before = read_back(ctx, batches[0])[0]
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.batch_select(batches[0])
    assert batches[0].tid and read_back(ctx, batches[0])[0] == before and len(ctx.pairdup_rows(batches[0])) == batches[0].n
    want_flags = pm.mark(recs)
    ctx.pairdup_mark(batches)
    lines = np.concatenate([ctx.batch_lines(b) for b in batches])
    assert lines["flag"].tolist() == want_flags and want_flags != [r["flag"] for r in recs]
    model = lines_as_records(lines, recs)
    outs, got = select_all(ctx, batches, model, regions)
    kept = rm.keep(model, regions)
    assert 0 < len(kept) < len(recs)
    assert [int(np.frombuffer(t[0], _abi.RECORD_DTYPE)["flag"][0]) for t in got] == [want_flags[i] for i in kept]      # flags carried
    # ssv_batch_sort behind the select: the model's order of the kept records
    sel_model = [model[i] for i in kept]
    order = cm.order(sel_model, len(pi.TARGETS))
    res = ctx.batch_sort(outs, len(pi.TARGETS))
    after = sum((read_back(ctx, b)[0] for b in res["batches"]), [])
    assert after == [got[i] for i in order]
    # ... and a select behind the sort
    sorted_model = [sel_model[i] for i in order]
    regions2 = [(0, 0, 101)]
    ctx.regions_set(regions2, len(pi.TARGETS), False)
    outs2, got2 = select_all(ctx, res["batches"], sorted_model, regions2)
    assert got2 == [after[i] for i in rm.keep(sorted_model, regions2)] and got2
    release(ctx, outs2)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_list_that_is_not_normalised_is_refused(ctx):
    good = [(0, 10, 20), (0, 30, 40), (2, 0, 5)]
    ctx.regions_set(good, 3)
    for bad in ([(0, 30, 40), (0, 10, 20)], [(1, 0, 5), (0, 0, 5)], [(0, 10, 20), (0, 15, 30)], [(0, 10, 20), (0, 20, 30)], [(0, 10, 10)], [(0, 12, 10)], [(0, -1, 10)],
                [(3, 0, 5)], [(-1, 0, 5)]):
        with pytest.raises(SeeksvError, match=r"\(-3\)"):
            ctx.regions_set(bad, 3)
    lib, h = ctx._lib, ctx._h
    assert lib.ssv_regions_set(h, None, 1, 3, 0) == -3 and lib.ssv_regions_set(h, None, -1, 3, 0) == -3
    # the list of before is still the one in use
    s = ri.BY_NAME["one_kept"]
    ctx.regions_set([(0, 10, 20)], 1)
    with pytest.raises(SeeksvError):
        ctx.regions_set([(0, 10, 20), (0, 20, 21)], 1)
    (b, _), = decoded(ctx, s["records"], s["targets"], "sam", [0, 1])
    out, info = ctx.region_retain(b)
    assert info["n_kept"] == 1
    ctx.batch_release(out)
    ctx.regions_set([], 0)                                       # n == 0 is a valid list


def test_errors_leave_the_input_readable_and_releasable(ctx):
    s = ri.BY_NAME["seq_repack"]
    recs = s["records"]
    lib, h = ctx._lib, ctx._h
    (b, _), = decoded(ctx, recs, s["targets"], "sam", [0, len(recs)])
    plain = ctx.batch_retain(b)
    before = read_back(ctx, plain)
    out, info = _abi.Batch(), _abi.RegionInfo()
    # no list set
    ctx.regions_clear()
    assert lib.ssv_region_retain(h, C.byref(b), 0, C.byref(out), C.byref(info)) == -4 and lib.ssv_batch_select(h, C.byref(plain), 0, C.byref(out), C.byref(info)) == -4
    set_list(ctx, s, False)
    # NULL arguments
    assert lib.ssv_region_retain(h, None, 0, C.byref(out), C.byref(info)) == -3 and lib.ssv_region_retain(h, C.byref(b), 0, None, C.byref(info)) == -3
    assert lib.ssv_region_retain(h, C.byref(b), 0, C.byref(out), None) == -3
    assert lib.ssv_batch_select(h, None, 0, C.byref(out), C.byref(info)) == -3 and lib.ssv_batch_select(h, C.byref(plain), 0, None, C.byref(info)) == -3
    assert lib.ssv_batch_select(h, C.byref(plain), 0, C.byref(out), None) == -3
    # a host batch; a device batch that is not retained; a copy of a batch released before
    hostb, keep = _abi.make_batch(ctx.batch_to_host(b))
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.region_retain(hostb)
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.batch_select(hostb)
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.batch_select(b)
    gone = ctx.batch_retain(b)
    stale = _abi.Batch()
    C.memmove(C.byref(stale), C.byref(gone), C.sizeof(_abi.Batch))
    ctx.batch_release(gone)
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.batch_select(stale)
    after = read_back(ctx, plain)
    assert after[0] == before[0] and after[1].tobytes() == before[1].tobytes() and after[2] == before[2] and plain.tid
    # ... and the calls go on as if none of these had been made
    out, info = ctx.batch_select(plain)
    assert info["n_kept"] == len(rm.keep(recs, s["regions"])) and not plain.tid
    with pytest.raises(SeeksvError):                             # the input went with the call: a second release is refused
        ctx.batch_release(plain)
    ctx.batch_release(out)


WORKER = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import ctypes as C
import region_inputs as ri
import region_model as rm
from seeksv_amd import _abi
from seeksv_amd.device import Context, SeeksvError
from test_pairdup_gpu import decoded
s = ri.BY_NAME["seq_repack"]
ctx = Context(0)
def plain():
    (b, _), = decoded(ctx, s["records"], s["targets"], "sam", [0, len(s["records"])])
    return ctx.batch_retain(b)
first = plain()
second = plain()
step = second.tid - first.tid                             # what one such batch takes in the arena: batches lie back to back
at = first.tid
assert at and step > 0
out, info = _abi.Batch(), _abi.RegionInfo()
ctx.regions_set(rm.normalise(s["regions"], s["lens"]), 1)
assert ctx._lib.ssv_batch_select(ctx._h, C.byref(second), 0, C.byref(out), None) == -3
assert ctx._lib.ssv_batch_select(ctx._h, C.byref(second), 0, None, C.byref(info)) == -3
ctx.regions_clear()
assert ctx._lib.ssv_batch_select(ctx._h, C.byref(second), 0, C.byref(out), C.byref(info)) == -4
stale = _abi.Batch()
C.memmove(C.byref(stale), C.byref(second), C.sizeof(_abi.Batch))
stale.mem = _abi.MEM_DEVICE
ctx.regions_set(rm.normalise(s["regions"], s["lens"]), 1)
assert ctx._lib.ssv_batch_select(ctx._h, C.byref(stale), 0, C.byref(out), C.byref(info)) == -3
third = plain()
assert third.tid - second.tid == step, (third.tid - second.tid, step)      # no refused call left a slab behind: the next batch lies right behind the second
sel, info = ctx.batch_select(second)
assert sel.tid - third.tid == step and info["n_kept"] == len(rm.keep(s["records"], s["regions"])) and not second.tid
for b in (first, third, sel):
    ctx.batch_release(b)
again = plain()
assert again.tid == at                             # ... and everything went back: the arena starts over
ctx.batch_release(again)
ctx.close()
print("ok")
'''


def test_a_refused_select_gives_its_slab_back():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", WORKER % (os.path.dirname(here), here)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


# ---- nothing new without the stage -------------------------------------------------------------------------------------------------------------------------------

def pipeline(ctx, recs, targets, restrict):
    """plain retention (or region_retain with a list that keeps everything) + the clip scan, -M's retention, -u's sort -> launches per profiling group"""
    ctx.prof_enable(1)
    ctx.prof_reset()
    keep = []
    for b, _ in decoded(ctx, recs, targets, "sam", bounds_of(len(recs), 2)):
        keep.append(ctx.region_retain(b)[0] if restrict else ctx.batch_retain(b))
    ctx.getclip(keep)
    ctx.dup_begin()
    more = [ctx.dup_retain(b, nm)[0] for b, nm in decoded(ctx, recs, targets, "sam", [0, len(recs)])]
    more.append(ctx.dup_retain(*empty_batch(), last=True)[0])
    ctx.dup_finish()
    res = ctx.batch_sort([ctx.batch_retain(b) for b, _ in decoded(ctx, recs[::-1], targets, "sam", [0, 40, len(recs)])], len(targets))
    prof = {g: v["launches"] for g, v in ctx.prof_all().items()}
    ctx.prof_enable(0)
    release(ctx, keep + more + res["batches"])
    return prof


def test_launch_counts(ctx):
    s = ri.BY_NAME["seq_repack"]
    recs, targets = s["records"], s["targets"]
    ctx.regions_clear()
    plain = pipeline(ctx, recs, targets, False)
    assert all(plain[g] == 0 for g in GROUPS)                    # without a list set, no launch in the two new groups
    assert plain["clip_scan"] > 0 and plain["dup_retain"] > 0 and plain["sort_radix"] > 0
    ctx.regions_set([(0, 0, 1000)], 1)
    assert pipeline(ctx, recs, targets, False) == plain          # a list that nobody asks for changes nothing
    mine = pipeline(ctx, recs, targets, True)
    assert mine["region_select"] > 0 and mine["region_gather"] > 0
    for g in plain:                                              # the stage adds to its own two groups only: every other group's count is unchanged
        if g not in GROUPS:
            assert mine[g] == plain[g], g
    ctx.regions_clear()
