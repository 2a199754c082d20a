"""-m gpu: the retained form.  ssv_batch_retain, ssv_dup_retain, ssv_pairdup_retain and ssv_batch_sort each hand out a batch that stays in HBM; the
passes behind them read all four alike, so all four must lay the same records out in the same way.  The record sets are tests/retained_form_inputs.py's, through the
SAM decoder; a refused call must give its slab back; a table of input batches with an empty one in it is one sequence all the same."""
import os
import subprocess
import sys

import numpy as np
import pytest

import coordsort_model as cm
import pairdup_inputs as pi
import retained_form_inputs as rf
from seeksv_amd import _abi
from seeksv_amd.device import Context
from test_pairdup_gpu import decoded, empty_batch, mark_and_check, read_back, release

pytestmark = pytest.mark.gpu

NT = len(rf.TARGETS)
PARTS = ("pos", "n_cigar", "cigar_ends", "rec", "cigar", "seqqual")


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def one_decode(ctx, recs):
    """(Batch, Names) of the records as one decoded batch: valid until the next decode"""
    if not recs:
        return empty_batch()
    (b, nm), = decoded(ctx, recs, rf.TARGETS, "sam", [0, len(recs)])
    return b, nm


def four_producers(ctx, recs):
    """-> {producer: retained batch of all the records in coordinate order}, and the other batches the calls made (empty ones)"""
    n, out, spare = len(recs), {}, []
    b, nm = one_decode(ctx, recs)
    out["batch_retain"] = ctx.batch_retain(b)
    ctx.dup_begin()
    first, carried = ctx.dup_retain(b, nm)
    last, carried_last = ctx.dup_retain(*empty_batch(), last=True)
    st = ctx.dup_finish()
    assert st["heads_marked"] == 0 and st["tails_marked"] == 0 and first.n + last.n == n and carried == 0 and carried_last == last.n
    out["dup_retain"], other = (first, last) if first.n == n else (last, first)      # (a placed last record is held back until the stream ends)
    spare.append(other)
    out["pairdup_retain"] = ctx.pairdup_retain(b, nm)
    rb, _ = one_decode(ctx, recs[::-1])
    res = ctx.batch_sort([ctx.batch_retain(rb)], NT)
    assert res["n_records"] == n and len(res["batches"]) == 1 and res["already_sorted"] == (n < 2)
    out["batch_sort"] = res["batches"][0]
    return out, spare


@pytest.mark.parametrize("name", ["FORM", "ONE", "NONE"])
def test_four_producers_one_form(ctx, name):
    recs = getattr(rf, name)
    n = len(recs)
    got, spare = four_producers(ctx, recs)
    back = {}
    for who, b in got.items():
        assert b.n == n and b.mem == (_abi.MEM_DEVICE | _abi.MEM_PERSISTENT), who
        # where the parts lie behind the slab's start (its tid column): the same in all four, each part 256-byte aligned
        assert b.tid and b.tid % 256 == 0, who
        off = {p: getattr(b, p) - b.tid for p in PARTS}
        assert all(o > 0 and o % 256 == 0 for o in off.values()) and list(off.values()) == sorted(off.values()), (who, off)
        back[who] = (off, read_back(ctx, b))
    ref_off, (ref_t, ref_lines, ref_whole) = back["batch_retain"]
    assert ref_lines["tid"].tolist() == [r["tid"] for r in recs] and ref_lines["pos"].tolist() == [r["pos"] for r in recs]
    assert ref_lines["flag"].tolist() == [r["flag"] for r in recs]                  # (no 0x400 anywhere)
    if n == len(rf.FORM):
        assert int(ref_lines["n_cigar"].max()) == 17 and int(ref_lines["n_cigar"][-1]) == 0 and ref_t[-1][1][3] == 0xff

    def bare(lines):
        x = lines.copy()
        x["cigar_off"] = 0
        x["seq_off"] = 0
        x["flag"] &= ~np.uint16(0x400)
        return x.tobytes()

    for who, (off, (t, lines, whole)) in back.items():
        assert off == ref_off, who
        assert whole[:5] == ref_whole[:5], who                                      # tid, pos, n_cigar, cigar_ends, the operations: byte for byte
        assert lines["cigar_off"].tolist() == ref_lines["cigar_off"].tolist() and got[who].n_cigar_total == got["batch_retain"].n_cigar_total, who
        assert bare(lines) == bare(ref_lines), who
        assert [x[1:3] for x in t] == [x[1:3] for x in ref_t], who
        both = [i for i in range(n) if t[i][3] is not None and ref_t[i][3] is not None]
        assert all(t[i][3] == ref_t[i][3] for i in both), who
        if n == len(rf.FORM):
            assert any(len(t[i][3]) > 16 for i in both), who                         # (a read of 40 bases among them: 60 bytes)
    # the two duplicate markers keep the bases of the soft-clipped reads only, and the same ones
    assert [x[3] for x in back["dup_retain"][1][0]] == [x[3] for x in back["pairdup_retain"][1][0]]
    assert got["dup_retain"].seqqual_bytes == got["pairdup_retain"].seqqual_bytes <= got["batch_retain"].seqqual_bytes == got["batch_sort"].seqqual_bytes
    release(ctx, list(got.values()) + spare)
    assert all(not b.tid and b.n == 0 for b in list(got.values()) + spare)


WORKER = r'''
import sys
import pathlib
import tempfile
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import pairdup_inputs as pi
import retained_form_inputs as rf
from seeksv_amd.device import Context, SeeksvError
from test_pairdup_gpu import decoded
ctx = Context(0)
def plain():
    (b, _), = decoded(ctx, rf.FORM, rf.TARGETS, "sam", [0, len(rf.FORM)])
    return ctx.batch_retain(b)
first = plain()
at = first.tid
assert at
ctx.batch_release(first)
recs = pi.orders(pi.BY_NAME["reverse_ends"])[3][1]
refused = False
with tempfile.TemporaryDirectory() as d:
    for b, names in decoded(ctx, recs, pi.TARGETS, "bam", [0, len(recs)], pathlib.Path(d), keep_all_seq=False):
        try:
            ctx.pairdup_retain(b, names)                  # refused behind the point where it took its slab: a record that takes part has no qualities
        except SeeksvError as e:
            assert "without its qualities" in str(e), e
            refused = True
assert refused
again = plain()
assert again.tid == at, (again.tid, at)                   # the refused call gave its slab back: the next batch lies where the first one lay
try:
    ctx.pairdup_rows(again)
    raise SystemExit("rows of a refused call are live")
except SeeksvError as e:
    assert "(-3)" in str(e), e
ctx.batch_release(again)
ctx.close()
print("ok")
'''


def test_a_refused_call_gives_its_slab_back():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", WORKER % (os.path.dirname(here), here)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


def seam_batches(ctx, retain):
    """SEAM as three batches, the middle one empty; retain(batch, names) -> retained batch"""
    out = []
    for k, (b, nm) in enumerate(decoded(ctx, rf.SEAM, pi.TARGETS, "sam", [0, rf.SEAM_CUT, len(rf.SEAM)])):
        out.append(retain(b, nm))
        if k == 0:
            out.append(retain(*empty_batch()))
    assert [int(b.n) for b in out] == [rf.SEAM_CUT, 0, len(rf.SEAM) - rf.SEAM_CUT]
    return out


def test_a_table_with_an_empty_batch_in_it(ctx):
    recs = rf.SEAM
    # ssv_pairdup_mark: the flags are the model's on the concatenation (mark_and_check)
    batches = seam_batches(ctx, ctx.pairdup_retain)
    lines, st = mark_and_check(ctx, recs, batches)
    assert st["pairs"] == rf.SEAM_CUT and st["pairs_marked"] == 5
    # ssv_batch_sort, of these batches (marked flags and all) and of plain ones
    for inputs in (batches, seam_batches(ctx, lambda b, nm: ctx.batch_retain(b))):
        before, model = [], []
        for b in inputs:
            t, ln, _ = read_back(ctx, b)
            before += t
            model += [dict(tid=int(t_), pos=int(p), flag=int(f)) for t_, p, f in zip(ln["tid"].tolist(), ln["pos"].tolist(), ln["flag"].tolist())]
        want = cm.order(model, NT)
        assert want != list(range(len(recs)))
        res = ctx.batch_sort(inputs, NT)
        assert res["n_records"] == len(recs) and not res["already_sorted"] and [int(b.n) for b in res["batches"]] == [len(recs)]
        after = read_back(ctx, res["batches"][0])[0]
        assert after == [before[i] for i in want]
        release(ctx, res["batches"])
