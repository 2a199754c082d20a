"""-m gpu: ssv_batch_sort (seeksv_amd/csrc/sort_kernels.h) against the plain model (tests/coordsort_model.py) on the hand-made sets of tests/coordsort_inputs.py.
The records reach the stage through the two device decoders - SAM text (Context.sam_batches) and BAM (Context.bam_batches, which ships the bases of clipped
records only: a mix of records with and without bases) - as 1, 2 and 3 retained input batches.  What is compared is what the decoders gave: every retained input
record is read back before the sort (line, hot columns, operations, bases + qualities), the model orders them, and the concatenated outputs must be exactly
that, whatever the output batch size; the change lists per output batch are the model's over the decoded flags."""
import ctypes as C

import numpy as np
import pytest

import coordsort_inputs as ci
import coordsort_model as cm
import markdup_inputs as mi
from seeksv_amd import _abi, host
from seeksv_amd.device import Context, SeeksvError

pytestmark = pytest.mark.gpu

NO_SEQ = np.uint64(2 ** 64 - 1)
RETAINED = _abi.MEM_DEVICE | _abi.MEM_PERSISTENT
SETS = [s for s in ci.SETS if s["name"] != "deep_tie"]
IDS = [s["name"] for s in SETS]


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def retained_from_sam(ctx, s, n_batches):
    names = ci.targets_of(s)[0]
    parts = [mi.sam_text(b, names) for b in ci.batches_of(s, n_batches)]
    cuts = np.cumsum([len(p) for p in parts])[:-1].tolist()
    return [ctx.batch_retain(b) for b, _ in ctx.sam_batches(b"".join(parts), names, cuts=cuts)]


def retained_from_bam(ctx, s, n_batches, tmp_path):
    names, lens = ci.targets_of(s)
    out = []
    for k, part in enumerate(ci.batches_of(s, n_batches)):
        path = str(tmp_path / f"in{k}.bam")
        ci.write_bam(path, names, lens, part)
        with host.BamReader(path) as rd:
            out += [ctx.batch_retain(b) for b, _ in ctx.bam_batches(rd)]
    return out


def retained(ctx, s, decoder, n_batches, tmp_path):
    return retained_from_sam(ctx, s, n_batches) if decoder == "sam" else retained_from_bam(ctx, s, n_batches, tmp_path)


def read_back(ctx, b):
    """a retained batch -> one tuple per record of everything the batch says about it, free of where it lies in the batch's arrays:
    (line with cigar_off / seq_off taken out, (tid, pos, n_cigar, cigar_ends) of the hot columns, operations, bases + qualities or None)"""
    assert b.mem == RETAINED
    lines = ctx.batch_lines(b)
    dv = _abi.Batch()
    C.memmove(C.byref(dv), C.byref(b), C.sizeof(_abi.Batch))
    dv.mem, dv.tid_runs, dv.n_tid_runs = _abi.MEM_DEVICE, None, 0      # (ssv_batch_to_host takes the plain device form)
    h = ctx.batch_to_host(dv)
    n = int(b.n)
    # the variable parts lie back to back in record order: what a batch of the decoders, of ssv_batch_retain and of the sort all promise
    nc = lines["n_cigar"].astype(np.int64)
    assert lines["cigar_off"].tolist() == (np.cumsum(nc) - nc).tolist() and int(nc.sum()) == b.n_cigar_total
    has = lines["seq_off"] != NO_SEQ
    lq = np.maximum(lines["l_qseq"].astype(np.int64), 0)
    sb = np.where(has, (lq + 1) // 2 + lq, 0)
    assert lines["seq_off"][has].tolist() == (np.cumsum(sb) - sb)[has].tolist() and int(sb.sum()) == b.seqqual_bytes
    canon = lines.copy()
    canon["cigar_off"] = 0
    canon["seq_off"] = np.where(has, np.uint64(0), NO_SEQ)
    out = []
    for i in range(n):
        co, so = int(lines["cigar_off"][i]), int(lines["seq_off"][i])
        ops = tuple(h["cigar"][co:co + int(nc[i])].tolist())
        assert ops[:5] == tuple(lines["cigar_head"][i][:min(5, len(ops))].tolist())
        sq = bytes(h["seqqual"][so:so + int(sb[i])]) if has[i] else None
        out.append((canon[i].tobytes(), (int(h["tid"][i]), int(h["pos"][i]), int(h["n_cigar"][i]), int(h["cigar_ends"][i])), ops, sq))
    assert all(int(lines["tid"][i]) == out[i][1][0] and int(lines["pos"][i]) == out[i][1][1] and int(lines["n_cigar"][i]) == out[i][1][2] for i in range(n))
    return out, lines


def model_records(lines):
    return [dict(tid=int(t), pos=int(p), flag=int(f)) for t, p, f in zip(lines["tid"].tolist(), lines["pos"].tolist(), lines["flag"].tolist())]


def sort_and_check(ctx, s, inputs, max_out):
    """sorts the retained inputs (consumed), holds everything against the model, releases the outputs; -> the result dict"""
    nt = s["n_targets"]
    before, recs, spans = [], [], [b.max_ref_span for b in inputs if b.n]
    for b in inputs:
        t, lines = read_back(ctx, b)
        before += t
        recs += model_records(lines)
    # the decoders handed over the set itself
    assert [(r["tid"], r["pos"]) for r in recs] == [(r["tid"], r["pos"]) for r in s["records"]]
    assert [np.frombuffer(t[0], _abi.RECORD_DTYPE)["isize"][0] for t in before] == list(range(len(before)))
    want_order = cm.order(recs, nt)
    already = cm.is_sorted(recs, nt)
    pointers = [b.tid for b in inputs]
    ctx.prof_enable(1)
    ctx.prof_reset()
    res = ctx.batch_sort(inputs, nt, max_out)
    prof = {g: ctx.prof_get(g)["launches"] for g in ("sort_keys", "sort_radix", "sort_gather")}
    ctx.prof_enable(0)
    assert res["n_records"] == len(recs) and res["already_sorted"] == already
    after, out_recs = [], []
    for b in res["batches"]:
        t, lines = read_back(ctx, b)
        after += t
        out_recs.append(model_records(lines))
        runs = _abi.runs_of_tid(lines["tid"])
        got = b.get_tid_runs()
        if already:
            continue                                     # (the inputs as they came: the decoder's own list, or none)
        if 1 <= len(runs) <= 64:
            assert got is not None and got["first"].tolist() == runs["first"].tolist() and got["tid"].tolist() == runs["tid"].tolist()
        else:
            assert got is None
    assert len(after) == len(before)
    bad = [k for k, (a, i) in enumerate(zip(after, want_order)) if a != before[i]]
    assert not bad, (bad[:5], [np.frombuffer(after[k][0], _abi.RECORD_DTYPE)["isize"][0] for k in bad[:5]], [want_order[k] for k in bad[:5]])
    assert res["changes"] == cm.batch_changes(out_recs)
    if already:
        assert [b.tid for b in res["batches"]] == pointers and prof["sort_radix"] == 0 and prof["sort_gather"] == 0
    else:
        cap = max_out if max_out else 16 << 20
        assert [int(b.n) for b in res["batches"]] == [c for _, c in cm.cut(len(recs), cap)]
        assert all(b.max_ref_span == max(spans) for b in res["batches"])
        assert prof["sort_keys"] > 0 and prof["sort_radix"] > 0 and prof["sort_gather"] > 0
    for b in res["batches"]:
        ctx.batch_release(b)
        assert not b.tid and b.n == 0
    return res


@pytest.mark.parametrize("n_batches", [1, 2, 3])
@pytest.mark.parametrize("decoder", ["sam", "bam"])
@pytest.mark.parametrize("s", SETS, ids=IDS)
def test_sets_through_both_decoders(ctx, s, decoder, n_batches, tmp_path):
    for max_out in (0, 64):
        sort_and_check(ctx, s, retained(ctx, s, decoder, n_batches, tmp_path), max_out)


@pytest.mark.parametrize("s", SETS, ids=IDS)
def test_every_output_batch_size(ctx, s):
    n = len(s["records"])
    for max_out in sorted({m for m in (1, 2, 63, 64, 65, n - 1, n, n + 1) if m > 0}):
        res = sort_and_check(ctx, s, retained_from_sam(ctx, s, 3), max_out)
        if not res["already_sorted"]:
            assert len(res["batches"]) == (n + max_out - 1) // max_out


def test_the_bam_decoder_gives_a_mix_of_records_with_and_without_bases(ctx, tmp_path):
    for name in ("read_lengths", "cigar_lengths"):
        s = ci.BY_NAME[name]
        inputs = retained_from_bam(ctx, s, 2, tmp_path)
        has = np.concatenate([ctx.batch_lines(b)["seq_off"] != NO_SEQ for b in inputs])
        assert 0 < int(has.sum()) < len(has)
        sort_and_check(ctx, s, inputs, 3)


def test_sorted_inputs_come_back_as_they_are(ctx):
    for name, nb in (("sorted", 3), ("n0", 1), ("n1", 1), ("all_equal", 2)):
        s = ci.BY_NAME[name]
        inputs = retained_from_sam(ctx, s, nb)
        res = sort_and_check(ctx, s, inputs, 7)          # (max_out_records does not cut what is not copied)
        assert res["already_sorted"] and len(res["batches"]) == len(inputs)
    # sorted inside every batch but not across them is not sorted
    s = ci.BY_NAME["three_batches"]
    assert not sort_and_check(ctx, s, retained_from_sam(ctx, s, 3), 0)["already_sorted"]
    # the outputs of one sort, sorted again, are in order
    s = ci.BY_NAME["n2049"]
    res = ctx.batch_sort(retained_from_sam(ctx, s, 3), 3, 500)
    again = ctx.batch_sort(res["batches"], 3, 500)
    assert again["already_sorted"] and [b.tid for b in again["batches"]] == [b.tid for b in res["batches"]] and again["changes"] == res["changes"]
    for b in again["batches"]:
        ctx.batch_release(b)


def test_refusals_leave_the_inputs_alone(ctx):
    s = ci.BY_NAME["n65"]
    inputs = retained_from_sam(ctx, s, 2)
    before = [read_back(ctx, b)[0] for b in inputs]
    with pytest.raises(SeeksvError, match="n_targets"):
        ctx.batch_sort(inputs, 2, 0)                     # the set has records on c2
    with pytest.raises(SeeksvError):
        ctx.batch_sort(inputs, 3, -1)
    lib, h = ctx._lib, ctx._h
    arr, out = (_abi.Batch * 2)(*inputs), _abi.Sorted()
    assert lib.ssv_batch_sort(h, arr, 2, 2, 0, C.byref(out)) == -3 and lib.ssv_batch_sort(h, arr, 2, 3, 0, None) == -3 and lib.ssv_batch_sort(h, None, 2, 3, 0, C.byref(out)) == -3
    plain = _abi.Batch()
    C.memmove(C.byref(plain), C.byref(inputs[0]), C.sizeof(_abi.Batch))
    plain.mem = _abi.MEM_DEVICE                          # not a retained batch
    with pytest.raises(SeeksvError, match="ssv_batch_retain"):
        ctx.batch_sort([plain], 3, 0)
    assert [read_back(ctx, b)[0] for b in inputs] == before
    sort_and_check(ctx, s, inputs, 0)                    # ... and they still sort, and their memory is released by the call
    for b in inputs:                                     # released by the sort: a second release is refused
        with pytest.raises(SeeksvError):
            ctx.batch_release(b)


def test_stability_at_depth(ctx):
    """10^5 records at one key, in three input batches: nothing moves - through the shortcut, and, with one record of a smaller key behind them, through the
    radix passes (every pass sees one digit 10^5 times)"""
    s = ci.BY_NAME["deep_tie"]
    res = sort_and_check(ctx, s, retained_from_sam(ctx, s, 3), 0)
    assert res["already_sorted"]
    moved = dict(s, records=s["records"] + [dict(s["records"][0], pos=77, isize=len(s["records"]))])
    res = sort_and_check(ctx, moved, retained_from_sam(ctx, moved, 3), 40000)
    assert not res["already_sorted"] and len(res["batches"]) == 3


def test_samdec_any_order(ctx):
    """the sorted-original mode refuses a chunk with more than 65,536 contig changes; with ssv_samdec_any_order it goes through, without its change list"""
    n = 66000
    recs = [dict(ci.rec(k % 2, 100 + k), qname=f"r{k}", isize=k) for k in range(n)]
    text = mi.sam_text(recs, ci.TARGETS)
    ctx.samdec_begin(ci.TARGETS)
    ctx.samdec_sorted(False)
    with pytest.raises(SeeksvError, match="not coordinate sorted"):
        ctx.samdec_decode(text, last=True)
    ctx.samdec_begin(ci.TARGETS)
    ctx.samdec_sorted(False)
    ctx.samdec_any_order(True)
    b = ctx.samdec_decode(text, last=True)
    lists = ctx.samdec_lists()
    assert b.n == n and lists["n_records"] == n and lists["tid_runs"] == [] and lists["last_tid"] == 1
    lines = ctx.batch_lines(b)
    assert lines["tid"].tolist() == [k % 2 for k in range(n)] and lines["pos"].tolist() == [100 + k for k in range(n)]
    # fewer changes than the list holds: handed out as without the call
    ctx.samdec_begin(ci.TARGETS)
    ctx.samdec_sorted(False)
    ctx.samdec_any_order(True)
    ctx.samdec_decode(mi.sam_text(recs[:5], ci.TARGETS), last=True)
    assert ctx.samdec_lists()["tid_runs"] == [(1, 1), (2, 0), (3, 1), (4, 0)]
    ctx.samdec_begin(ci.TARGETS)                          # off again after every begin
    ctx.samdec_sorted(False)
    with pytest.raises(SeeksvError, match="not coordinate sorted"):
        ctx.samdec_decode(text, last=True)
