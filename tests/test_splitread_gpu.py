"""-m gpu: the split-read session of `seeksv run -A` (ssv_rt_begin_original, seeksv_amd/csrc/splitread_kernels.h) against the plain model
(tests/splitread_model.py) and the answers written out in tests/splitread_inputs.py: every field of every pair, the seqs, the CIGAR sources and the six
counts - as one host batch, cut at every record, through both device decoders in their default form, with the name hash cut to 4 bits; an ssv_rt_begin
session beside it (equal on the agreement set; on hard-clipped input what it always was); the error sequence; which kernel groups run."""
import ctypes as C
import os

import pytest

import bamio
import readthrough_model as RM
import sam_text as ST
import splitread_inputs as SI
import splitread_model as SM
from seeksv_amd import _abi, host
from seeksv_amd.device import Context, SeeksvError

pytestmark = pytest.mark.gpu

SETS = SI.all_sets()
IDS = [s["name"] for s in SETS]


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def combined():
    """(records, rows, counts) of all sets side by side: as host batches, and as a file holds them - the model's answer, computed once"""
    out = {}
    for form in (False, True):
        records, rows, counts = SI.combined(file_form=form)
        b, names = SI.batch_of(records)
        assert SM.find_pairs([b], [names], 1, SI.CONTIGS) == (rows, counts)
        out[form] = (records, rows, counts)
    return out


def six(stats):
    return {k: stats[k] for k in SM.COUNTS}


def session(ctx, batches, names, min_mapq=1):
    rows, stats = ctx.readthrough_original(batches, names, min_mapq, SI.CONTIGS, raw=True)
    return rows, six(stats)


def same_rows(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def host_batches(records, cuts=()):
    b, names = SI.batch_of(records)
    return RM.split(dict(batch=b, qnames=names), list(cuts))


@pytest.mark.parametrize("s", SETS, ids=IDS)
def test_set_as_one_host_batch(ctx, s):
    rows, counts = session(ctx, *host_batches(s["records"]))
    same_rows(rows, s["rows"])
    assert counts == s["counts"]


@pytest.mark.parametrize("s", [s for s in SETS if len(s["records"]) <= 12], ids=[s["name"] for s in SETS if len(s["records"]) <= 12])
def test_set_cut_at_every_record(ctx, s):
    for cut in range(1, len(s["records"])):
        rows, counts = session(ctx, *host_batches(s["records"], [cut]))
        same_rows(rows, s["rows"])
        assert counts == s["counts"], cut


def test_all_sets_in_one_input_and_in_pieces(ctx, combined):
    records, want, want_counts = combined[False]
    n = len(records)
    for cuts in ([], [1], [n // 3, n // 3, 2 * n // 3], list(range(7, n, 7))):          # (an empty batch among them)
        rows, counts = session(ctx, *host_batches(records, cuts))
        same_rows(rows, want)
        assert counts == want_counts


def decoded(ctx, records, decoder, bounds, tmp_path):
    """generator over (Batch, Names) of the records cut at `bounds`, through a device decoder in the form `seeksv run` decodes its input (keep_all_seq off)"""
    parts = [records[a:b] for a, b in zip(bounds, bounds[1:])]
    if decoder == "sam":
        texts = [ST.text(p, SI.CONTIGS, SI.LENS, with_header=False).encode() for p in parts]
        ctx.samdec_begin(SI.CONTIGS)
        ctx.samdec_any_order(True)
        ctx.samdec_sorted(False)
        for k, t in enumerate(texts):
            yield ctx.samdec_decode(t, last=k == len(texts) - 1), ctx.samdec_names()
        return
    for k, part in enumerate(parts):
        path = str(tmp_path / f"part{k}.bam")
        bamio.write_bam(path, SI.CONTIGS, SI.LENS, part)
        with host.BamReader(path) as rd:
            for b, _ in ctx.bam_batches(rd, keep_all_seq=False, any_order=True):
                yield b, ctx.bamdec_names()


@pytest.mark.parametrize("decoder", ["bam", "sam"])
@pytest.mark.parametrize("n_batches", [1, 4])
def test_through_the_device_decoders(ctx, combined, tmp_path, decoder, n_batches):
    records, want, want_counts = combined[True]
    n = len(records)
    ctx.rt_begin_original(1, SI.CONTIGS)
    for b, nm in decoded(ctx, records, decoder, [n * k // n_batches for k in range(n_batches + 1)], tmp_path):
        ctx.rt_scan(b, nm)
    rows = ctx.rt_decode(ctx.rt_finish(), SI.CONTIGS)
    same_rows(rows, want)
    assert six(ctx.rt_original_stats()) == want_counts


def test_names_that_collide_under_four_hash_bits(ctx, combined):
    records, want, want_counts = combined[False]
    saved = os.environ.get("SSV_RT_HASH_BITS")
    os.environ["SSV_RT_HASH_BITS"] = "4"
    try:
        n = len(records)
        for cuts in ([], [n // 2]):
            rows, counts = session(ctx, *host_batches(records, cuts))
            same_rows(rows, want)
            assert counts == want_counts
    finally:
        if saved is None:
            os.environ.pop("SSV_RT_HASH_BITS", None)
        else:
            os.environ["SSV_RT_HASH_BITS"] = saved


@pytest.mark.parametrize("min_mapq", [0, 1, 31])
def test_agreement_set_both_sessions_give_the_same_pairs(ctx, min_mapq):
    records = SI.agreement(0)["records"] + SI.filler(20)
    for order in (records, SI.coordinate_sorted(records)):
        batches, names = host_batches(order, [len(order) // 2])
        want, n_cand = RM.find_junction(batches, names, min_mapq, SI.CONTIGS)
        old, old_cand = ctx.readthrough(batches, names, min_mapq, SI.CONTIGS, raw=True)
        new, counts = session(ctx, batches, names, min_mapq)
        same_rows(old, want)
        same_rows(new, want)
        assert old_cand == n_cand and counts == dict(candidates=n_cand, hard_clipped=0, pairs=len(want), pairs_borrowed=0, dropped_no_carrier=0, dropped_length=0)


def test_rt_begin_session_on_hard_clipped_input_is_what_it_was(ctx, combined):
    """FindJunction's rule drops every record with H at an end and pairs by name alone: readthrough_model says what that gives"""
    records, new_rows, _ = combined[True]
    batches, names = host_batches(records, [len(records) // 2])
    want, n_cand = RM.find_junction(batches, names, 1, SI.CONTIGS)
    got, got_cand = ctx.readthrough(batches, names, 1, SI.CONTIGS, raw=True)
    same_rows(got, want)
    assert got_cand == n_cand and [r["records"] for r in want] != [r["records"] for r in new_rows]
    with pytest.raises(SeeksvError, match=r"\(-4\)"):                        # ... and leaves no counts behind
        ctx.rt_original_stats()


def test_error_sequence(ctx):
    lib, h = ctx._lib, ctx._h
    batches, names = host_batches(SI.worked()["records"])
    with Context(0) as fresh, pytest.raises(SeeksvError, match=r"\(-4\)"):
        fresh.rt_original_stats()                                            # no session at all
    assert lib.ssv_rt_begin_original(h, None) == -3
    assert lib.ssv_rt_begin_original(None, None) == -3
    bad = _abi.RtParams(1, 2, None)                                          # contigs without their ranks
    assert lib.ssv_rt_begin_original(h, C.byref(bad)) == -3
    ctx.rt_begin_original(1, SI.CONTIGS)
    with pytest.raises(SeeksvError, match=r"\(-4\)"):                        # not finished yet
        ctx.rt_original_stats()
    ctx.rt_scan(batches[0], names[0])
    r = ctx.rt_finish()
    assert r.n_pairs == 3 and six(ctx.rt_original_stats()) == SI.worked()["counts"]
    assert six(ctx.rt_original_stats()) == SI.worked()["counts"]               # asking twice is fine
    assert lib.ssv_rt_original_stats(h, None) == -3
    with pytest.raises(SeeksvError, match=r"\(-4\)"):
        ctx.rt_scan(batches[0], names[0])                                    # the session is over
    with pytest.raises(SeeksvError, match=r"\(-4\)"):
        ctx.rt_finish()
    ctx.rt_begin_original(1, SI.CONTIGS)                                     # a new session takes the counts away
    with pytest.raises(SeeksvError, match=r"\(-4\)"):
        ctx.rt_original_stats()
    r = ctx.rt_finish()                                                      # an empty session
    assert r.n_pairs == 0 and r.n_candidates == 0 and six(ctx.rt_original_stats()) == dict.fromkeys(SM.COUNTS, 0)


def test_each_mode_runs_its_own_groups(ctx):
    batches, names = host_batches(SI.kinds_hard()["records"])
    ctx.prof_enable(1)
    ctx.prof_reset()
    ctx.readthrough(batches, names, 1, SI.CONTIGS)
    assert ctx.prof_get("rt_scan")["launches"] == 1 and ctx.prof_get("rt_finish")["launches"] == 1
    assert ctx.prof_get("splitread_scan")["launches"] == 0 and ctx.prof_get("splitread_finish")["launches"] == 0
    ctx.prof_reset()
    session(ctx, batches, names)
    assert ctx.prof_get("rt_scan")["launches"] == 0 and ctx.prof_get("rt_finish")["launches"] == 0
    assert ctx.prof_get("splitread_scan")["launches"] == 1 and ctx.prof_get("splitread_finish")["launches"] == 1
    ctx.prof_enable(0)
