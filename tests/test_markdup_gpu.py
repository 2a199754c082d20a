"""-m gpu: ssv_dup_begin / ssv_dup_retain / ssv_dup_finish (seeksv_amd/csrc/dup_kernels.h) against the plain model (tests/markdup_model.py) on the hand-made sets
of tests/markdup_inputs.py.  The records reach the stage through the two device decoders - SAM text cut at any byte (Context.sam_batches) and BAM chunks
(Context.bam_batches) - so a seam can fall anywhere; whatever the cuts, the concatenated outputs are the input, record for record, with the model's flags."""
import os

import numpy as np
import pytest

import bamio
import markdup_inputs as mi
import markdup_model as mm
from seeksv_amd import _abi, host
from seeksv_amd.device import Context, SeeksvError

pytestmark = pytest.mark.gpu

NO_SEQ = np.uint64(2 ** 64 - 1)
IDS = [s["name"] for s in mi.SETS]


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@pytest.fixture
def env():
    """environment variables the stage reads at ssv_dup_begin, taken back after the test"""
    saved = {}

    def put(**kw):
        for k, v in kw.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ[k] = str(v)
    yield put
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def empty_batch():
    b = _abi.Batch()
    b.mem = _abi.MEM_DEVICE
    return b, _abi.Names(_abi.MEM_DEVICE, 0, 0, None, None, 0)


def line_starts(text):
    return [0] + [i + 1 for i, ch in enumerate(text) if ch == 10]


def stream(ctx, batches, last_with_data=None, keep=None):
    """the stage over (Batch, Names) pairs in file order; the stream ends with `last` on an empty batch, or on batch number last_with_data.
    -> (record lines of all outputs, [(out.n, carried)], stats); keep: a list that gets the retained batches (the caller releases them)"""
    ctx.dup_begin()
    lines, shape = [], []

    def take(out, carried):
        assert out.mem == _abi.MEM_DEVICE | _abi.MEM_PERSISTENT and not out.tid_runs
        lines.append(ctx.batch_lines(out))
        shape.append((int(out.n), carried))
        if keep is not None:
            keep.append(out)
        else:
            ctx.batch_release(out)

    for k, (b, nm) in enumerate(batches):
        take(*ctx.dup_retain(b, nm, last=k == last_with_data))
    if last_with_data is None:
        take(*ctx.dup_retain(*empty_batch(), last=True))
    return np.concatenate(lines) if lines else np.zeros(0, _abi.RECORD_DTYPE), shape, ctx.dup_finish()


def canon(lines):
    """record lines without what depends on the batch a record came out in: cigar_off, and seq_off beyond whether the bases were kept"""
    c = lines.copy()
    c["cigar_off"] = 0
    c["seq_off"] = np.where(lines["seq_off"] == NO_SEQ, NO_SEQ, np.uint64(0))
    return c.tobytes()


def check_against_model(records, lines, bits=64):
    want = mm.mark(records, bits)
    assert len(lines) == len(records)
    for col in ("tid", "pos", "mtid", "mpos"):
        assert lines[col].tolist() == [r[col] for r in records], col
    assert lines["l_qseq"].tolist() == [len(r["seq"]) for r in records]
    got = lines["flag"].tolist()
    assert got == want, [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w][:10]


def sam_stream(ctx, records, cuts, **kw):
    return stream(ctx, ctx.sam_batches(mi.sam_text(records), mi.TARGETS, cuts=cuts), **kw)


# ---- flags against the model ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", mi.SMALL, ids=[s["name"] for s in mi.SMALL])
def test_small_sets_at_every_cut(ctx, s):
    """every single cut point between two records, one record per batch, and cuts inside lines: one answer, the model's"""
    recs = s["records"]
    starts = line_starts(mi.sam_text(recs))[:-1]
    whole, shape, _ = sam_stream(ctx, recs, [])
    check_against_model(recs, whole)
    assert sum(n for n, _ in shape) == len(recs)
    for cut in starts[1:]:
        got, _, _ = sam_stream(ctx, recs, [cut])
        assert canon(got) == canon(whole), cut
    each, shape, _ = sam_stream(ctx, recs, starts[1:])
    assert canon(each) == canon(whole)
    assert len(shape) == len(recs) + 1
    inside, _, _ = sam_stream(ctx, recs, [x + 3 for x in starts] + [7, 11])   # seams inside lines: some chunks finish no record at all
    assert canon(inside) == canon(whole)
    ended, _, _ = sam_stream(ctx, recs, [starts[len(starts) // 2]], last_with_data=1)   # `last` on the batch that holds the file's end
    assert canon(ended) == canon(whole)


@pytest.mark.parametrize("s", mi.SETS, ids=IDS)
def test_sets_through_the_bam_decoder(ctx, s, tmp_path):
    recs = s["records"]
    path = str(tmp_path / "in.bam")
    bamio.write_bam(path, mi.TARGETS, mi.TARGET_LENS, recs)

    def batches():
        with host.BamReader(path) as rd:
            for b, _ in ctx.bam_batches(rd, keep_all_seq=True, chunk_inflated=1 << 16):   # one BGZF block a chunk
                yield b, ctx.bamdec_names()
    lines, shape, st = stream(ctx, batches())
    check_against_model(recs, lines)
    assert [i for i, f in enumerate(lines["flag"].tolist()) if f != recs[i]["flag"]] == s["dup"]      # ... and the answers written by hand
    if len(recs) > 1500:
        assert len(shape) > 2                                                                          # the file really came in several chunks


@pytest.mark.parametrize("name", ["run_63_one_key", "run_64_one_key", "run_65_one_key", "run_130_one_key", "run_65_distinct", "run_300_two_heads", "interleaved", "mixed"])
def test_larger_sets_cut_as_text(ctx, name):
    recs = mi.BY_NAME[name]["records"]
    text = mi.sam_text(recs)
    starts = line_starts(text)[:-1]
    whole, _, _ = sam_stream(ctx, recs, [])
    check_against_model(recs, whole)
    for cuts in ([starts[len(starts) // 2]], starts[1::7], [len(text) // 3, 2 * len(text) // 3], starts[1:len(starts) // 2:1]):
        got, _, _ = sam_stream(ctx, recs, cuts)
        assert canon(got) == canon(whole)


def test_a_batch_that_is_one_run_and_the_growing_hold_back(ctx):
    recs = mi.BY_NAME["run_65_one_key"]["records"]
    starts = line_starts(mi.sam_text(recs))[:-1]
    lines, shape, st = sam_stream(ctx, recs, starts[1:])            # one record a batch: the 65 heads are held back until the first tail arrives
    check_against_model(recs, lines)
    assert [n for n, _ in shape[:65]] == [0] * 65 and shape[65] == (65, 65)
    assert st["held_max"] == 65
    assert shape[-1][0] == 65 and shape[-1][1] == 65                # the flush on an empty batch: the 65 tails, one run
    # records with tid < 0 take no part and are not held back
    recs = mi.BY_NAME["mixed"]["records"]
    lines, shape, st = sam_stream(ctx, recs, [])
    assert shape == [(15, 0), (0, 0)] and st["held_max"] == 0


def test_an_unplaced_tail_of_100000_records_costs_no_more_than_its_copy(ctx):
    """the end of a real file: reads without a place, all at (-1, -1).  They take no part, are not selected, not grouped and not held back - the stage passes
    over them in the time of any other 100,000 records (as one run of one key in an all-pairs kernel they would be 1.6 * 10^8 steps of a single wavefront)"""
    import time
    placed = mi.BY_NAME["mixed"]["records"][:13]
    tail = [dict(qname=f"u{k // 2}", flag=77 if k % 2 == 0 else 141, tid=-1, pos=-1, mapq=0, cigar="", mtid=-1, mpos=-1, isize=0, seq="ACGTACGTAC", qual=mi.Q30) for k in range(100000)]
    recs = placed + tail
    text = mi.sam_text(recs)
    sam_stream(ctx, placed, [])                       # (buffers of the usual size are there)
    t0 = time.perf_counter()
    lines, shape, st = stream(ctx, ctx.sam_batches(text, mi.TARGETS, cuts=[len(text) // 3, 2 * len(text) // 3]))
    seconds = time.perf_counter() - t0
    check_against_model(recs, lines)
    assert st["held_max"] <= 2 and st["groups"] == 3 and st["heads_marked"] == 3
    assert seconds < 5.0, seconds
    # a deep pile of placed records that take no part, two heads among them: tiles without a head are passed over
    pile = [mi.rec(f"f{k}", 0, 2000, 0, 9000, mi.HEAD & ~0x1) for k in range(50000)]
    recs = pile[:20000] + [mi.rec("k", 0, 2000, 0, 9000, mi.HEAD)] + pile[20000:] + [mi.rec("d", 0, 2000, 0, 9000, mi.HEAD), mi.rec("k", 0, 9000, 0, 2000, mi.TAIL), mi.rec("d", 0, 9000, 0, 2000, mi.TAIL)]
    t0 = time.perf_counter()
    lines, shape, st = sam_stream(ctx, recs, [])
    seconds = time.perf_counter() - t0
    check_against_model(recs, lines)
    assert [i for i, f in enumerate(lines["flag"].tolist()) if f & 0x400] == [50001, 50003] and seconds < 5.0, seconds


def test_a_tail_two_batches_behind_its_head(ctx):
    recs = mi.BY_NAME["mixed"]["records"]
    starts = line_starts(mi.sam_text(recs))[:-1]
    # b's head is record 1, its tail record 7: batches [0, 4) [4, 6) [6, 8) ...
    lines, shape, _ = sam_stream(ctx, recs, [starts[4], starts[6], starts[8], starts[11]])
    check_against_model(recs, lines)
    assert lines["flag"][1] & 0x400 and lines["flag"][7] & 0x400 and len(shape) == 6


# ---- the set ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_digest_set_grows(ctx, env):
    env(SSV_DUP_SET_SLOTS=16)
    recs = mi.BY_NAME["run_1000_one_key"]["records"]
    text = mi.sam_text(recs)
    starts = line_starts(text)[:-1]
    for cuts in ([], starts[100::100]):
        lines, _, st = sam_stream(ctx, recs, cuts)
        check_against_model(recs, lines)
        assert st["set_entries"] == 999 and st["heads_marked"] == 999 and st["tails_marked"] == 999
    recs = mi.BY_NAME["interleaved"]["records"]                      # forty inserts of one digest each, one batch a place: 16 slots hold 8
    lines, _, st = sam_stream(ctx, recs, line_starts(mi.sam_text(recs))[4:-1:4])
    check_against_model(recs, lines)
    assert st["set_entries"] == 40


@pytest.mark.parametrize("bits", [4, 1])
def test_narrow_digests_follow_the_model(ctx, env, bits):
    env(SSV_DUP_DIGEST_BITS=bits)
    more = 0
    for s in mi.SETS:
        if len(s["records"]) > 400:
            continue
        recs = s["records"]
        lines, _, st = sam_stream(ctx, recs, [])
        check_against_model(recs, lines, bits)
        more += sum(1 for f, r in zip(lines["flag"].tolist(), recs) if f != r["flag"]) - len(s["dup"])
        stats = {}
        mm.mark(recs, bits, stats)
        assert st["set_entries"] == stats["set_entries"] <= 1 << bits
        if s["name"] in ("interleaved", "mixed"):
            starts = line_starts(mi.sam_text(recs))[:-1]
            cut, _, _ = sam_stream(ctx, recs, starts[1::3])
            assert canon(cut) == canon(lines)
    assert more > 0       # the collisions did mark tails that 64 bits leave alone


@pytest.mark.parametrize("s", mi.SETS, ids=IDS)
def test_stats(ctx, s):
    lines, shape, st = sam_stream(ctx, s["records"], [])
    want = {}
    mm.mark(s["records"], stats=want)
    held = st.pop("held_max")
    assert st == want
    last = s["records"][-1]
    trailing = 0 if last["tid"] < 0 else next(e - b for b, e in reversed(mm.runs(s["records"])))
    assert held == trailing


# ---- the retained batch ------------------------------------------------------------------------------------------------------------------------------------------

def clipped_sample():
    """300 single reads (they take no part: nothing is marked) of 40 bases, every third soft-clipped at one end, and twenty pairs among them"""
    rng = np.random.RandomState(5)
    recs = []
    for k in range(300):
        seq = "".join("ACGT"[x] for x in rng.randint(0, 4, 40))
        cigar = ("15S25M", "25M15S", "40M")[k % 3]
        pos = 1000 + 5 * (k // 6)
        recs.append(dict(qname=f"s{k}", flag=16 * (k % 2), tid=0, pos=pos, mapq=60, cigar=cigar, mtid=-1, mpos=-1, isize=0, seq=seq, qual=bytes(rng.randint(20, 41, 40).tolist())))
    for k in range(20):
        h, t = mi.pair(f"p{k}", 0, 1100 + k, 0, 3000 + k)
        recs += [h, t]
    return mi.in_order(recs)[0]


def test_retained_batch_form_and_clip_table(ctx):
    recs = clipped_sample()
    text = mi.sam_text(recs)
    starts = line_starts(text)[:-1]
    cuts = starts[50::50]
    plain = [ctx.batch_retain(b) for b, _ in ctx.sam_batches(text, mi.TARGETS, cuts=cuts)]
    want = ctx.getclip(plain)
    kept = []
    lines, shape, st = stream(ctx, ctx.sam_batches(text, mi.TARGETS, cuts=cuts), keep=kept)
    check_against_model(recs, lines)
    assert st["heads_marked"] == 0 and st["taking_part"] == 40
    clipped = np.array(["S" in r["cigar"] for r in recs])
    assert ((lines["seq_off"] != NO_SEQ) == clipped).all()                # bases and qualities stay for the soft-clipped records only
    assert sum(int(b.seqqual_bytes) for b in kept) == int(clipped.sum()) * 60
    assert sum(int(b.n_cigar_total) for b in kept) == sum(2 if c else 1 for c in clipped)
    got = ctx.getclip([b for b in kept if b.n])
    assert want["n_clusters"] == got["n_clusters"] > 0
    for name in ("tid", "pos", "side", "support", "left_len", "right_len", "str", "cigar"):
        assert np.array_equal(want[name], got[name]), name
    for b in plain + kept:
        ctx.batch_release(b)


# ---- errors --------------------------------------------------------------------------------------------------------------------------------------------------------

def one_batch(ctx, records):
    return next(iter(ctx.sam_batches(mi.sam_text(records), mi.TARGETS)))


def test_abi_errors_leave_the_stream_as_it_was(ctx, tmp_path):
    recs = mi.BY_NAME["mixed"]["records"]
    ctx.dup_begin()
    ctx.dup_finish()
    with pytest.raises(SeeksvError, match=r"\(-4\)"):                      # no ssv_dup_begin
        ctx.dup_retain(*one_batch(ctx, recs))
    with pytest.raises(SeeksvError, match=r"\(-4\)"):
        ctx.dup_finish()
    ctx.dup_begin()
    b, nm = one_batch(ctx, recs)
    hostb, keep = _abi.make_batch(ctx.batch_to_host(b))
    with pytest.raises(SeeksvError, match=r"\(-3\)"):                      # a host batch
        ctx.dup_retain(hostb, [r["qname"] for r in recs])
    lib, h = ctx._lib, ctx._h
    out, carried = _abi.Batch(), _abi.C.c_int64()
    assert lib.ssv_dup_retain(h, None, _abi.C.byref(nm), 0, _abi.C.byref(out), _abi.C.byref(carried)) == -3
    assert lib.ssv_dup_retain(h, _abi.C.byref(b), None, 0, _abi.C.byref(out), _abi.C.byref(carried)) == -3
    assert lib.ssv_dup_retain(h, _abi.C.byref(b), _abi.C.byref(nm), 0, None, _abi.C.byref(carried)) == -3
    assert lib.ssv_dup_retain(h, _abi.C.byref(b), _abi.C.byref(nm), 0, _abi.C.byref(out), None) == -3
    assert lib.ssv_dup_finish(h, None) == -3
    # (tid, pos) goes down inside a batch, and against the held-back run
    with pytest.raises(SeeksvError, match="not coordinate sorted"):
        ctx.dup_retain(*one_batch(ctx, mi.UNSORTED))
    first, carried1 = ctx.dup_retain(*one_batch(ctx, recs[4:7]))            # c0:400 f g | c0:900 a' - a' is held back
    assert (first.n, carried1) == (2, 0)
    with pytest.raises(SeeksvError, match="not coordinate sorted"):
        ctx.dup_retain(*one_batch(ctx, recs[0:2]))
    # a record that takes part without its qualities
    path = str(tmp_path / "in.bam")
    bamio.write_bam(path, mi.TARGETS, mi.TARGET_LENS, recs[7:])
    with host.BamReader(path) as rd:
        for bb, _ in ctx.bam_batches(rd, keep_all_seq=False):
            with pytest.raises(SeeksvError, match="without its qualities"):
                ctx.dup_retain(bb, ctx.bamdec_names())
    # ... and the stream goes on as if none of these calls had been made
    second, carried2 = ctx.dup_retain(*one_batch(ctx, recs[7:]), last=True)
    assert (second.n, carried2) == (9, 1)
    lines = np.concatenate([ctx.batch_lines(first), ctx.batch_lines(second)])
    check_against_model(recs[4:], lines)
    with pytest.raises(SeeksvError, match=r"\(-4\)"):                      # a call after `last`
        ctx.dup_retain(*empty_batch())
    st = ctx.dup_finish()
    assert st["records"] == 11 and st["held_max"] == 1
    ctx.batch_release(first)
    ctx.batch_release(second)


# ---- nothing new without the stage -------------------------------------------------------------------------------------------------------------------------------

def test_no_launch_in_the_dup_groups_for_a_plain_retain_and_scan(ctx):
    recs = clipped_sample()
    text = mi.sam_text(recs)
    ctx.prof_enable(1)
    ctx.prof_reset()
    plain = [ctx.batch_retain(b) for b, _ in ctx.sam_batches(text, mi.TARGETS)]
    ctx.getclip(plain)
    for g in ("dup_select", "dup_mark", "dup_retain"):
        assert ctx.prof_get(g)["launches"] == 0, g
    assert ctx.prof_get("clip_scan")["launches"] > 0
    kept = []
    stream(ctx, ctx.sam_batches(mi.sam_text(mi.BY_NAME["mixed"]["records"]), mi.TARGETS), keep=kept)
    assert all(ctx.prof_get(g)["launches"] > 0 for g in ("dup_select", "dup_mark", "dup_retain"))
    ctx.prof_enable(0)
    for b in plain + kept:
        ctx.batch_release(b)
