"""-m gpu: ssv_pairdup_retain / ssv_pairdup_rows / ssv_pairdup_mark (seeksv_amd/csrc/pairdup_kernels.h) against the plain model (tests/pairdup_model.py) on the
hand-made sets of tests/pairdup_inputs.py, each in its four orders.  The records reach the stage through the two device decoders - SAM text cut between any two
records (Context.sam_batches) and BAM files, one a batch (Context.bam_batches) - so mates land in different batches; whatever the cuts, the flags are the model's."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import bamio
import coordsort_inputs as ci
import coordsort_model as cm
import pairdup_inputs as pi
import pairdup_model as pm
from seeksv_amd import _abi, host
from seeksv_amd.device import Context, SeeksvError

pytestmark = pytest.mark.gpu

NO_SEQ = np.uint64(2 ** 64 - 1)
RETAINED = _abi.MEM_DEVICE | _abi.MEM_PERSISTENT
GROUPS = ("pairdup_ends", "pairdup_join", "pairdup_mark")
IDS = [s["name"] for s in pi.SETS]


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@pytest.fixture
def env():
    """environment variables the stage reads, taken back after the test"""
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


def bounds_of(n, n_batches):
    return [n * k // n_batches for k in range(n_batches + 1)]


def decoded(ctx, recs, targets, decoder, bounds, tmp_path=None, keep_all_seq=True):
    """generator over (Batch, Names) of the records cut at the record indices `bounds` (first 0, last len(recs)); valid until the next one"""
    parts = [recs[a:b] for a, b in zip(bounds, bounds[1:])]
    if decoder == "sam":
        texts = [pi.sam_text(p, targets) for p in parts]
        cuts = np.cumsum([len(t) for t in texts])[:-1].tolist()
        text = b"".join(texts)
        ctx.samdec_begin(targets)
        ctx.samdec_any_order(True)
        ctx.samdec_sorted(keep_all_seq)
        edges = [0] + [c for c in cuts] + [len(text)]
        for k in range(len(edges) - 1):
            yield ctx.samdec_decode(text[edges[k]:edges[k + 1]], last=k == len(edges) - 2), ctx.samdec_names()
        return
    for k, part in enumerate(parts):
        path = str(tmp_path / f"part{k}.bam")
        ci.write_bam(path, targets, [100000] * len(targets), part)      # (any number of contigs)
        with host.BamReader(path) as rd:
            for b, _ in ctx.bam_batches(rd, keep_all_seq=keep_all_seq, any_order=True):
                yield b, ctx.bamdec_names()


def retained(ctx, recs, targets, decoder, bounds, tmp_path=None):
    return [ctx.pairdup_retain(b, nm) for b, nm in decoded(ctx, recs, targets, decoder, bounds, tmp_path)]


def lines_of(ctx, batches):
    got = [ctx.batch_lines(b) for b in batches]
    return np.concatenate(got) if got else np.zeros(0, _abi.RECORD_DTYPE)


def release(ctx, batches):
    for b in batches:
        ctx.batch_release(b)


def mark_and_check(ctx, recs, batches, bits=64):
    """ssv_pairdup_mark over the batches; flags and counts against the model -> (lines, stats)"""
    want_st = {}
    want = pm.mark(recs, bits, want_st)
    st = ctx.pairdup_mark(batches)
    lines = lines_of(ctx, batches)
    assert len(lines) == len(recs)
    for col in ("tid", "pos", "mtid", "mpos"):
        assert lines[col].tolist() == [r[col] for r in recs], col
    got = lines["flag"].tolist()
    assert got == want, [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w][:10]
    assert st == want_st
    return lines, st


def read_back(ctx, b):
    """a retained batch -> (one tuple per record of everything the batch says about it, free of where it lies in the batch's arrays, the whole batch as bytes)"""
    assert b.mem == RETAINED
    lines = ctx.batch_lines(b)
    dv = _abi.Batch()
    C.memmove(C.byref(dv), C.byref(b), C.sizeof(_abi.Batch))
    dv.mem, dv.tid_runs, dv.n_tid_runs = _abi.MEM_DEVICE, None, 0      # (ssv_batch_to_host takes the plain device form)
    h = ctx.batch_to_host(dv)
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
    for i in range(int(b.n)):
        co, so = int(lines["cigar_off"][i]), int(lines["seq_off"][i])
        ops = tuple(h["cigar"][co:co + int(nc[i])].tolist())
        sq = bytes(h["seqqual"][so:so + int(sb[i])]) if has[i] else None
        out.append((canon[i].tobytes(), (int(h["tid"][i]), int(h["pos"][i]), int(h["n_cigar"][i]), int(h["cigar_ends"][i])), ops, sq))
    whole = tuple(np.asarray(h[k]).tobytes() for k in ("tid", "pos", "n_cigar", "cigar_ends", "cigar", "seqqual"))
    return out, lines, whole


# ---- the rows --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("decoder", ["sam", "bam"])
@pytest.mark.parametrize("s", pi.SETS, ids=IDS)
def test_every_row_field_of_every_record(ctx, s, decoder, tmp_path):
    for name, recs, _ in pi.orders(s):
        batches = retained(ctx, recs, s["targets"], decoder, bounds_of(len(recs), 2), tmp_path)
        rows = np.concatenate([ctx.pairdup_rows(b) for b in batches])
        want = [pm.row(r) for r in recs]
        got = list(zip(rows["name_hash"].tolist(), rows["u"].tolist(), rows["score"].tolist(), rows["kind"].tolist()))
        assert got == want, (name, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5])
        release(ctx, batches)


# ---- flags and counts against the model --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_batches", [1, 2, 3])
@pytest.mark.parametrize("s", pi.SETS, ids=IDS)
def test_flags_and_stats_for_every_set_and_order(ctx, s, n_batches, tmp_path):
    for name, recs, where in pi.orders(s):
        batches = retained(ctx, recs, s["targets"], "sam", bounds_of(len(recs), n_batches))
        lines, st = mark_and_check(ctx, recs, batches)
        if not s["claim"].get("ties"):                            # ... and the answers written by hand
            assert sorted(where[i] for i, f in enumerate(lines["flag"].tolist()) if f != recs[i]["flag"]) == s["dup"], name
        release(ctx, batches)
    if n_batches == 2:                                           # the BAM decoder, one file a batch
        recs = pi.orders(s)[3][1]
        batches = retained(ctx, recs, s["targets"], "bam", bounds_of(len(recs), 2), tmp_path)
        mark_and_check(ctx, recs, batches)
        release(ctx, batches)


@pytest.mark.parametrize("s", pi.SMALL, ids=[s["name"] for s in pi.SMALL])
def test_small_sets_cut_at_every_record(ctx, s):
    """one cut between any two records, and one record a batch: mates land in different batches"""
    for name, recs, _ in pi.orders(s):
        n = len(recs)
        for bounds in [[0, k, n] for k in range(1, n)] + [list(range(n + 1))]:
            batches = retained(ctx, recs, s["targets"], "sam", bounds)
            assert [int(b.n) for b in batches] == [b - a for a, b in zip(bounds, bounds[1:])]
            mark_and_check(ctx, recs, batches)
            release(ctx, batches)


@pytest.mark.parametrize("bits", [4, 1])
def test_narrow_name_hashes_follow_the_model(ctx, env, bits):
    env(SSV_DUP_DIGEST_BITS=bits)
    fewer = 0
    for s in pi.SETS:
        if s["targets"] is pi.BIG_TARGETS:
            continue
        for name, recs, _ in pi.orders(s):
            batches = retained(ctx, recs, s["targets"], "sam", bounds_of(len(recs), 2))
            rows = np.concatenate([ctx.pairdup_rows(b) for b in batches])
            assert rows["name_hash"].tolist() == [pm.row(r, bits)[0] for r in recs] and int(rows["name_hash"].max()) < 1 << bits
            lines, st = mark_and_check(ctx, recs, batches, bits)
            fewer += len(s["dup"]) - sum(1 for f, r in zip(lines["flag"].tolist(), recs) if f != r["flag"])
            release(ctx, batches)
    assert fewer > 0       # names that collide are name groups of more than two records: pairs that 64 bits mark are left alone


# ---- the retained batch ------------------------------------------------------------------------------------------------------------------------------------------

def clipped_sample():
    """240 single reads of 40 bases, every third soft-clipped at one end (they take no part), the two clipping forms among them, the seven-operation pair on the next contig"""
    rng = np.random.RandomState(7)
    recs = []
    for k in range(240):
        cigar = ("15S25M", "25M15S", "40M")[k % 3]
        r = pi.read(f"s{k}", 16 * (k % 2), 0, 90 + 2 * (k // 4), cigar, -1, -1, bytes(rng.randint(20, 41, 40).tolist()))
        r["seq"] = "".join("ACGT"[x] for x in rng.randint(0, 4, 40))
        recs.append(r)
    recs += pi.BY_NAME["clip_forms"]["records"] + [dict(r, qname="7" + r["qname"], tid=1, mtid=1) for r in pi.BY_NAME["cigar7"]["records"]]
    return pi.in_order(recs)[0]


def test_retained_batch_is_dup_retain_form_but_for_the_marked_flags(ctx):
    recs = clipped_sample()
    (b, nm), = decoded(ctx, recs, pi.TARGETS, "sam", [0, len(recs)])
    ctx.dup_begin()
    ref, carried = ctx.dup_retain(b, nm, last=True)               # the same decoded batch through `run -M`'s retention: its rule marks nothing here
    ctx.dup_finish()
    mine = ctx.pairdup_retain(b, nm)
    assert carried == 0 and ref.n == mine.n == len(recs)
    want_t, want_lines, want_whole = read_back(ctx, ref)
    assert want_lines["flag"].tolist() == [r["flag"] for r in recs]
    got_t, got_lines, got_whole = read_back(ctx, mine)
    assert got_lines.tobytes() == want_lines.tobytes() and got_whole == want_whole and got_t == want_t     # before the mark: the same bytes
    for f in ("n_cigar_total", "seqqual_bytes", "max_ref_span", "mem"):
        assert getattr(mine, f) == getattr(ref, f), f
    clipped = np.array([pm.cigar_ops(r)[0][1] == "S" or pm.cigar_ops(r)[-1][1] == "S" for r in recs])
    assert ((got_lines["seq_off"] != NO_SEQ) == clipped).all() and 0 < clipped.sum() < len(recs)
    lines, st = mark_and_check(ctx, recs, [mine])
    marked = np.array(pm.mark(recs)) != np.array([r["flag"] for r in recs])
    assert marked.sum() == 4
    _, after_lines, after_whole = read_back(ctx, mine)
    undone = after_lines.copy()
    undone["flag"][marked] &= ~np.uint16(0x400)
    assert undone.tobytes() == want_lines.tobytes() and after_whole == want_whole        # after it: the marked flags, nothing else
    # the clip pass reads it like any retained batch
    want = ctx.getclip([ref])
    got = ctx.getclip([mine])
    assert want["n_clusters"] > 0 and got["n_clusters"] > 0
    release(ctx, [ref, mine])


def test_tid_runs_are_the_decoders(ctx, tmp_path):
    recs = pi.BY_NAME["key_tid_a"]["records"]
    path = str(tmp_path / "in.bam")
    bamio.write_bam(path, pi.TARGETS, pi.TARGET_LENS, recs)
    with host.BamReader(path) as rd:
        for b, _ in ctx.bam_batches(rd, keep_all_seq=True):
            want = b.get_tid_runs()
            out = ctx.pairdup_retain(b, ctx.bamdec_names())
            got = out.get_tid_runs()
            assert (want is None) == (got is None) and (want is None or (want["first"].tolist(), want["tid"].tolist()) == (got["first"].tolist(), got["tid"].tolist()))
            assert want is not None
            ctx.batch_release(out)


# ---- the sort behind the mark ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["clip_forms", "reverse_ends", "unmapped_between", "group_65", "key_rev_a"])
def test_batch_sort_after_the_mark(ctx, name):
    s = pi.BY_NAME[name]
    nt = len(s["targets"])
    for order, recs, _ in pi.orders(s)[1:]:
        batches = retained(ctx, recs, s["targets"], "sam", bounds_of(len(recs), 3))
        mark_and_check(ctx, recs, batches)
        before, model = [], []
        for b in batches:
            t, lines, _ = read_back(ctx, b)
            before += t
            model += [dict(tid=int(t_), pos=int(p), flag=int(f)) for t_, p, f in zip(lines["tid"].tolist(), lines["pos"].tolist(), lines["flag"].tolist())]
        assert [r["flag"] for r in model] == pm.mark(recs)
        want = cm.order(model, nt)
        res = ctx.batch_sort(batches, nt, 50)
        after = []
        for b in res["batches"]:
            after += read_back(ctx, b)[0]
        assert res["n_records"] == len(recs) and not res["already_sorted"], order
        assert after == [before[i] for i in want], order
        release(ctx, res["batches"])


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------------------------

def test_20000_pairs_of_one_key_and_100000_unplaced_records_complete(ctx):
    """an amplicon: every pair at one key.  No pass is quadratic in the size of a group; no time is asserted (the observed one is in DESIGN.md 8d)"""
    n = 20000
    recs = []
    for k in range(n):
        recs += list(pi.pair(f"a{k}", pi.FWD100, pi.REV300, q=20 + k % 20))
    recs += [pi.read(f"u{k // 2}", 77 if k % 2 == 0 else 141, -1, -1, None, -1, -1) for k in range(100000)]
    t0 = time.perf_counter()
    batches = retained(ctx, recs, pi.TARGETS, "sam", bounds_of(len(recs), 3))
    t1 = time.perf_counter()
    st = ctx.pairdup_mark(batches)
    t2 = time.perf_counter()
    print(f"140,000 records: decode + retain {t1 - t0:.4f} s, ssv_pairdup_mark {t2 - t1:.4f} s")
    assert st == dict(records=140000, taking_part=2 * n, unpaired=0, pairs=n, groups_many=1, pairs_marked=n - 1)
    flags = lines_of(ctx, batches)["flag"].tolist()
    keeper = next(k for k in range(n) if k % 20 == 19)           # the first pair with the highest score
    want = [r["flag"] | (0x400 if i < 2 * n and i // 2 != keeper else 0) for i, r in enumerate(recs)]
    assert flags == want
    release(ctx, batches)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_batches_byte_identical(ctx, tmp_path):
    recs = pi.orders(pi.BY_NAME["reverse_ends"])[3][1]
    batches = retained(ctx, recs, pi.TARGETS, "sam", bounds_of(len(recs), 2))
    plain = [ctx.batch_retain(b) for b, _ in decoded(ctx, recs, pi.TARGETS, "sam", [0, len(recs)])]
    def snap():
        return [(lines.tobytes(), whole) for _, lines, whole in (read_back(ctx, b) for b in batches + plain)]

    def rows():
        return [ctx.pairdup_rows(b).tobytes() for b in batches]

    before, rows_before = snap(), rows()
    with pytest.raises(SeeksvError, match=r"\(-3\)"):              # a batch of ssv_batch_retain among them
        ctx.pairdup_mark(batches + plain)
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.pairdup_mark(plain)
    with pytest.raises(SeeksvError, match=r"\(-3\)"):              # one batch twice
        ctx.pairdup_mark([batches[0], batches[1], batches[0]])
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.pairdup_rows(plain[0])
    lib, h = ctx._lib, ctx._h
    arr = (_abi.Batch * 2)(*batches)
    assert lib.ssv_pairdup_mark(h, arr, 2, None) == -3 and lib.ssv_pairdup_mark(h, None, 2, C.byref(_abi.PairdupStats())) == -3
    assert lib.ssv_pairdup_mark(h, arr, -1, C.byref(_abi.PairdupStats())) == -3
    assert snap() == before and rows() == rows_before
    # retain: NULL arguments, a host batch, a record that takes part without its qualities - no batch is made, the live ones stay as they are
    (b, nm), = decoded(ctx, recs, pi.TARGETS, "sam", [0, len(recs)])
    out = _abi.Batch()
    assert lib.ssv_pairdup_retain(h, None, C.byref(nm), C.byref(out)) == -3 and lib.ssv_pairdup_retain(h, C.byref(b), None, C.byref(out)) == -3
    assert lib.ssv_pairdup_retain(h, C.byref(b), C.byref(nm), None) == -3
    hostb, keep = _abi.make_batch(ctx.batch_to_host(b))
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.pairdup_retain(hostb, [r["qname"] for r in recs])
    with pytest.raises(SeeksvError, match="without its qualities"):
        for bb, names in decoded(ctx, recs, pi.TARGETS, "bam", [0, len(recs)], tmp_path, keep_all_seq=False):
            ctx.pairdup_retain(bb, names)
    assert snap() == before and rows() == rows_before
    # ... and the mark goes on as if none of these calls had been made; a second call on the same batches is refused and changes nothing
    mark_and_check(ctx, recs, batches)
    after = snap()
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.pairdup_mark(batches)
    with pytest.raises(SeeksvError, match=r"\(-3\)"):              # the rows are dead
        ctx.pairdup_rows(batches[0])
    assert snap() == after
    # a batch released before the mark takes its rows with it: a plain batch in its place is no batch of ssv_pairdup_retain
    gone = retained(ctx, recs, pi.TARGETS, "sam", [0, len(recs)])
    release(ctx, gone)
    again = [ctx.batch_retain(b) for b, _ in decoded(ctx, recs, pi.TARGETS, "sam", [0, len(recs)])]
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.pairdup_mark(again)
    release(ctx, batches + plain + again)
    assert ctx.pairdup_mark([]) == dict(records=0, taking_part=0, unpaired=0, pairs=0, groups_many=0, pairs_marked=0)


# ---- nothing new without the stage -------------------------------------------------------------------------------------------------------------------------------

def test_no_launch_in_the_three_groups_without_the_calls(ctx):
    recs = clipped_sample()
    ctx.prof_enable(1)
    ctx.prof_reset()
    plain = [ctx.batch_retain(b) for b, _ in decoded(ctx, recs, pi.TARGETS, "sam", bounds_of(len(recs), 2))]      # plain retain + scan
    ctx.getclip(plain)
    ctx.dup_begin()                                                                                              # `run -M`'s retention
    kept = [ctx.dup_retain(b, nm)[0] for b, nm in decoded(ctx, recs, pi.TARGETS, "sam", [0, len(recs)])]
    kept.append(ctx.dup_retain(*empty_batch(), last=True)[0])
    ctx.dup_finish()
    shuffled = pi.orders(pi.BY_NAME["group_65"])[3][1]                                                           # `run -u`'s sort
    res = ctx.batch_sort([ctx.batch_retain(b) for b, _ in decoded(ctx, shuffled, pi.TARGETS, "sam", [0, 40, len(shuffled)])], len(pi.TARGETS))
    for g in GROUPS:
        assert ctx.prof_get(g)["launches"] == 0, g
    assert ctx.prof_get("clip_scan")["launches"] > 0 and ctx.prof_get("dup_retain")["launches"] > 0 and ctx.prof_get("sort_radix")["launches"] > 0
    mine = retained(ctx, shuffled, pi.TARGETS, "sam", [0, 40, len(shuffled)])
    assert ctx.prof_get("pairdup_ends")["launches"] > 0 and ctx.prof_get("pairdup_join")["launches"] == 0 and ctx.prof_get("pairdup_mark")["launches"] == 0
    ctx.pairdup_mark(mine)
    assert all(ctx.prof_get(g)["launches"] > 0 for g in GROUPS)
    ctx.prof_enable(0)
    release(ctx, plain + kept + res["batches"] + mine)


def empty_batch():
    b = _abi.Batch()
    b.mem = _abi.MEM_DEVICE
    return b, _abi.Names(_abi.MEM_DEVICE, 0, 0, None, None, 0)
