"""-m gpu: the narrow wire form of the compact cluster table (6-byte rows, position escapes, CIGAR kinds; seeksv_amd/csrc/table_wire.h) changes nothing
a caller sees.  Every input is packed three times - as it comes, with SSV_TABLE_WIRE=wide (the columns themselves cross) and in format 0 - and the first
two must agree byte for byte in every handed-out and every expanded array, both must be the ASCII table, and the bytes that crossed must be fewer and add up."""
import os

import numpy as np
import pytest

import golden_util as G
from seeksv_amd import _abi, host
from test_hip_golden import _compact_checks
from test_oracle_golden import GETCLIP_CASES

pytestmark = pytest.mark.gpu

M, I, D, N, S, H, P, EQ, X = range(9)
PIECES = ("rows", "flags", "cigar", "runs", "base_exc", "pos_esc", "str")


@pytest.fixture(scope="module")
def ctx():
    from seeksv_amd.device import Context
    c = Context(0)
    yield c
    c.close()


# ---- crafted batches: reads cut out of one pseudo-random genome per contig, so that reads on one start agree where they overlap ----

def craft(reads):
    """reads: (tid, pos0, [(length, op), ...], has_qualities) -> a host batch, coordinate sorted"""
    reads = sorted(reads, key=lambda r: (r[0], r[1]))
    n = len(reads)
    rng = np.random.default_rng(7)
    genome = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, 1 << 16)]
    qgen = np.array([12, 23, 30, 37], np.uint8)[rng.integers(0, 4, 1 << 16)]
    seq_off, blobs, cig, nc, lqs, span, o = [], [], [], [], [], 1, 0
    for tid, pos0, ops, has_q in reads:
        lq = sum(l for l, op in ops if op in (M, I, S, EQ, X))
        lead = ops[0][0] if ops[0][1] == S else 0
        j = (pos0 - lead + 7919 * tid + np.arange(lq + (lq & 1))) % len(genome)
        codes = genome[j]
        packed = ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8)
        q = qgen[j[:lq]] if has_q else np.full(lq, 0xff, np.uint8)
        seq_off.append(o); blobs += [packed, q]; o += len(packed) + lq
        cig += [(l << 4) | op for l, op in ops]; nc.append(len(ops)); lqs.append(lq)
        span = max(span, sum(l for l, op in ops if op in (M, D, N, EQ, X)))
    nc = np.asarray(nc, np.int64)
    tid = np.asarray([r[0] for r in reads], np.int32)
    pos = np.asarray([r[1] for r in reads], np.int32)
    return dict(tid=tid, pos=pos, flag=np.full(n, 99, np.uint16), mapq=np.full(n, 60, np.uint8), n_cigar=nc.astype(np.uint16), l_qseq=np.asarray(lqs, np.int32), mtid=tid,
                mpos=(pos + 200).astype(np.int32), isize=np.full(n, 250, np.int32), xc=np.zeros(n, np.uint8), cigar=np.asarray(cig, np.uint32), cigar_off=(np.cumsum(nc) - nc).astype(np.uint32),
                seq_off=np.asarray(seq_off, np.uint64), seqqual=np.concatenate(blobs + [np.zeros(16, np.uint8)]), max_ref_span=int(span))


L5, L3 = [(20, S), (30, M)], [(30, M), (20, S)]


def filler(n, tid=0, start=1000, step=37):
    """n reads, `20S30M` and `30M20S` in turn: both sides fill, one event per read"""
    return [(tid, start + step * k, L5 if k % 2 == 0 else L3, True) for k in range(n)]


def stack(n, tid, pos0, ops=L5):
    return [(tid, pos0, ops, True)] * n


def crafted(name):
    if name == "gaps":       # neighbouring clusters of one run 65534 / 65535 / 65536 bases apart (on both sides), among enough others for several tiles
        far = [(0, p, ops, True) for p, ops in ((400000, L5), (400000 + 65534, L5), (400000 + 65534 + 65535, L5), (400000 + 65534 + 65535 + 65536, L5),
                                                (700000, L3), (700000 + 65534, L3), (700000 + 65534 + 65535, L3), (700000 + 65534 + 65535 + 65536, L3))]
        return filler(700) + far
    if name == "contigs":    # runs on several contigs and both sides, two of them of a cluster or two
        return filler(300, 0) + filler(4, 1, 500) + filler(260, 3) + filler(150, 7, 90000, 3)
    if name == "tile_edge":  # one side only (sorted slot = read): slots 236 .. 275 are one bin - the second tile's first twenty slots hold no cluster
        return [(0, 1000 + 11 * k, L5, True) for k in range(236)] + stack(40, 0, 5000) + [(0, 6000 + 11 * k, L5, True) for k in range(500)]
    if name in ("len255", "len256"):
        x = int(name[3:])
        return filler(600) + [(0, 30000, [(x, S), (300 - x, M)], True), (0, 30100, [(300 - x, M), (x, S)], True), (0, 30200, [(255, S), (45, M)], True)]
    if name in ("support254", "support255", "support256"):
        return filler(500) + stack(int(name[7:]), 0, 40000) + filler(100, 0, 50000)
    if name == "cigars":
        kinds = [[(20, S), (30, M)], [(30, M), (20, S)], [(10, S), (30, M), (10, S)], [(5, S), (10, M), (2, I), (10, M), (3, D), (10, M), (13, S)], [(5, H), (10, S), (30, M)],
                 [(20, S), (30, EQ)], [(10, S), (20, EQ), (5, X), (15, M)], [(30, X), (20, S)], [(12, S), (18, M), (400, N), (20, M)], [(50, S)], [(25, M), (3, D), (25, S)]]
        return [(0, 1000 + 29 * k, kinds[k % len(kinds)], True) for k in range(800)]
    if name == "consensus":  # two and three reads on one start whose clips differ in length: the cluster's lengths are the consensus', its CIGAR one record's
        r = filler(400)
        for k in range(120):
            r += [(1, 2000 + 90 * k, [(20, S), (30, M)], True), (1, 2000 + 90 * k, [(30, S), (30 + k % 3, M)], True)] + ([(1, 2000 + 90 * k, [(25, S), (40, M)], True)] if k % 4 == 0 else [])
        return r
    if name == "noqual":
        return [(0, 1000 + 31 * k, L5 if k % 2 else L3, k % 3 != 0) for k in range(700)] + [(0, 60000, L5, False)] * 3 + [(0, 61000, L5, k == 1) for k in range(3)]
    raise KeyError(name)


CRAFTED = ["gaps", "contigs", "tile_edge", "len255", "len256", "support254", "support255", "support256", "cigars", "consensus", "noqual"]


# ---- one input, three tables ----

def raw_arrays(t):
    """the handed-out arrays of a format-3 table, as bytes"""
    import ctypes as C
    n = int(t.n_clusters)

    def raw(ptr, nbytes):
        if not nbytes:
            return b""
        return bytes((C.c_uint8 * nbytes).from_address(ptr if isinstance(ptr, int) else C.cast(ptr, C.c_void_p).value))
    return dict(pos=raw(t.pos, 4 * n), c_len=raw(t.c_len, 2 * n * t.len_bytes), c_support=raw(t.c_support, n * t.support_bytes), c_ncig=raw(t.c_ncig, n * t.ncig_bytes), c_flags=raw(t.c_flags, n),
                c_cigar=raw(t.c_cigar, int(t.cigar_ops) * t.cigar_bytes), str=raw(t.str, int(t.str_bytes)), runs=raw(t.runs, 16 * int(t.n_runs)), base_exc=raw(t.base_exc, 8 * int(t.n_base_exc)),
                widths=(int(t.len_bytes), int(t.support_bytes), int(t.ncig_bytes), int(t.cigar_bytes), int(t.base_bits), int(t.qual_bits), int(t.qual_group), int(t.n_clusters), int(t.n_events)))


EXPANDED = (("tid", np.int32), ("side", np.uint8), ("support", np.int32), ("left_len", np.int32), ("right_len", np.int32), ("qual_missing", np.uint8), ("str_off", np.uint64),
            ("cigar_off", np.uint64), ("n_cigar", np.int32))


def expanded_arrays(t):
    n = int(t.n_clusters)
    assert all(bool(getattr(t, k)) for k, _ in EXPANDED) or n == 0
    d = {k: np.ctypeslib.as_array(getattr(t, k), shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dt) for k, dt in EXPANDED}
    d["support_sum"] = int(t.support_sum)
    return d


def scan(ctx, batches, kw):
    ctx.clip_begin(**kw)
    for b in batches:
        ctx.clip_scan(b)


def check_wire(w, t):
    """the reported bytes add up, and the pieces that cross as they are handed out are the table's"""
    n = int(t.n_clusters)
    assert w["total"] == sum(w[k] for k in PIECES)
    assert w["str"] == t.str_bytes and w["flags"] == n and w["runs"] == 16 * t.n_runs and w["base_exc"] == 8 * t.n_base_exc
    if w["narrow"]:
        assert w["rows"] == 6 * n and w["cigar"] <= t.cigar_ops * t.cigar_bytes and w["pos_esc"] >= 8 * t.n_runs
    else:
        assert w["rows"] == n * (4 + 2 * t.len_bytes + t.support_bytes + t.ncig_bytes) and w["cigar"] == t.cigar_ops * t.cigar_bytes and w["pos_esc"] == 0


def three_tables(ctx, batches, kw, monkeypatch, expect_narrow=None):
    ref = ctx.getclip(batches, **kw)
    ctx.clip_table_format(3)
    try:
        out = []
        for wide in (False, True):
            if wide:
                monkeypatch.setenv("SSV_TABLE_WIRE", "wide")
            else:
                monkeypatch.delenv("SSV_TABLE_WIRE", raising=False)
            scan(ctx, batches, kw)
            t = ctx.clip_cluster(as_dict=False)
            d = host.table_to_dict(t)
            w = ctx.clip_table_wire_bytes(t)
            if t.n_clusters:
                check_wire(w, t)
            _compact_checks(ctx, d, ref, t, check_size=False)   # == the ASCII table, column by column and string by string; expands t
            out.append((raw_arrays(t), expanded_arrays(t), w, d))
    finally:
        monkeypatch.delenv("SSV_TABLE_WIRE", raising=False)
        ctx.clip_table_format(0)
    (ra, xa, wa, d), (rb, xb, wb, _) = out
    assert wb["narrow"] == 0
    for k in ra:
        assert ra[k] == rb[k], k
    for k in xa:
        assert np.array_equal(xa[k], xb[k]), k
    if expect_narrow is None:   # what a row holds (table_wire.h)
        expect_narrow = ref["n_clusters"] > 0 and max(ref["left_len"].max(), ref["right_len"].max()) <= 255 and ref["support"].max() <= 254 and ref["n_cigar"].max() <= 63
    assert bool(wa["narrow"]) == bool(expect_narrow)
    if wa["narrow"]:
        assert wa["total"] < wb["total"]
    else:
        assert wa == wb
    return ref, d, wa, wb


@pytest.mark.parametrize("sub,bam,prefix,kw", [c for c in GETCLIP_CASES if c[2] != "unsorted"], ids=[c[2] for c in GETCLIP_CASES if c[2] != "unsorted"])
def test_wire_golden_cases(ctx, monkeypatch, sub, bam, prefix, kw):
    batches = host.read_bam(os.path.join(G.GOLDEN, sub, bam), 1 << 20)[2]
    three_tables(ctx, batches, kw, monkeypatch)


@pytest.mark.parametrize("read_len", [150, 400])
def test_wire_synthetic_reads(ctx, monkeypatch, read_len):
    from seeksv_amd import synth
    w = synth.Workload(genome_frac=1 / 4096, depth=30, n_sv=12, read_len=read_len)
    ref, d, wa, wb = three_tables(ctx, [w.generate_host(0, w.n_total)], {}, monkeypatch)
    if read_len == 150:   # the flagship's shape: the small columns and the CIGARs shrink to less than half
        small = lambda x: x["total"] - x["str"]
        assert wa["narrow"] == 1 and small(wa) < 0.5 * small(wb)


@pytest.mark.parametrize("name", CRAFTED)
def test_wire_crafted(ctx, monkeypatch, name):
    b = craft(crafted(name))
    ref, d, wa, wb = three_tables(ctx, [b], {}, monkeypatch)
    ll, lr, sup, nc, cg, co = ref["left_len"], ref["right_len"], ref["support"], ref["n_cigar"], ref["cigar"], ref["cigar_off"].astype(np.int64)
    assert ref["n_events"] > 512   # several tiles of 256 sorted slots
    if name == "gaps":
        steps = np.diff(ref["pos"])[(np.diff(ref["tid"]) == 0) & (np.diff(ref["side"].astype(int)) == 0)]
        assert all(int((steps == s).sum()) == 2 for s in (65534, 65535, 65536)) and wa["narrow"] == 1
        assert wa["pos_esc"] > wb["pos_esc"] == 0
    if name == "contigs":
        assert len(d["runs"]) == 8 and wa["narrow"] == 1 and np.diff(np.append(d["runs"]["first"], ref["n_clusters"])).min() <= 2
    if name == "tile_edge":
        assert sup.max() == 40 and ref["n_clusters"] == ref["n_events"] - 39 and wa["narrow"] == 1
    if name.startswith("len"):
        assert max(ll.max(), lr.max()) == int(name[3:]) and wa["narrow"] == (1 if name == "len255" else 0)
    if name.startswith("support"):
        assert sup.max() == int(name[7:]) and wa["narrow"] == (1 if name == "support254" else 0)
    if name == "cigars":
        assert nc.max() == 7 and wa["narrow"] == 1 and 0 < wa["cigar"] < wb["cigar"]
    if name == "consensus":
        two = np.flatnonzero((nc == 2) & (sup > 1))
        assert any((cg[co[k]] >> 4) != ll[k] or (cg[co[k] + 1] >> 4) != lr[k] for k in two) and wa["narrow"] == 1
    if name == "noqual":
        assert ref["qual_missing"].sum() > 200 and wa["narrow"] == 1


# ---- tables in flight ----

def _collect(c, prev):
    t = c.clip_table_wait(prev=prev)
    pre = bool(t.tid)          # the helper thread has built the expanded columns already
    c.clip_table_expand(t, 2)
    return raw_arrays(t), expanded_arrays(t), pre


def _pipeline(monkeypatch, expand_first, env=()):
    """two tables of different size and a pass without clusters through clip_cluster_async / wait_prev / wait on a context of its own -> what was handed out"""
    from seeksv_amd.device import Context
    for k, v in env:
        monkeypatch.setenv(k, v)
    big, small = craft(crafted("cigars")), craft(filler(90) + stack(5, 0, 9000))
    none = craft([(0, 1000 + 10 * k, [(50, M)], True) for k in range(300)])
    c = Context(0)
    try:
        c.clip_table_format(3)
        if expand_first:
            scan(c, [small], {})
            c.clip_table_expand(c.clip_cluster(as_dict=False), 2)
        scan(c, [big], {}); na, _ = c.clip_cluster_async()
        scan(c, [small], {}); nb, _ = c.clip_cluster_async()
        a, b = _collect(c, True), _collect(c, False)
        scan(c, [none], {}); n0, e0 = c.clip_cluster_async()
        assert (n0, e0) == (0, 0) and c.clip_table_wait().n_clusters == 0
        b2 = _collect(c, True)   # still valid: one cluster call ago
        scan(c, [big], {}); c.clip_cluster_async()
        a2 = _collect(c, False)
        assert a[0]["widths"][7] == na and b[0]["widths"][7] == nb and na > nb > 0
        assert a[2] == b[2] == expand_first and a2[2]   # (queued before / after the context's first expand)
        for x, y in ((a, a2), (b, b2)):
            assert x[0] == y[0] and all(np.array_equal(x[1][k], y[1][k]) for k in x[1])
        return a, b
    finally:
        c.close()


@pytest.fixture(scope="module")
def pipeline_ref():
    """the same two tables with the columns themselves crossing, computed once"""
    mp = pytest.MonkeyPatch()
    try:
        return _pipeline(mp, False, (("SSV_TABLE_WIRE", "wide"),))
    finally:
        mp.undo()


@pytest.mark.parametrize("expand_first", [False, True])
@pytest.mark.parametrize("path", ["link", "hip", "refuse"])
def test_wire_pipelined(monkeypatch, pipeline_ref, expand_first, path):
    """... on the named copy engine, on the runtime's copies (SSV_LINK_COPY=hip), and with an engine that takes two pieces of a table and refuses the third
    (SSV_LINK_REFUSE_AFTER=2): both variables are read by the context under test, which is created here"""
    env = {"link": (), "hip": (("SSV_LINK_COPY", "hip"),), "refuse": (("SSV_LINK_REFUSE_AFTER", "2"),)}[path]
    got = _pipeline(monkeypatch, expand_first, env)
    for x, y in zip(got, pipeline_ref):
        assert x[0] == y[0] and all(np.array_equal(x[1][k], y[1][k]) for k in x[1])


def test_wire_context_closed_with_rebuild_pending():
    from seeksv_amd.device import Context
    b = craft(crafted("cigars"))
    for collect in (False, True):
        c = Context(0)
        c.clip_table_format(3)
        scan(c, [b], {})
        n, e = c.clip_cluster_async()
        assert n > 0
        if collect:
            assert c.clip_table_wait().n_clusters == n
            scan(c, [b], {}); c.clip_cluster_async()
        c.close()
