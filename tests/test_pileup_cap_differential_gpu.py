"""-m gpu: the kernels that replay the read cap of the reference's pileup (k_cap_mark / k_cap_sweep / k_cap_tail / k_cap_regrow) against the
oracle on the inputs of tests/pileup_cap_inputs.py - pinned by the REAL reference through the oracle (tests/test_pileup_cap_inputs.py,
tests/golden/pileup_cap/reference.json), all but the one that libbam refuses to index.  Counts, range sums and point depths are integers: equal, no
tolerance.  The file is scanned whole, cut around the stacks' first records and the points where the pileup fills up, cut around every
multiple of the kernels' 4096-record tile, and in batches of 1000 / 4096 / 8192 records; and through ssv_getsv_prime, the state a rank
rebuilds from the records before its own."""
import ctypes as C
import functools

import numpy as np
import pytest

import bamio
import oracle_lib as O
import pileup_cap_inputs as P
from seeksv_amd import _abi, host
from test_hip_golden import discordant_depth_and_max
from test_oracle_golden import split_batch

pytestmark = pytest.mark.gpu
QS = (20, 0)


@pytest.fixture(scope="module")
def ctx():
    from seeksv_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bam_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("pileup_cap")


_cache = {}


def loaded(bam_dir, name, q):
    """-> (case, the file as one host batch, per-record reference spans, header, plan, statistics, what the oracle computes): made once, shared"""
    if name not in _cache:
        c = P.case(name)
        path = str(bam_dir / (name + ".bam"))
        P.write_bam(path, c)
        names, lens, batches = host.read_bam(path)
        assert len(batches) == 1 and len(batches[0]["tid"]) == len(c.recs)
        span = np.array([ref_span(r["cigar"]) for r in c.recs], np.int64)
        _cache[name] = (c, batches[0], span, host.Header(names, lens))
    c, hb, span, hdr = _cache[name]
    if (name, q) not in _cache:
        stats = O.isize_stats([hb], q, 5000000)
        cols = [(c.names[t], col) for t, pos in c.stacks for col in range(max(1, pos - 150), min(c.lens[t], pos + 300) + 1)]
        plan = host.Plan(hdr, c.junctions, stats[2], stats[3], extra_points=sorted(set(cols)))   # windows over every stack, a point per column
        want = (O.discordant([hb], plan.junctions, stats[2], stats[3], 4, q),) + O.depth([hb], plan.windows, plan.ranges, plan.points, q)
        assert int(want[2].max()) > (7900 if P.KIND[name] != "control" else 3000)
        _cache[name, q] = (plan, stats, want)
    return (c, hb, span, hdr) + _cache[name, q]


@functools.lru_cache(maxsize=None)
def ref_span(cigar):
    """the span a batch states for its records (max_ref_span): M, D, N, =, X"""
    return max(1, sum(l for l, op in bamio.parse_cigar(cigar) if op in (0, 2, 3, 7, 8)))


def cut(hb, span, cuts):
    """the batch cut at the record indices `cuts`; every part says its own longest reference span, as the reader's batches do"""
    n = len(hb["tid"])
    edges = [0] + sorted(set(k for k in cuts if 0 < k < n)) + [n]
    parts = []
    for lo, hi in zip(edges, edges[1:]):
        b = split_batch(hb, lo, hi)
        b["max_ref_span"] = int(span[lo:hi].max())
        parts.append(b)
    return parts


def stack_cuts(c):
    out = []
    for tid, pos in c.stacks:
        s = c.first_index(tid, pos)
        out += [s - 1, s, s + 1, s + 7997, s + 7998, s + 7999]
    return out


def assert_equal(got, want, what, max_too=True):
    for k, label in enumerate(("counts", "range sums", "point depths")):
        assert np.array_equal(got[k], want[k]), (what, label, np.flatnonzero(got[k] != want[k])[:8])
    if max_too:
        assert len(got) == len(want) == 4 and got[3] == want[3], (what, "max_depth", got[3], want[3])


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("name", P.ALL_CASES)
def test_cap_kernels_equal_the_oracle_however_the_file_is_cut(ctx, bam_dir, name, q):
    c, hb, span, hdr, plan, stats, want = loaded(bam_dir, name, q)
    n = len(c.recs)
    runs = [("whole", [])]
    runs.append(("cut at the stacks", stack_cuts(c)))
    runs.append(("cut at the tiles", [m + d for m in range(P.TILE, n, P.TILE) for d in (-1, 1)]))
    runs += [(f"batches of {k}", list(range(k, n, k))) for k in (1000, 4096, 8192)]
    for what, cuts in runs:
        got = discordant_depth_and_max(ctx, cut(hb, span, cuts), plan, stats[2], stats[3], q, hdr.target_lens)
        assert_equal(got, want, what)


def prime(ctx, batch):
    """ssv_getsv_prime through the C ABI -> sufficient"""
    lib = _abi.hip_lib()
    lib.ssv_getsv_prime.argtypes = [C.c_void_p, C.POINTER(_abi.Batch), C.POINTER(C.c_int32)]
    lib.ssv_getsv_prime.restype = C.c_int
    b, keep = _abi.make_batch(batch)
    sufficient = C.c_int32(-1)
    rc = lib.ssv_getsv_prime(ctx._h, C.byref(b), C.byref(sufficient))
    assert rc == 0, lib.ssv_last_error(ctx._h)
    assert sufficient.value in (0, 1)
    return sufficient.value


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("name", P.ALL_CASES)
def test_primed_context_continues_the_pileup(ctx, bam_dir, name, q):
    """a context that scans [0, k) and one that is primed with [0, k) and scans [k, n) add up to the whole run: the primed one drops exactly
    the reads that the pileup, having seen [0, k), drops - before, inside and behind the (last) stack"""
    c, hb, span, hdr, plan, stats, want = loaded(bam_dir, name, q)
    n = len(c.recs)
    s = c.first_index(*c.stacks[-1])
    m = sum(1 for r in c.recs if (r["tid"], r["pos"]) == c.stacks[-1])
    for where, k in (("before", max(1, s - 300)), ("inside", s + m * 5 // 8), ("behind", s + m + 300)):
        assert 0 < k < n
        head, tail = cut(hb, span, [k])
        a = discordant_depth_and_max(ctx, [head], plan, stats[2], stats[3], q, hdr.target_lens)
        ctx.getsv_begin(plan.junctions, plan.windows, stats[2], stats[3], hdr.target_lens, 4, q, q)
        prime(ctx, head)                   # (from the file's first record: exact whatever it answers)
        ctx.getsv_scan(tail)
        b = ctx.getsv_finish(plan.ranges, plan.points)
        assert_equal(tuple(x.astype(np.int64) + y.astype(np.int64) for x, y in zip(a[:3], b[:3])), want, where, max_too=False)
        assert max(a[3], b[3]) <= want[3] <= a[3] + b[3], where     # (every column's depth is the two runs' sum: the maximum is not additive, only bounded)
    # a replayed batch that begins inside the stack and is shorter than 16,384 records cannot tell: the caller must replay a longer run
    for length in (9000, 13000):
        lo = s + 50
        part = cut(hb, span, [lo, min(n - 1, lo + length)])[1]
        assert len(part["tid"]) < 16384
        ctx.getsv_begin(plan.junctions, plan.windows, stats[2], stats[3], hdr.target_lens, 4, q, q)
        assert prime(ctx, part) == 0, length
        ctx.getsv_finish(plan.ranges, plan.points)
