"""-m gpu: the insert-size statistics (ssv_isize_*: the smallest caller of the device scan) at their edges - qualifying counts and caps around
a tile of 256, the cap on a batch edge, an empty batch, max_pairs 0, more pairs than one trip of k_isize_reduce's grid (1024 x 256), and
insert sizes whose squared deviations wrap as an int (cluster.cpp:77).  ctx.isize_stats is compared with the oracle and with a model of
cluster.cpp:48-80 in Python integers; the model is held against the oracle first.

The batches are minimal: one `100M` per record and no bases; only flag, mapq and isize vary."""
import math

import numpy as np
import pytest

import oracle_lib as O
from seeksv_amd import _abi, device

pytestmark = pytest.mark.gpu

MIN_MAPQ = 20
QUALIFIES = 99        # PAIRED | PROPER_PAIR | MREVERSE | READ1
ALL = 5000000


@pytest.fixture(scope="module")
def ctx():
    with device.Context(0) as c:
        yield c


def batch(isize, flag=None, mapq=None):
    isize = np.asarray(isize, np.int32)
    n = len(isize)
    return dict(tid=np.zeros(n, np.int32), pos=np.arange(n, dtype=np.int32), flag=np.full(n, QUALIFIES, np.uint16) if flag is None else np.asarray(flag, np.uint16),
                mapq=np.full(n, 60, np.uint8) if mapq is None else np.asarray(mapq, np.uint8), n_cigar=np.ones(n, np.uint16), l_qseq=np.zeros(n, np.int32),
                mtid=np.zeros(n, np.int32), mpos=np.arange(n, dtype=np.int32) + 200, isize=isize, cigar_off=np.arange(n, dtype=np.uint32),
                cigar=np.full(n, (100 << 4) | 0, np.uint32), xc=np.zeros(n, np.uint8), seq_off=np.full(n, _abi.NO_SEQ, np.uint64), seqqual=np.zeros(16, np.uint8),
                max_ref_span=100)


def _wrap32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x & 0x80000000 else x


def collected(batches, max_pairs, min_mapq=MIN_MAPQ):
    """cluster.cpp:48-69: the insert sizes taken, in file order.  A record below the MAPQ is skipped BEFORE the count is compared with
    read_pair_used (`continue`, :51); every other record is followed by that comparison, whether it was taken or not (:68)."""
    flag, mapq, isize = (np.concatenate([np.asarray(b[k]) for b in batches]).astype(np.int64) for k in ("flag", "mapq", "isize"))
    seen = mapq >= min_mapq
    taken = seen & (flag & 1 != 0) & (flag & 2 != 0) & (flag & 1024 == 0) & (isize > 0)
    stop = np.flatnonzero(seen & (np.cumsum(taken) == max_pairs))
    end = int(stop[0]) + 1 if len(stop) else len(isize)
    return isize[:end][taken[:end]].tolist()


def stats_of(v):
    """cluster.cpp:71-80 -> (rc, n, mean, sd, the sum of the wrapped squares)"""
    if not v:
        return 1, 0, 0, 0, 0
    mean = _wrap32((sum(v) & (2 ** 64 - 1)) // len(v))                          # :72 unsigned long / int -> int
    dev = (np.array(v, np.int64) - mean).astype(np.int32).astype(np.int64)      # :77 int - int
    d = int((dev * dev).astype(np.int32).astype(np.int64).sum())                # the product is an int too; added one by one to a double
    return 0, len(v), mean, (int(math.sqrt(d / len(v))) if d >= 0 else None), d  # :80


def check(ctx, batches, max_pairs, min_mapq=MIN_MAPQ):
    """model == oracle first, then the device against both -> the model's (rc, n, mean, sd)"""
    rc, n, mean, sd, d = stats_of(collected(batches, max_pairs, min_mapq))
    assert d >= 0, "the reference takes the square root of a negative number here: nothing is defined"
    want = O.isize_stats(batches, min_mapq, max_pairs)
    assert (rc, n, mean, sd) == want, ("model != oracle", (rc, n, mean, sd), want)
    got = ctx.isize_stats(batches, min_mapq, max_pairs)
    assert got == want, (got, want, max_pairs)
    return want


def _sizes(n, seed):
    return np.random.default_rng([0x151e, seed]).integers(100, 1000, n).astype(np.int32)


def _dense(q, seed):
    """q qualifying records in front (255: one short of the first tile, 256: the tile, 257: one into the second), then 50 that do not
    qualify, each for one reason in turn: unpaired, not a proper pair, duplicate, isize 0, isize < 0, MAPQ below the bar"""
    n = q + 50
    isize, flag, mapq = _sizes(n, seed), np.full(n, QUALIFIES, np.uint16), np.full(n, 60, np.uint8)
    r = np.arange(50) % 6
    flag[q:] = np.select([r == 0, r == 1, r == 2], [QUALIFIES & ~1, QUALIFIES & ~2, QUALIFIES | 1024], QUALIFIES)
    isize[q:] = np.select([r == 3, r == 4], [0, -300], isize[q:])
    mapq[q:] = np.where(r == 5, MIN_MAPQ - 1, 60)
    return batch(isize, flag, mapq)


def _sparse(q, seed):
    """q qualifying records, every third record between them disqualified (the same reasons in turn): tiles that are partly full"""
    n = q + q // 2 + 1
    isize, flag, mapq = _sizes(n, seed), np.full(n, QUALIFIES, np.uint16), np.full(n, 60, np.uint8)
    out = np.flatnonzero(np.arange(n) % 3 == 1)
    r = np.arange(len(out)) % 6
    flag[out] = np.select([r == 0, r == 1, r == 2], [QUALIFIES & ~1, QUALIFIES & ~2, QUALIFIES | 1024], QUALIFIES)
    isize[out] = np.select([r == 3, r == 4], [0, -300], isize[out])
    mapq[out] = np.where(r == 5, MIN_MAPQ - 1, 60)
    b = batch(isize, flag, mapq)
    extra = len(collected([b], -1)) - q
    assert extra >= 0
    if extra:   # drop qualifying records from the end until exactly q are left
        keep = np.ones(n, bool)
        keep[np.setdiff1d(np.arange(n), out)[-extra:]] = False
        b = batch(isize[keep], flag[keep], mapq[keep])
    assert len(collected([b], -1)) == q
    return b


@pytest.mark.parametrize("layout", ["dense", "sparse"])
@pytest.mark.parametrize("q", [255, 256, 257])
def test_counts_and_caps_around_a_tile(ctx, q, layout):
    b = (_dense if layout == "dense" else _sparse)(q, q)
    assert check(ctx, [b], ALL)[1] == q
    for cap in (q - 1, q, q + 1):
        assert check(ctx, [b], cap)[1] == min(cap, q)
    for cap in (254, 255, 256, 257, 258, 1):
        check(ctx, [b], cap)


def test_cap_on_a_batch_edge(ctx):
    """the cap reached on the last record of a batch (the next batch is not read), on the first record of the next, and one later"""
    a, b = _sparse(300, 1), _sparse(256, 2)
    assert collected([a], -1)[-1] == a["isize"][-1] and a["flag"][-1] == QUALIFIES and b["flag"][0] == QUALIFIES and b["mapq"][0] == 60
    for cap in (299, 300, 301, 302, 300 + 255, 300 + 256, 300 + 257):
        assert check(ctx, [a, b], cap)[1] == min(cap, 556)
    assert check(ctx, [a, b], 300) == check(ctx, [a], ALL)
    # a batch that ends with records that do not qualify, the cap reached in the middle of it
    c = _dense(256, 3)
    for cap in (256, 257, 256 + 300):
        check(ctx, [c, a], cap)


def test_an_empty_batch_between_two(ctx):
    a, b, none = _sparse(257, 4), _dense(255, 5), batch(np.zeros(0, np.int32))
    whole = check(ctx, [a, b], ALL)
    assert check(ctx, [a, none, b], ALL) == whole and whole[1] == 512
    assert check(ctx, [none, a, none, none, b, none], ALL) == whole
    assert check(ctx, [a, none, b], 258) == check(ctx, [a, b], 258)
    assert check(ctx, [none], ALL) == (1, 0, 0, 0)


def test_max_pairs_zero(ctx):
    """read_pair_used == 0 (cluster.cpp:68): the count is compared with it after every record that is not skipped, so the pass ends at
    the first such record when that one does not qualify - and never when it does (the count is 1 by then and only grows)"""
    first_out = batch([300, 310, 320], flag=[QUALIFIES & ~2, QUALIFIES, QUALIFIES])
    assert check(ctx, [first_out], 0) == (1, 0, 0, 0)
    low_then_out = batch([300, 310, 320, 330], flag=[QUALIFIES, QUALIFIES | 1024, QUALIFIES, QUALIFIES], mapq=[MIN_MAPQ - 1, 60, 60, 60])
    assert check(ctx, [low_then_out], 0) == (1, 0, 0, 0)
    assert check(ctx, [batch(np.zeros(0, np.int32))], 0) == (1, 0, 0, 0)
    first_in = _sparse(257, 6)
    assert check(ctx, [first_in], 0) == check(ctx, [first_in], ALL)
    low_then_in = batch([300, 310, 320, 330], flag=[QUALIFIES & ~1, QUALIFIES, QUALIFIES | 1024, QUALIFIES], mapq=[0, 60, 60, 60])
    assert check(ctx, [low_then_in], 0)[1] == 2
    # the first record that is not skipped lies in a later batch
    skipped = batch([300] * 5, mapq=[0] * 5)
    assert check(ctx, [skipped, first_in, _dense(255, 7)], 0)[1] == 512
    assert check(ctx, [skipped, first_out, first_in], 0) == (1, 0, 0, 0)
    # a negative value is never equal to the count: no limit
    assert check(ctx, [first_in, first_out], -1) == check(ctx, [first_in, first_out], ALL)


N_BIG = 300001     # more than k_isize_reduce's 1024 workgroups of 256 reach in one trip


def test_more_pairs_than_one_trip_of_the_reduction(ctx):
    assert N_BIG > 1024 * 256
    isize = _sizes(N_BIG, 8)
    whole = batch(isize)
    cuts = [0, 100000, 100000 + 256 * 391, N_BIG]      # three batches, the second one whole tiles
    parts = [batch(isize[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    want = check(ctx, [whole], ALL)
    assert want[1] == N_BIG
    assert check(ctx, parts, ALL) == want
    assert check(ctx, parts, 1024 * 256) == check(ctx, [whole], 1024 * 256)
    assert check(ctx, parts, 1024 * 256 + 1) == check(ctx, [whole], 1024 * 256 + 1)


def _wrapping(kind):
    """insert sizes whose deviations from the mean exceed 46,340, so the int product of cluster.cpp:77 wraps: 100 mixed with 200,000
    (`far`), or with values just below 2^31 (`huge`).  Deterministic; the first seed for which the wrapped squares add up to >= 0."""
    for seed in range(64):
        rng = np.random.default_rng([0x3a9, seed])
        n = 3001
        big = rng.integers(150000, 200001, n) if kind == "far" else 2 ** 31 - 1 - rng.integers(0, 1000, n)
        v = np.where(rng.random(n) < (0.4 if kind == "far" else 0.3), big, 100 + rng.integers(0, 50, n))
        v[0], v[-1] = big[0], 100
        if stats_of(v.tolist())[4] >= 0:
            return v.astype(np.int32)
    raise AssertionError("no seed gives a defined result")


@pytest.mark.parametrize("kind", ["far", "huge"])
def test_squares_that_wrap_as_int(ctx, kind):
    v = _wrapping(kind)
    vals = v.tolist()
    rc, n, mean, sd, d = stats_of(vals)
    sq = [_wrap32(x - mean) * _wrap32(x - mean) for x in vals]
    assert sum(_wrap32(s) for s in sq) == d
    assert max(abs(x - mean) for x in vals) > 46340 and any(_wrap32(s) < 0 for s in sq) and any(_wrap32(s) != s for s in sq)
    assert d >= 0 and sum(abs(_wrap32(s)) for s in sq) < 2 ** 53          # the one-by-one double sum is the integer sum
    if kind == "huge":
        assert sum(vals) > 2 ** 32
    assert check(ctx, [batch(v)], ALL) == (0, n, mean, sd)
    cut = [0, 1000, 1000, 2049, len(v)]
    assert check(ctx, [batch(v[a:b]) for a, b in zip(cut[:-1], cut[1:])], ALL) == (0, n, mean, sd)
