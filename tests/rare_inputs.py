"""Inputs that make a first guess of the hot path fail, in plain numpy (tests only; importable without a GPU): a quality alphabet that
is complete only behind the events the first guess looks at, batches whose candidates do not fit the initial staging of the two streaming
passes, and BAM records whose bytes look like record starts.  tests/test_rare_inputs.py checks with the oracle that each input has the
property the GPU tests (tests/test_rare_paths_gpu.py) rely on."""
import struct
import zlib

import numpy as np

NO_SEQ = np.uint64(2 ** 64 - 1)
_ACGT = np.array([1, 2, 4, 8], np.uint8)

LADDER_NAMES, LADDER_LENS = ["c0"], [200000]
CLIP_OVERFLOW_NAMES, CLIP_OVERFLOW_LENS = ["c0"], [200000]
GETSV_OVERFLOW_NAMES, GETSV_OVERFLOW_LENS = ["c0", "c1"], [40000, 40000]
GETSV_OVERFLOW_STATS = (300, 30)   # insert size mean, sd of the concordant pairs


def _seqqual(codes, quals):
    """4-bit base codes [n, lq] and quality bytes [n, lq] -> (seq_off, seqqual) of a host batch: per read the packed bases, then the qualities"""
    n, lq = codes.shape
    if lq & 1:
        codes = np.concatenate([codes, np.zeros((n, 1), np.uint8)], axis=1)
    packed = ((codes[:, 0::2] << 4) | codes[:, 1::2]).astype(np.uint8)
    entry = np.concatenate([packed, quals.astype(np.uint8)], axis=1)
    return (np.arange(n) * entry.shape[1]).astype(np.uint64), np.concatenate([entry.reshape(-1), np.zeros(16, np.uint8)])


def _batch(tid, pos, n_cigar, cigar, lq, seq_off, seqqual, max_ref_span, flag=None, mapq=None, mtid=None, mpos=None, isize=None):
    n = len(pos)
    nc = np.asarray(n_cigar, np.int64)
    return dict(tid=np.asarray(tid, np.int32), pos=np.asarray(pos, np.int32), flag=np.full(n, 99, np.uint16) if flag is None else np.asarray(flag, np.uint16),
                mapq=np.full(n, 60, np.uint8) if mapq is None else np.asarray(mapq, np.uint8), n_cigar=nc.astype(np.uint16), l_qseq=np.full(n, lq, np.int32),
                mtid=np.asarray(tid, np.int32) if mtid is None else np.asarray(mtid, np.int32), mpos=(np.asarray(pos) + 200).astype(np.int32) if mpos is None else np.asarray(mpos, np.int32),
                isize=np.full(n, 250, np.int32) if isize is None else np.asarray(isize, np.int32), xc=np.zeros(n, np.uint8), cigar=np.asarray(cigar, np.uint32),
                cigar_off=(np.cumsum(nc) - nc).astype(np.uint32), seq_off=seq_off, seqqual=seqqual, max_ref_span=int(max_ref_span))


def ladder_batch(first, late, n=6000, late_from=5000, lq=50, n_every=0, big_bin=0, long_skip=False):
    """One contig, read i at pos 1000 + 2 i, `20S30M` and `30M20S` alternating in runs of three (both event lists fill, one event per read: event order is
    read order).  Every 17th triple and the last 30 reads are stacks of three identical reads on one start (multi-event bins: the consensus path).  Bases cycle
    through A/C/G/T.  The qualities (phred values) of the reads before `late_from` come from `first` alone - none at all (0xff) where `first` is empty -, from
    `late_from` on from first + late: a guess of the alphabet from fewer than `late_from` events misses every value of `late`.
    n_every = k: every k-th base is N; big_bin: that many identical reads more on one further start; long_skip: `10M4096N20M20S` on some reads."""
    first, union = sorted(first), sorted(set(first) | set(late))
    assert (n - 30) % 3 == 0 and late_from < n - 30 and not set(first) & set(late)
    i = np.arange(n + big_bin)
    t = i // 3
    stack = ((t % 17 == 0) | (i >= n - 30)) & (i < n)
    src = np.where(stack, 3 * t, np.minimum(i, n))           # the read whose bases and qualities read i carries
    pos = 1000 + 2 * src + np.where(i >= n, 1000, 0)
    left = (t % 2 == 0) | (i >= n)
    skip = (~left & ~stack & (i % 97 == 5)) if long_skip else np.zeros(len(i), bool)
    j = np.arange(lq)
    codes = _ACGT[(src[:, None] + j) % 4]
    if n_every:
        codes = np.where((src[:, None] * lq + j) % n_every == 0, np.uint8(15), codes).astype(np.uint8)
    k = src[:, None] * 7 + j
    quals = np.asarray(union, np.uint8)[k % len(union)]
    early = src < late_from
    quals[early] = np.asarray(first, np.uint8)[k[early] % len(first)] if first else 0xff
    S, M, N = 4, 0, 3
    cig = np.zeros((len(i), 4), np.uint32)
    cig[left, :2] = [(20 << 4) | S, (30 << 4) | M]
    cig[~left, :2] = [(30 << 4) | M, (20 << 4) | S]
    cig[skip] = [(10 << 4) | M, (4096 << 4) | N, (20 << 4) | M, (20 << 4) | S]
    nc = np.where(skip, 4, 2)
    seq_off, seqqual = _seqqual(codes, quals)
    return _batch(np.zeros(len(i), np.int32), pos, nc, cig[np.arange(4) < nc[:, None]], lq, seq_off, seqqual, 4126 if long_skip else 30)


def ladder_values(k, start=3, step=5):
    """k distinct phred values below 64, in no particular order"""
    v = [(start + step * x) % 61 for x in range(k)]
    assert len(set(v)) == k
    return v


def clip_overflow_batch():
    """12 x 8192 records (twelve tiles of the clip scan, one per workgroup) at pos 100 + i, 30 bases: tiles 0-5 with every tenth read clipped (`10S20M`), tiles
    6-11 all clipped - 8192 candidates where a workgroup's share of the initial staging (max(65536, n / 8) entries over 12 workgroups) holds 5462"""
    n, lq = 12 * 8192, 30
    i = np.arange(n)
    clipped = (i >= 6 * 8192) | (i % 10 == 0)
    j = np.arange(lq)
    seq_off, seqqual = _seqqual(_ACGT[(i[:, None] + j) % 4], np.array([2, 12, 23, 37], np.uint8)[(i[:, None] * 3 + j) % 4])
    cig = np.zeros((n, 2), np.uint32)
    cig[clipped] = [(10 << 4) | 4, (20 << 4) | 0]
    cig[~clipped, 0] = (30 << 4) | 0
    nc = np.where(clipped, 2, 1)
    return _batch(np.zeros(n, np.int32), 100 + i, nc, cig[np.arange(2) < nc[:, None]], lq, seq_off, seqqual, 30)


GETSV_OVERFLOW_JUNCTIONS = [("c0", p, "+", "c0", p + 3000, "+") for p in range(5200, 13400, 400)]


def getsv_overflow_batch(tail_contig=False):
    """20 x 4096 records (twenty tiles of the getsv scan) of `50M`, ten to a start from 5000 on, on a 40 kb contig: every third one half of a pair 3300 apart
    (discordant at mean 300, sd 30), the others concordant.  With GETSV_OVERFLOW_JUNCTIONS every record starts in a tile that a depth window marks: every
    tile holds 4096 candidates where a workgroup's share of the initial staging holds 3277.  tail_contig: 100 records of the second contig behind them (two
    runs of the tid column)."""
    n = 20 * 4096
    i = np.arange(n)
    pos = 5000 + i // 10
    far, fwd = i % 3 == 0, i % 2 == 0
    flag = np.where(far, 97, np.where(fwd, 99, 147))
    mpos = np.where(far, pos + 3250, np.where(fwd, pos + 250, pos - 250))
    isize = np.where(far, 3300, np.where(fwd, 300, -300))
    tid = np.zeros(n, np.int32)
    if tail_contig:
        m = 100
        tid, pos, flag = np.concatenate([tid, np.ones(m, np.int32)]), np.concatenate([pos, 100 + np.arange(m)]), np.concatenate([flag, np.full(m, 99)])
        mpos, isize = np.concatenate([mpos, 350 + np.arange(m)]), np.concatenate([isize, np.full(m, 300)])
    n = len(pos)
    return _batch(tid, pos, np.ones(n, np.int64), np.full(n, (50 << 4) | 0, np.uint32), 50, np.full(n, NO_SEQ, np.uint64), np.zeros(16, np.uint8), 50,
                  flag=flag, mtid=tid, mpos=mpos, isize=isize)


def getsv_overflow_plan():
    """-> (header, plan) of getsv_overflow_batch: close both"""
    from seeksv_amd import host
    hdr = host.Header(GETSV_OVERFLOW_NAMES, GETSV_OVERFLOW_LENS)
    return hdr, host.Plan(hdr, GETSV_OVERFLOW_JUNCTIONS, *GETSV_OVERFLOW_STATS)


# ---- records whose bytes look like record starts ----

DECOY_FAKE = struct.pack("<iiiBBHHHiiii", 36, 0, 5, 2, 0, 0, 0, 0, 0, -1, -1, 0) + b"x\0" + b"\0\0"   # block_size 36: a 40-byte "record" on contig 0 at pos 5, named "x"
DECOY_AT = (100, 250, 400, 550)
DECOY_FAKES = (1500, 5000, 1500, 5000)


def decoy_records():
    """test_bam_reader._records(600, 21) plus four records with one short read whose aux field XD:B:C is an array of back-to-back DECOY_FAKEs, every one of
    which passes the device decoder's header test: a BGZF block that lies inside such an array finds three chained plausible headers at once.  The first
    two records end with the array (the chain of fakes leads exactly to the next true record); the other two carry four zero bytes at the array's end and an
    NM:C tag behind it (the chain of fakes ends in a block_size below 32)."""
    from test_bam_reader import _records
    assert len(DECOY_FAKE) == 40
    recs = _records(600, 21)
    for k, (at, fakes) in enumerate(zip(DECOY_AT, DECOY_FAKES)):
        body = DECOY_FAKE * fakes + (b"\0\0\0\0" if k >= 2 else b"")
        aux = b"XDBC" + struct.pack("<i", len(body)) + body + (b"NMC\x01" if k >= 2 else b"")
        recs.insert(at + k, dict(qname=f"decoy{k}", flag=99, tid=0, pos=700 + k, mapq=60, cigar="4S8M", mtid=0, mpos=900, isize=212, seq="ACGTACGTACGT", qual=bytes(range(20, 32)), aux=aux))
    return recs


def bgzf_blocks(path):
    """the inflated bytes of a BGZF file and the offset at which each block's bytes begin in them"""
    raw = open(path, "rb").read()
    out, starts, o = bytearray(), [], 0
    while o < len(raw):
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        starts.append(len(out))
        out += zlib.decompress(raw[o + 18:o + bsize - 8], -15)
        o += bsize
    return bytes(out), starts


def true_record_starts(stream):
    """offsets of the records of a BAM's inflated bytes"""
    l_text, = struct.unpack_from("<i", stream, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", stream, p)
    p += 4
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", stream, p)
        p += 8 + l
    starts = []
    while p < len(stream):
        starts.append(p)
        p += 4 + struct.unpack_from("<i", stream, p)[0]
    assert p == len(stream)
    return starts


def plausible_record(u, o, n_targets, tlen):
    """the device decoder's header test (bamdec_kernels.h, plausible_record) restated: could a BAM record start at u[o]?"""
    total = len(u)
    bs, = struct.unpack_from("<I", u, o)
    if bs < 32 or bs > (1 << 28):
        return False
    refid, pos, l_name, _mapq, _bin, ncig, _flag, l_seq, next_ref, next_pos = struct.unpack_from("<iiBBHHHiii", u, o + 4)
    if refid < -1 or refid >= n_targets or next_ref < -1 or next_ref >= n_targets or pos < -1 or next_pos < -1 or l_seq < 0 or l_name < 2:
        return False
    if tlen is not None and refid >= 0 and pos >= tlen[refid]:
        return False
    if 32 + l_name + 4 * ncig + (l_seq + 1) // 2 + l_seq > bs:
        return False
    nul = o + 4 + 32 + l_name - 1
    return nul >= total or u[nul] == 0


def first_guess(u, begin, end, n_targets, tlen, run=3):
    """k_find_records' guess for the block [begin, end) restated: the first offset from which `run` plausible headers chain (or the stream ends); None: no guess.
    THIS RESTATES THE RULE AS IT STANDS TODAY and proves only that a fixture still fools it: the device decoder is never held against it, only against the host reader."""
    total = len(u)
    o = begin
    while o < end and o + 36 <= total:
        q, k = o, 0
        while k < run and q + 36 <= total:
            if not plausible_record(u, q, n_targets, tlen):
                break
            q += 4 + struct.unpack_from("<I", u, q)[0]
            k += 1
        if k == run or (k > 0 and q + 36 > total):
            return o
        o += 1
    return None


# ---- the late-alphabet cases: (id, first, late, (qual_bits, qual_group) of the final alphabet with grouping on) ----

_V = ladder_values(46)
_SHAPE = {2: (1, 1), 5: (7, 3), 6: (3, 1), 9: (7, 2), 12: (4, 1), 17: (11, 2), 46: (8, 1)}   # by alphabet size: the rows of test_compact_table_quality_alphabets
TRANSITIONS = [(f"{k}to{k + 1}", _V[:k], [_V[k]], _SHAPE[k + 1]) for k in (4, 5, 8, 11, 16, 45)] + [
    ("noneto5", [], _V[:5], _SHAPE[5]),
    ("1to2", _V[:1], [_V[1]], _SHAPE[2]),
    ("5to6_late70", _V[:5], [70], _SHAPE[6]),          # the direct kernel first (all below phred 64), the final pack must take the staged one
    ("5with70to6", _V[:4] + [70], [_V[4]], _SHAPE[6]),   # the staged kernel first
]
TRANSITION = {t[0]: t for t in TRANSITIONS}
TRANSITION["9to12"] = ("9to12", _V[:9], _V[9:12], _SHAPE[12])          # (run with SSV_QUAL_GROUPS=0: one field per quality before and after)
TRANSITION["five-values"] = ("five-values", _V[:5], [], _SHAPE[5])     # nothing late: the rungs of the pack ladder without that one
