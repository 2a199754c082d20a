"""-m gpu: ssv_realign_split_batch (k_rr_sizes, k_rr_rows) - the split query's reads, hits and mates as a device batch - against
tests/realign_split_model.bam_records record for record, on the hash index and on the sorted one, and the batch through the -F pass against the same rows
handed over as a host batch and against tests/readthrough_model.find_junction.  Inputs: tests/run_split_inputs.py, held to their properties on the CPU in
tests/test_run_split_inputs.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import readthrough_model as RM
import realign_model as M
import realign_split_inputs as SI
import run_split_inputs as RI
import sam_text as ST
from seeksv_amd import _abi

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -3, -4
INDEXES = pytest.mark.parametrize("max_occ", [None, SI.CAP], ids=["hash", "sorted"])


@pytest.fixture(scope="module")
def ctx():
    from seeksv_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rt():
    """the -F pass's context: another one on the same GPU, as in `seeksv run`"""
    from seeksv_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def index(ctx, max_occ):
    words, off = M.pack_2bit(SI.reference())
    return ctx.realign_index(words, off) if max_occ is None else ctx.realign_index_sorted(words, off, max_occ)


@functools.lru_cache(maxsize=None)
def want_rows(name, max_occ):
    """the model's rows of a set, computed once per index and shared"""
    s = RI.SETS[name]()
    return tuple(RI.model_rows(s, RI.model_results(s, max_occ)))


def split_batch(ctx, entries, quals=True):
    return ctx.realign_split_batch([e[1] for e in entries], [e[0] for e in entries], [e[2] for e in entries] if quals else None)


def to_host(ctx, b, nm):
    """-> (the classic columns, the join's columns with the names, the record lines)"""
    host = ctx.batch_to_host(b)
    packed = ctx.aln_pack(b, nm)
    lines = np.frombuffer(ST.device_to_host(ctx, b.rec, b.n * 64), dtype=_abi.RECORD_DTYPE) if b.n else np.zeros(0, _abi.RECORD_DTYPE)
    return host, packed, lines


def check_rows(b, host, packed, lines, rows, quals=True):
    n = len(rows)
    assert b.n == n == packed["n"] == len(lines) and b.mem == _abi.MEM_DEVICE and b.max_ref_span == 1024 and b.n_tid_runs == 0 and not b.tid_runs
    assert b.n_cigar_total == sum(len(r["cigar"]) for r in rows) == len(host["cigar"]) and b.seqqual_bytes == len(host["seqqual"])
    sq = host["seqqual"]
    used = 0
    for i, r in enumerate(rows):
        L, ops = len(r["seq"]), [(l << 4) | op for l, op in r["cigar"]]
        what = (i, r["qname"][:30], L)
        assert packed["names"][i].decode() == r["qname"], what
        for cols in (host, packed):
            assert (int(cols["flag"][i]), int(cols["tid"][i]), int(cols["pos"][i]), int(cols["mapq"][i])) == (r["flag"], r["tid"], r["pos"], r["mapq"]), what
            co = int(cols["cigar_off"][i])
            assert int(cols["n_cigar"][i]) == len(ops) and [int(x) for x in cols["cigar"][co:co + len(ops)]] == ops, what
        assert (int(host["l_qseq"][i]), int(host["mtid"][i]), int(host["mpos"][i]), int(host["isize"][i]), int(host["xc"][i])) == (L, -1, -1, 0, 0), what
        so, nb = int(host["seq_off"][i]), (L + 1) // 2
        assert so % 4 == 0 and so >= used and so + nb + L <= len(sq), what       # whole dwords, no record inside another, inside the blob
        used = so + nb + L
        assert RM.record_bases(host, i) == r["seq"], what
        if L % 2:
            assert int(sq[so + nb - 1]) & 15 == 0, what
        q = sq[so + nb:so + nb + L]
        assert (q == 0xff).all() if not quals else [int(x) for x in q] == [ord(ch) - 33 for ch in r["qual"]], what
        assert int(host["cigar_ends"][i]) == (0xff if not ops else (ops[0] & 15) | (ops[-1] & 15) << 4), what
        ln = lines[i]
        for k in ("tid", "pos", "flag", "mapq", "xc", "n_cigar", "l_qseq", "mtid", "mpos", "isize", "cigar_off", "seq_off"):
            assert int(ln[k]) == int(host[k][i]), (what, k)
        assert [int(x) for x in ln["cigar_head"]] == (ops + [0] * 5)[:5], what


@INDEXES
@pytest.mark.parametrize("name", list(RI.SETS))
def test_every_record_of_every_set(ctx, name, max_occ):
    """hits and mates are ssv_realign_query_split's byte for byte; every field of every record is the model's; the columns, cigar_ends and the record
    lines agree"""
    s = RI.SETS[name]()
    index(ctx, max_occ)
    h0, m0 = ctx.realign_split([e[1] for e in s])
    hits, mates, b, nm = split_batch(ctx, s)
    assert hits.tobytes() == h0.tobytes() and mates.tobytes() == m0.tobytes()
    rows = want_rows(name, max_occ)
    assert len(rows) == len(s) + int((mates["tid"] >= 0).sum())
    if name == "empty":
        assert b.n == 0 and b.mem == _abi.MEM_DEVICE
        return
    check_rows(b, *to_host(ctx, b, nm), rows)


@INDEXES
def test_without_qualities_only_the_qualities_differ(ctx, max_occ):
    s = RI.length_set() + tuple(("A_" + e[0][:200], e[1], e[2]) for e in RI.alphabet_set())
    index(ctx, max_occ)
    _, _, b, nm = split_batch(ctx, s)
    with_q = to_host(ctx, b, nm)
    hits, mates, b, nm = split_batch(ctx, s, quals=False)
    host, packed, lines = to_host(ctx, b, nm)
    rows = RI.model_rows(s, RI.model_results(s, max_occ))
    check_rows(b, host, packed, lines, rows, quals=False)
    is_q = np.zeros(len(host["seqqual"]), bool)
    for i, r in enumerate(rows):
        so, L = int(host["seq_off"][i]), len(r["seq"])
        is_q[so + (L + 1) // 2:so + (L + 1) // 2 + L] = True
    for k in host:
        if k == "seqqual":
            assert (host[k][is_q] == 0xff).all() and np.array_equal(host[k][~is_q], with_q[0][k][~is_q])
        else:
            assert np.array_equal(host[k], with_q[0][k]), k
    assert lines.tobytes() == with_q[2].tobytes() and packed["names"] == with_q[1]["names"]


def rt_raw(r):
    """an _abi.RtResult copied out: (n_pairs, n_candidates, the pairs, their seqs, their CIGAR sources) as bytes"""
    n = int(r.n_pairs)
    ps = [r.pairs[k] for k in range(n)]
    seq_end = max([p.seq_off + p.up_len + p.down_len for p in ps] + [0])
    cig_end = max([p.cig_off + p.up_cig_n + p.down_cig_n for p in ps] + [0])
    return (n, int(r.n_candidates), C.string_at(r.pairs, n * C.sizeof(_abi.RtPair)) if n else b"", C.string_at(r.seqs, seq_end) if seq_end else b"",
            C.string_at(r.cigars, 4 * cig_end) if cig_end else b"")


def through_F(ctx, rt, pieces, min_mapq=1):
    """every piece of reads through ssv_realign_split_batch, its device batch through the -F pass of the other context in place"""
    rt.rt_begin(min_mapq, SI.NAMES)
    for s in pieces:
        _, _, b, nm = split_batch(ctx, s)
        rt.rt_scan(b, nm)
        rt.sync()
    r = rt.rt_finish()
    return rt_raw(r), (rt.rt_decode(r, SI.NAMES), int(r.n_candidates))


def rows_through_F(rt, rows, min_mapq=1):
    batch, names = RM.batch_from_records(rows)
    rt.rt_begin(min_mapq, SI.NAMES)
    rt.rt_scan(batch, names)
    r = rt.rt_finish()
    return rt_raw(r), (rt.rt_decode(r, SI.NAMES), int(r.n_candidates))


F_SETS = ("all_mate", "alphabet", "length", "strand")


@INDEXES
def test_the_batch_through_the_F_pass(ctx, rt, max_occ):
    """the device batch scanned in place gives the ssv_rt_result of the model's rows handed over as a host batch - pairs, seqs and CIGAR sources byte for
    byte - and find_junction's pairs; in one call and in two pieces cut between two reads"""
    index(ctx, max_occ)
    for name in F_SETS:
        s = RI.SETS[name]()
        rows = list(want_rows(name, max_occ))
        want_raw, want = rows_through_F(rt, rows)
        model = RI.model_junctions(rows, SI.NAMES)
        assert want == (model[0], model[1]) and (len(model[0]) > 0 or name == "length")
        cut = len(s) // 2 + 1
        for pieces in ((s,), (s[:cut], s[cut:])):
            got_raw, got = through_F(ctx, rt, pieces)
            assert got == want, (name, len(pieces))
            assert got_raw == want_raw, (name, len(pieces))
    assert sum(len(RI.model_junctions(list(want_rows(n, max_occ)), SI.NAMES)[0]) for n in F_SETS) > 30


def test_the_batch_through_the_F_pass_with_colliding_name_hashes(ctx, rt, monkeypatch):
    """SSV_RT_HASH_BITS=4: the names of a read's two records are one offset of the name blob; pairing compares them in full"""
    monkeypatch.setenv("SSV_RT_HASH_BITS", "4")
    index(ctx, None)
    s = RI.all_mate_set() + tuple(("x" + e[0][:250], e[1], e[2]) for e in RI.strand_set())
    rows = RI.model_rows(s, RI.model_results(s))
    want_raw, want = rows_through_F(rt, rows)
    model = RI.model_junctions(rows, SI.NAMES)
    assert want == (model[0], model[1]) and len(model[0]) > 20
    got_raw, got = through_F(ctx, rt, (s[:5], s[5:]))
    assert got == want and got_raw == want_raw
    for w in (0, 61):   # the pass's MAPQ floor
        assert through_F(ctx, rt, (s,), min_mapq=w)[1] == tuple(RI.model_junctions(rows, SI.NAMES, w))


def test_error_codes_come_first():
    """(a context of its own) the split query's errors, NULL names / out, names of 0 and 255 bytes, before the index, n = 0"""
    from seeksv_amd.device import Context
    words, off = M.pack_2bit(SI.reference())
    with Context(0) as c:
        fn = c._lib.ssv_realign_split_batch
        hits, mates = np.zeros(2, dtype=np.dtype(_abi.REALIGN_HIT)), np.zeros(2, dtype=np.dtype(_abi.REALIGN_HIT))
        mates["score"] = -7
        read = SI.read("ff")
        seq, qoff = C.c_char_p((read + "ACGT").encode()), np.array([0, len(read), len(read) + 4], np.uint64)
        names, noff = C.c_char_p(b"r1\0q\0"), np.array([0, 3, 5], np.uint64)
        b, nm = _abi.Batch(), _abi.Names()
        H, Mt, Q, NO, B, NM = hits.ctypes.data, mates.ctypes.data, qoff.ctypes.data, noff.ctypes.data, C.byref(b), C.byref(nm)
        assert fn(c._h, seq, Q, 2, None, names, NO, H, Mt, B, NM) == E_STATE                    # before the index
        assert fn(None, seq, Q, 2, None, names, NO, H, Mt, B, NM) == E_ARG
        assert c._lib.ssv_realign_index(c._h, words.ctypes.data, 0, int(off[-1]), off.ctypes.data, len(off) - 1, None) == 0
        assert fn(c._h, seq, Q, 2, None, None, NO, H, Mt, B, NM) == E_ARG                       # NULL names
        assert fn(c._h, seq, Q, 2, None, names, None, H, Mt, B, NM) == E_ARG
        assert fn(c._h, seq, Q, 2, None, names, NO, H, Mt, None, NM) == E_ARG                   # NULL out
        assert fn(c._h, seq, Q, 2, None, names, NO, H, Mt, B, None) == E_ARG
        assert fn(c._h, seq, Q, 2, None, names, NO, H, None, B, NM) == E_ARG
        assert fn(c._h, seq, Q, 2, None, names, NO, None, Mt, B, NM) == E_ARG
        assert fn(c._h, None, Q, 2, None, names, NO, H, Mt, B, NM) == E_ARG
        assert fn(c._h, seq, Q, -1, None, names, NO, H, Mt, B, NM) == E_ARG
        empty = np.array([0, 1, 3], np.uint64)                                                  # an empty name
        assert fn(c._h, seq, Q, 2, None, C.c_char_p(b"\0q\0"), empty.ctypes.data, H, Mt, B, NM) == E_ARG
        assert b"name" in c._lib.ssv_last_error(c._h)
        long_off = np.array([0, 3, 3 + 256], np.uint64)                                         # 255 bytes and the NUL
        assert fn(c._h, seq, Q, 2, None, C.c_char_p(b"r1\0" + b"n" * 255 + b"\0"), long_off.ctypes.data, H, Mt, B, NM) == E_ARG
        assert int(mates["score"][0]) == -7                                                     # nothing was written by a refused call
        ok_off = np.array([0, 3, 3 + 255], np.uint64)                                           # 254 bytes are a name
        assert fn(c._h, seq, Q, 2, None, C.c_char_p(b"r1\0" + b"n" * 254 + b"\0"), ok_off.ctypes.data, H, Mt, B, NM) == 0
        assert b.n == 3 and int(hits["tid"][0]) >= 0 and int(mates["tid"][0]) >= 0 and int(hits["tid"][1]) == -1 and int(mates["tid"][1]) == -1
        assert fn(c._h, seq, Q, 0, None, names, NO, H, Mt, B, NM) == 0 and b.n == 0 and b.mem == _abi.MEM_DEVICE   # n = 0
        assert c._lib.ssv_realign_free(c._h) == 0
        assert fn(c._h, seq, Q, 2, None, names, NO, H, Mt, B, NM) == E_STATE
