"""-m gpu: one batch in every form ssv_batch_t allows (include/seeksv_hip.h) gives one cluster table, and a device batch comes back from
ssv_batch_to_host column by column.  The batch is the one of tests/golden/getclip/filters.bam (32 records): cut to 0 and 1 records, whole, and - so that
one size has more than one 256-thread block, of which the last holds a single record - 257 records of the batch with every record nine times in a row."""
import ctypes as C
import os

import numpy as np
import pytest

import golden_util as G
from seeksv_amd import _abi, host

pytestmark = pytest.mark.gpu
FIXED = ("tid", "pos", "flag", "mapq", "n_cigar", "l_qseq", "mtid", "mpos", "isize", "cigar_off", "xc", "seq_off", "cigar_ends")
TABLE = ("tid", "pos", "side", "support", "left_len", "right_len", "str", "cigar", "n_cigar")


@pytest.fixture(scope="module")
def ctx():
    from seeksv_amd.device import Context
    with Context(0) as c:
        yield c


def ninefold(b):
    """every record nine times in a row (still coordinate sorted), each copy with CIGAR operations and bases of its own"""
    n, r = len(b["tid"]), 9
    out = {k: np.repeat(b[k], r) for k in FIXED}
    cig, seq = [], []
    for i in range(n):
        ops = b["cigar"][int(b["cigar_off"][i]):int(b["cigar_off"][i]) + int(b["n_cigar"][i])]
        shipped = int(b["seq_off"][i]) != _abi.NO_SEQ
        l = int(b["l_qseq"][i])
        bases = b["seqqual"][int(b["seq_off"][i]):int(b["seq_off"][i]) + (l + 1) // 2 + l] if shipped else b["seqqual"][:0]
        for k in range(r):
            out["cigar_off"][i * r + k] = sum(len(x) for x in cig)
            out["seq_off"][i * r + k] = sum(len(x) for x in seq) if shipped else _abi.NO_SEQ
            cig.append(ops)
            seq.append(bases)
    out["cigar"], out["seqqual"], out["max_ref_span"] = np.concatenate(cig), np.concatenate(seq), b["max_ref_span"]
    return out


def cut(b, n):
    """the first n records (the variable parts whole: the offsets are absolute)"""
    return {k: (v[:n] if k in FIXED else v) for k, v in b.items()}


@pytest.fixture(scope="module")
def cases():
    _, _, batches = host.read_bam(os.path.join(G.GOLDEN, "getclip", "filters.bam"))
    assert len(batches) == 1 and len(batches[0]["tid"]) == 32 and batches[0]["xc"].any() and "cigar_ends" in batches[0]
    whole = batches[0]
    return {0: cut(whole, 0), 1: cut(whole, 1), 257: cut(ninefold(whole), 257), "whole": whole}


def to_device(b, drop=()):
    """the columns copied to the GPU with torch -> (_abi.Batch with MEM_DEVICE and no rec, keepalive); 16 spare bytes behind every column, so that no
    pointer is null even for n = 0 and whole words may be read off the end of seqqual"""
    import torch
    dev, ptr = {}, {}
    for k, v in b.items():
        if isinstance(v, np.ndarray) and k not in drop:
            raw = np.concatenate((np.ascontiguousarray(v).view(np.uint8), np.zeros(16, np.uint8)))
            dev[k] = torch.from_numpy(raw).cuda()
            ptr[k] = dev[k].data_ptr()
    torch.cuda.synchronize()
    ptr.update(n_cigar_total=len(b["cigar"]), seqqual_bytes=len(b["seqqual"]), max_ref_span=b["max_ref_span"])
    for k in drop:
        ptr[k] = None
    batch, _ = _abi.make_batch(ptr, mem=_abi.MEM_DEVICE, n=len(b["tid"]))
    return batch, dev


def same_table(got, want, what):
    assert got["n_clusters"] == want["n_clusters"] and got["n_events"] == want["n_events"], what
    for k in TABLE:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("n", [0, 1, 257, "whole"])
def test_every_form_gives_the_same_table(ctx, cases, n):
    b = cases[n]
    runs = [host.host_tid_runs(b, 0)]
    table = lambda x: ctx.getclip([x], tid_runs=runs)
    want = table(b)
    if n in (257, "whole"):
        assert want["n_clusters"] > 0
    announced, keep = _abi.make_batch(b)
    ctx.prefetch(announced)
    same_table(table(announced), want, "host, announced with prefetch")
    if n == 0:
        # a scan call returns at once for an empty batch and stages nothing, so the announcement is still there (drivers announce no empty
        # batch); for every other size the scan took it, or the next host batch below would be refused
        ctx.prefetch_drop()
    same_table(table({k: v for k, v in b.items() if k != "cigar_ends"}), want, "host, no cigar_ends")
    # xc = NULL says "all 0": the table of the batch with a column of zeros
    cleared = dict(b, xc=np.zeros_like(b["xc"]))
    same_table(table(dict(b, xc=None)), table(cleared), "host, xc = None")
    dev, keep_dev = to_device(b)
    assert dev.mem == _abi.MEM_DEVICE and not dev.rec and (dev.xc and dev.cigar_ends)
    same_table(table(dev), want, "device columns")
    kept = ctx.batch_retain(dev)
    try:
        same_table(table(kept), want, "device columns, retained")
    finally:
        ctx.batch_release(kept)


@pytest.mark.parametrize("drop", [(), ("xc", "cigar_ends")])
@pytest.mark.parametrize("n", [0, 1, 257, "whole"])
def test_batch_to_host_returns_every_column(ctx, cases, n, drop):
    b = cases[n]
    dev, keep_dev = to_device(b, drop)
    h = _abi.Batch()
    assert ctx._lib.ssv_batch_to_host(ctx._h, C.byref(dev), C.byref(h)) == 0
    assert h.mem == _abi.MEM_HOST and h.n == len(b["tid"]) and not h.rec
    assert h.n_cigar_total == len(b["cigar"]) and h.seqqual_bytes == len(b["seqqual"]) and h.max_ref_span == b["max_ref_span"]
    for k in ("xc", "cigar_ends"):
        assert (getattr(h, k) is None) == (k in drop), k
    got = _abi.batch_to_arrays(h)
    for k in FIXED + ("cigar", "seqqual"):
        if k not in drop:
            assert got[k].dtype == b[k].dtype and np.array_equal(got[k], b[k]), k
