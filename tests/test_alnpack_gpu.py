"""-m gpu: ssv_aln_pack (seeksv_amd/csrc/alnpack_kernels.h) through Context.aln_pack: a batch of clipped-sequence re-alignments and its read names -> the
columns the host join reads.  Held against the inputs themselves and against the plain-Python name hash of tests/clip_sam.py (which
tests/test_alnpack_model.py anchors on the host's clip_text_hash): names of every length around the 8-byte words the kernels read, starting at every
byte offset in the source and landing at every byte offset in the packed blob; host batches and the SAM decoder's device batches."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clip_sam
import readthrough_inputs as RT
import sam_text as ST
from seeksv_amd import _abi
from seeksv_amd.device import Context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seeksv_amd", "csrc")
LENGTHS = tuple(range(18)) + (31, 32, 33, 63, 64, 65, 253, 254)
N_OPS = (0, 1, 3, 300)


def scan_tile():
    """elements one workgroup of the device-wide scan covers (scan.h: BLOCK * SCAN_ITEMS)"""
    items = int(re.search(r"constexpr int SCAN_ITEMS = (\d+);", open(os.path.join(CSRC, "scan.h")).read()).group(1))
    block = int(re.search(r"constexpr int BLOCK = (\d+);", open(os.path.join(CSRC, "common.h")).read()).group(1))
    assert "SCAN_TILE = BLOCK * SCAN_ITEMS" in open(os.path.join(CSRC, "scan.h")).read()
    return items * block


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def make_case(n, seed):
    """n records (every fourth unaligned, the others with 1, 3 or 300 operations - or none) and their names: every length of LENGTHS first, then lengths drawn from them, laid out in a
    source blob with gaps of 0-7 non-zero bytes between them (so that source and packed offsets differ) behind a bias of 3 bytes"""
    rng = np.random.RandomState(seed)
    lens = [LENGTHS[(k + seed) % len(LENGTHS)] if k < len(LENGTHS) else LENGTHS[int(rng.randint(0, len(LENGTHS)))] for k in range(n)]
    names = [bytes(rng.choice(list(b"ACGTN"), l).tolist()) for l in lens]
    tid = rng.randint(0, 3, n).astype(np.int32)
    pos = rng.randint(0, 1 << 30, n).astype(np.int32)
    flag = rng.choice([0, 16, 256, 272, 2048], n).astype(np.uint16)
    mapq = rng.randint(0, 256, n).astype(np.uint8)
    n_cigar = np.array([N_OPS[int(rng.randint(0, 4))] for _ in range(n)], dtype=np.uint16)
    unaligned = np.arange(n) % 4 == 1
    tid[unaligned], pos[unaligned], flag[unaligned], mapq[unaligned], n_cigar[unaligned] = -1, -1, 4, 0, 0
    cigar_off = np.zeros(n, dtype=np.uint32)
    cigar_off[1:] = np.cumsum(n_cigar[:-1].astype(np.int64))
    total = int(n_cigar.astype(np.int64).sum())
    cigar = ((rng.randint(1, 1 << 20, total).astype(np.uint32) << 4) | rng.randint(0, 9, total).astype(np.uint32)).astype(np.uint32)
    batch = dict(tid=tid, pos=pos, flag=flag, mapq=mapq, n_cigar=n_cigar, l_qseq=np.zeros(n, np.int32), mtid=np.full(n, -1, np.int32), mpos=np.full(n, -1, np.int32),
                 isize=np.zeros(n, np.int32), cigar_off=cigar_off, cigar=cigar, xc=np.zeros(n, np.uint8), seq_off=np.full(n, _abi.NO_SEQ, np.uint64))
    bias = 3
    blob, off = bytearray(b"\x07" * bias), np.zeros(max(n, 1), dtype=np.uint64)
    for k, nm in enumerate(names):
        blob += bytes(rng.randint(1, 256, int(rng.randint(0, 8))).astype(np.uint8).tolist())
        off[k] = len(blob) - bias
        blob += nm + b"\0"
    return batch, names, bytes(blob), off, bias


def host_names(blob, off, bias):
    buf = C.create_string_buffer(blob, len(blob))
    return _abi.Names(_abi.MEM_HOST, 0, bias, C.cast(buf, C.c_void_p), off.ctypes.data, len(blob)), (buf, off)


def check(out, batch, names):
    """every column, every CIGAR word, every name byte, every hash and name_bytes"""
    n = len(names)
    assert out["n"] == n
    for k in ("tid", "pos", "flag", "mapq", "n_cigar"):
        assert out[k].dtype == batch[k].dtype and out[k].tolist() == batch[k][:n].tolist(), k
    assert len(out["cigar"]) == int(batch["n_cigar"][:n].astype(np.int64).sum())
    assert len(out["cigar_off"]) == n
    for i in range(n):
        nc, a, b = int(batch["n_cigar"][i]), int(out["cigar_off"][i]), int(batch["cigar_off"][i])
        assert out["cigar"][a:a + nc].tolist() == batch["cigar"][b:b + nc].tolist(), i
    want_blob = b"".join(x + b"\0" for x in names)
    assert out["name_bytes"] == len(want_blob)
    assert out["names_blob"] == want_blob
    want_off = np.zeros(n, dtype=np.uint64)
    if n:
        want_off[1:] = np.cumsum([len(x) + 1 for x in names[:-1]])
    assert out["name_off"].tolist() == want_off.tolist()
    assert out["names"] == list(names)
    assert out["name_hash"].tolist() == [clip_sam.text_hash(x) for x in names]


def test_case_covers_every_offset_with_every_length():
    """the inputs of the large case: every name length at every source offset modulo 8 and at every packed offset modulo 8, and every pair of the two"""
    n = 2 * scan_tile() + 1
    batch, names, blob, off, bias = make_case(n, 0)
    src = [(int(o) + bias) % 8 for o in off]
    dst = np.concatenate(([0], np.cumsum([len(x) + 1 for x in names[:-1]]))) % 8
    assert {(len(x), s) for x, s in zip(names, src)} == {(l, s) for l in LENGTHS for s in range(8)}
    assert {(len(x), int(d)) for x, d in zip(names, dst)} == {(l, d) for l in LENGTHS for d in range(8)}
    assert {(s, int(d)) for s, d in zip(src, dst)} == {(s, d) for s in range(8) for d in range(8)}
    assert {(s, len(x) % 8) for x, s in zip(names, src)} == {(s, l) for s in range(8) for l in range(8)}
    assert set(batch["n_cigar"].tolist()) == set(N_OPS)


@pytest.mark.parametrize("n", [0, 1, 65, "two_tiles_plus_1"])
def test_host_batch_host_names(ctx, n):
    n = 2 * scan_tile() + 1 if n == "two_tiles_plus_1" else n
    assert n in (0, 1, 65) or n > 2 * 256  # (the large case spans several workgroups of every kernel and three tiles of the scan)
    batch, names, blob, off, bias = make_case(n, 0)
    nm, keep = host_names(blob, off, bias)
    check(ctx.aln_pack(batch, nm), batch, names)
    if n == 65:  # ... and the names as a plain list (packed back to back in the source too)
        check(ctx.aln_pack(batch, names), batch, names)


def projected(r):
    e = ST.expected(r)
    return dict(qname=e["qname"], flag=e["flag"], tid=e["tid"], pos=e["pos"], mapq=e["mapq"], cigar=e["cigar"])


@pytest.mark.parametrize("cuts", ["every_1000_bytes", "inside_names"])
def test_through_the_decoder(ctx, cuts):
    """the SAM decoder's device batches and device names (C strings inside its copy of the text, at the line starts): cut every 1000 bytes, and cut inside read
    names - the carried line then shifts where the next chunk's names lie"""
    recs = ST.clip_positions(RT.random_records(0, n_names=300), RT.LENS)
    text = ST.text(recs, RT.NAMES, RT.LENS, with_header=False).encode("latin-1")
    if cuts == "every_1000_bytes":
        at = list(range(1000, len(text), 1000))
    else:
        starts = [0] + [m.end() for m in re.finditer(b"\n", text)][:-1]
        at = [s + 1 + k % 5 for k, s in enumerate(starts[5::11])]
        assert all(b"\t" not in text[s:a] and b"\n" not in text[s:a + 1] for s, a in zip(starts[5::11], at))
    got, batches = [], 0
    for b, nm in ctx.sam_batches(text, RT.NAMES, cuts=at):
        if not b.n:
            continue
        batches += 1
        h = ctx.batch_to_host(b)
        names = [x.encode("latin-1") for x in ST.names_to_host(ctx, nm, b.n)]
        out = ctx.aln_pack(b, nm)
        check(out, h, names)
        for i in range(out["n"]):
            a = int(out["cigar_off"][i])
            got.append(dict(qname=out["names"][i].decode("latin-1"), flag=int(out["flag"][i]), tid=int(out["tid"][i]), pos=int(out["pos"][i]), mapq=int(out["mapq"][i]),
                            cigar=[[int(c) >> 4, int(c) & 15] for c in out["cigar"][a:a + int(out["n_cigar"][i])]]))
    assert batches > 10
    assert got == [projected(r) for r in recs]


def test_two_packs_in_a_row(ctx):
    """the second result is right, and a smaller one behind a larger one carries nothing of the larger"""
    big, big_names, blob, off, bias = make_case(65, 1)
    nm, keep = host_names(blob, off, bias)
    check(ctx.aln_pack(big, nm), big, big_names)
    small, small_names, blob2, off2, bias2 = make_case(3, 2)
    nm2, keep2 = host_names(blob2, off2, bias2)
    out = ctx.aln_pack(small, nm2)
    check(out, small, small_names)
    assert out["n"] == 3 and len(out["name_hash"]) == 3 and len(out["names_blob"]) == sum(len(x) + 1 for x in small_names)
    check(ctx.aln_pack(big, nm), big, big_names)
    empty, no_names, blob0, off0, bias0 = make_case(0, 3)
    out = ctx.aln_pack(empty, [])
    assert out["n"] == 0 and out["name_bytes"] == 0 and out["names"] == [] and len(out["cigar"]) == 0 and len(out["tid"]) == 0


def test_bad_arguments_leave_the_context_usable(ctx):
    batch, names, blob, off, bias = make_case(5, 4)
    bb, keep = _abi.make_batch(batch)
    nm, keep_names = host_names(blob, off, bias)
    cols = _abi.AlnCols()
    lib, h = ctx._lib, ctx._h
    assert lib.ssv_aln_pack(h, C.byref(bb), C.byref(nm), None) == -3          # SSV_E_ARG
    assert lib.ssv_last_error(h).decode().startswith("ssv_aln_pack")
    assert lib.ssv_aln_pack(h, C.byref(bb), None, C.byref(cols)) == -3
    assert "names" in lib.ssv_last_error(h).decode()
    assert lib.ssv_aln_pack(h, None, C.byref(nm), C.byref(cols)) == -3
    null_base = _abi.Names(_abi.MEM_HOST, 0, 0, None, off.ctypes.data, len(blob))
    assert lib.ssv_aln_pack(h, C.byref(bb), C.byref(null_base), C.byref(cols)) == -3
    check(ctx.aln_pack(batch, nm), batch, names)
