"""-m gpu: the device SAM-text decoder in its mode for coordinate-sorted originals (ssv_samdec_sorted / ssv_samdec_lists, seeksv_amd/csrc/samdec_kernels.h)
against ssv_bamdec_decode(keep_all_seq = 0) on the BAM of the same records (tests/bamio.py): every column, seqqual byte for byte, tid_runs, the info lists,
and unmapped_raw with `bin` masked and the optional fields stripped on the BAM side.  Every comparison is exact."""
import os
import struct
import tempfile

import numpy as np
import pytest

import bamio
import original_sam
import original_sam_inputs as I
import readthrough_inputs as RT
import sam_text as ST
from seeksv_amd import _abi, host
from seeksv_amd.device import Context, SeeksvError

pytestmark = pytest.mark.gpu

NAMES, LENS = RT.NAMES, RT.LENS
EXAMPLE = os.path.join(RT.GOLDEN, "example")
NO_SEQ = np.uint64(2 ** 64 - 1)
COLS = [k for k, _ in _abi.BATCH_FIELDS]
FIXED = ("tid", "pos", "flag", "mapq", "n_cigar", "l_qseq", "mtid", "mpos", "isize", "xc", "cigar_ends")


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


# ---- the two decoders -----------------------------------------------------------------------------------------------------------------------------------------

def strip_raw(raw):
    """the side channel of the BAM decoder as the text decoder gives it: bin 0, no optional fields"""
    out, p = bytearray(), 0
    while p < len(raw):
        bs, = struct.unpack_from("<i", raw, p)
        l_name, n_cig, l_seq = raw[p + 12], struct.unpack_from("<H", raw, p + 16)[0], struct.unpack_from("<i", raw, p + 20)[0]
        keep = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        rec = bytearray(raw[p + 4:p + 4 + keep])
        rec[10:12] = b"\0\0"
        out += struct.pack("<i", keep) + rec
        p += 4 + bs
    return bytes(out)


def bam_side(r):
    """a record as the BAM of the same file has it: XC as aux bytes, UNMAP set where the CIGAR is '*' (libbam's text reader sets it)"""
    r = dict(r)
    if r.get("cigar", "") in ("", "*", []):
        r["flag"] = r.get("flag", 0) | 4
    if isinstance(r.get("qual"), str):
        r["qual"] = bytes((ord(ch) - 33) & 0xff for ch in r["qual"])
    r["aux"] = ST.bam_aux(r)
    return r


def collect(ctx, b, info, out):
    out["batches"].append(ctx.batch_to_host(b) if b.n else None)
    runs = b.get_tid_runs()
    out["tid_runs"].append([] if runs is None else [(int(f), int(t)) for f, t in zip(runs["first"], runs["tid"])])
    out["seq_ptr"].append(bool(b.seqqual) if b.n else True)
    out["changes"] += [(out["n"] + i, t) for i, t in info["tid_runs"]]
    out["raw"] += info["unmapped_raw"]
    out["unmapped"] += info["unmapped"]
    out["last_tid"] = info["last_tid"]
    assert info["n_records"] == b.n
    out["n"] += b.n


def new_out():
    return dict(batches=[], tid_runs=[], seq_ptr=[], changes=[], raw=bytearray(), unmapped=[], last_tid=0, n=0)


def via_bam(ctx, recs, names=NAMES, lens=LENS):
    out = new_out()
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "x.bam")
        bamio.write_bam(p, names, lens, [bam_side(r) for r in recs])
        with host.BamReader(p) as rd:
            for b, info in ctx.bam_batches(rd, keep_all_seq=False):
                collect(ctx, b, info, out)
    out["raw"] = strip_raw(bytes(out["raw"]))
    return out


def via_text(ctx, text, names=NAMES, cuts=(), mode=True):
    """the text in pieces cut at `cuts` -> what every call gave"""
    out = new_out()
    ctx.samdec_begin(names)
    if mode:
        ctx.samdec_sorted(False)
    bounds = [0] + [c for c in sorted(set(cuts)) if 0 < c < len(text)] + [len(text)]
    for k in range(len(bounds) - 1):
        b = ctx.samdec_decode(text[bounds[k]:bounds[k + 1]], last=k == len(bounds) - 2)
        info = ctx.samdec_lists()
        assert info["inflated_bytes"] == bounds[k + 1] - bounds[k]
        collect(ctx, b, info, out)
    out["raw"] = bytes(out["raw"])
    return out


def records_of(out):
    """the batches of a run as one list of per-record tuples: the fixed columns, the operations, whether bases + qualities ship, and their bytes"""
    recs = []
    for b in out["batches"]:
        if b is None:
            continue
        for i in range(len(b["tid"])):
            co, nc, lq, so = int(b["cigar_off"][i]), int(b["n_cigar"][i]), int(b["l_qseq"][i]), b["seq_off"][i]
            ships = so != NO_SEQ
            recs.append(tuple(int(b[k][i]) for k in FIXED) + (b["cigar"][co:co + nc].tobytes(), bool(ships),
                                                               bytes(b["seqqual"][int(so):int(so) + (lq + 1) // 2 + lq]) if ships else b""))
    return recs


def same_lists(a, w):
    assert a["changes"] == w["changes"]
    assert a["raw"] == w["raw"]
    assert a["unmapped"] == w["unmapped"]
    assert a["last_tid"] == w["last_tid"] and a["n"] == w["n"]


def same_whole(ctx, recs, names=NAMES, lens=LENS, text=None):
    """one call on the whole text against the BAM decoder's one chunk: the batch's arrays as they are"""
    text = I.body(recs, names, lens) if text is None else text
    a, w = via_text(ctx, text, names), via_bam(ctx, recs, names, lens)
    assert len(a["batches"]) == len(w["batches"]) == 1
    ab, wb = a["batches"][0], w["batches"][0]
    if wb is None or ab is None:
        assert ab is None and wb is None
    else:
        for k in COLS:
            assert k in ab and k in wb and np.array_equal(ab[k], wb[k]), k
        assert ab["max_ref_span"] == wb["max_ref_span"]
    assert a["tid_runs"] == w["tid_runs"] and a["seq_ptr"] == w["seq_ptr"]
    same_lists(a, w)
    return a, w


# ---- the shipping rule ----------------------------------------------------------------------------------------------------------------------------------------

def test_shipping_rule(ctx):
    """S first, S last, both, H S M (a first H does not ship), S H last, 50S alone, CIGAR '*', SEQ '*', odd and even lengths, XC on lines that ship and on lines
    that do not: columns, seq_off, seqqual_bytes and the bytes as the BAM decoder gives them"""
    recs = I.shipping_records()
    a, _ = same_whole(ctx, recs)
    b = a["batches"][0]
    assert [bool(s != NO_SEQ) for s in b["seq_off"]] == [I.ships(r) for r in recs]
    assert {r["qname"]: int(x) for r, x in zip(recs, b["xc"]) if x} == dict(s_last=1, s_even=1)  # (soft-clipped records alone carry it)


def test_nothing_ships(ctx):
    """a chunk without one soft clip: seqqual_bytes 0 and still a buffer behind seqqual, as the BAM decoder leaves it"""
    a, _ = same_whole(ctx, I.side_channel_one()[0])
    assert len(a["batches"][0]["seqqual"]) == 0 and a["seq_ptr"] == [True]


def test_long_read_among_short(ctx):
    """one 20,000-base clipped read among 50-base ones"""
    same_whole(ctx, I.long_read_records())


@pytest.mark.parametrize("k", I.LIST_SIZES)
def test_shipping_list_sizes(ctx, k):
    """300 lines of which k ship"""
    a, _ = same_whole(ctx, I.list_size_records(k))
    assert int((a["batches"][0]["seq_off"] != NO_SEQ).sum()) == k


# ---- the side channel -----------------------------------------------------------------------------------------------------------------------------------------

def test_side_channel_none_and_one(ctx):
    none, one = I.side_channel_one()
    a, _ = same_whole(ctx, none)
    assert a["raw"] == b"" and a["unmapped"] == []
    a, _ = same_whole(ctx, one)
    assert len(a["unmapped"]) == 1


def test_side_channel_forms(ctx):
    """first and last line of the chunk, two in a row, names of 1 and 254 bytes, l_seq 0 and 1, QUAL '*', a multi-operation CIGAR (mate unmapped, and clipped:
    the line ships too) beside '*', a '*' CIGAR whose flag lacks UNMAP; then the same lines with hex flags, CRLF and no final newline"""
    recs = I.side_channel_forms()
    a, _ = same_whole(ctx, recs)
    assert [u[0] for u in a["unmapped"]] == [r["qname"] for r in recs if I.side_channel(r)] and len(a["unmapped"]) == 10
    same_whole(ctx, recs, text=I.body(recs, hex_flags=True, crlf=True, final_newline=False))


def test_side_channel_seventy(ctx):
    """70 records in a chunk: more than a wavefront's lanes, across workgroups"""
    a, _ = same_whole(ctx, I.side_channel_seventy())
    assert len(a["unmapped"]) == 70


def test_low_quality_byte(ctx):
    """a QUAL byte of 32: refused in a side-channel line and in a line that ships, accepted in a line that is neither"""
    quiet, refused = I.low_quality_sets()
    a = via_text(ctx, I.body(quiet))
    assert a["n"] == 3 and [int(x) for x in a["batches"][0]["flag"]] == [0, 0, 0]
    for recs in refused:
        with pytest.raises(SeeksvError, match="Parse error at line 2: quality byte below 33"):
            via_text(ctx, I.body(recs))
        assert ctx.samdec_last()["refused_line"] == 2


# ---- contig changes -------------------------------------------------------------------------------------------------------------------------------------------

def test_contig_changes(ctx):
    """none (contig 0 throughout: the walk starts there); a change on the first record, on the last, two in a row; UNMAP|MUNMAP records of another contig
    between two records of one contig are no change"""
    none, recs = I.change_records()
    a, _ = same_whole(ctx, none)
    assert a["changes"] == [] and a["last_tid"] == 0 and a["tid_runs"] == [[(0, 0)]]
    a, _ = same_whole(ctx, recs)
    assert a["changes"] == I.changes_model(recs) == [(0, 1), (5, 2), (6, 0), (8, 2)] and a["last_tid"] == 2
    assert a["tid_runs"] == [[(0, 1), (2, 2), (4, 1), (5, 2), (6, 0), (8, 2)]]


def test_contig_changes_across_chunks(ctx):
    """the last contig is carried from chunk to chunk: a change on the first record of a chunk, and none when the chunk goes on where the last one stopped"""
    recs = I.across_chunks_records()
    lines = I.body(recs).split(b"\n")
    w = via_bam(ctx, recs)
    assert w["changes"] == I.changes_model(recs)
    for cut_after in range(1, len(recs)):
        a = via_text(ctx, I.body(recs), cuts=[sum(len(l) + 1 for l in lines[:cut_after])])
        assert records_of(a) == records_of(w)
        same_lists(a, w)


def test_change_list_limit(ctx):
    """65,536 contig changes in one chunk are taken, as the BAM decoder takes them; 65,537 are refused: the text is not coordinate sorted"""
    recs = I.alternating(65537)
    lens = I.ALTERNATING_LENS
    a, w = via_text(ctx, I.body(recs[:65536])), via_bam(ctx, recs[:65536], lens=lens)
    assert len(a["changes"]) == 65536 and a["changes"] == [(k, 1 - k % 2) for k in range(65536)]
    same_lists(a, w)
    assert a["tid_runs"] == w["tid_runs"] == [[]]  # (more runs than a batch's list holds: not handed out)
    with pytest.raises(SeeksvError, match="more than 65536 contig changes in one chunk: the SAM text is not coordinate sorted"):
        via_text(ctx, I.body(recs))
    with pytest.raises(SeeksvError, match="more than 65536 contig changes in one chunk"):
        via_bam(ctx, recs, lens=lens)


# ---- seams ----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twelve_whole(ctx):
    recs = I.twelve()
    text = I.body(recs)
    a, w = same_whole(ctx, recs)
    assert len(a["unmapped"]) == 6 and a["changes"] == I.changes_model(recs) and len(a["changes"]) == 3
    return text, records_of(a), a


def test_seam_at_every_offset(ctx, twelve_whole):
    """a 12-line file with one line of each kind, cut at every byte offset into two calls: the records and the concatenated lists of the one-call result"""
    text, want, whole = twelve_whole
    for cut in range(1, len(text)):
        a = via_text(ctx, text, cuts=[cut])
        assert records_of(a) == want, cut
        same_lists(a, whole)


def test_one_byte_per_call(ctx, twelve_whole):
    text, want, whole = twelve_whole
    a = via_text(ctx, text, cuts=range(1, len(text)))
    assert len(a["batches"]) == len(text) and records_of(a) == want
    same_lists(a, whole)


# ---- real reads -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sample", ["cancer", "normal"])
def test_example_sample(ctx, sample):
    """a bundled sample as text, in chunks of 64 KB cut anywhere, against the BAM decoder on the file itself"""
    path = os.path.join(EXAMPLE, sample + ".sort.bam")
    text, n_head, names = original_sam.sam_of_bam(path)
    lines = text.split(b"\n")
    rec_text = b"\n".join(lines[n_head:])
    w = new_out()
    with host.BamReader(path) as rd:
        for b, info in ctx.bam_batches(rd, keep_all_seq=False):
            collect(ctx, b, info, w)
    w["raw"] = strip_raw(bytes(w["raw"]))
    a = via_text(ctx, rec_text, names, cuts=range(65536, len(rec_text), 65536))
    assert a["n"] == w["n"] > 1000 and len(a["batches"]) > 3
    assert records_of(a) == records_of(w)
    same_lists(a, w)
    assert any(r[-2] for r in records_of(w))


# ---- the mode off, and the arguments --------------------------------------------------------------------------------------------------------------------------

def test_mode_off(ctx):
    """without ssv_samdec_sorted a decode is today's: every line ships, xc whatever the CIGAR, no tid_runs, no lists"""
    recs = I.shipping_records()
    ctx.samdec_begin(NAMES)
    b = ctx.samdec_decode(I.body(recs), last=True)
    assert b.n == len(recs) and b.n_tid_runs == 0 and not b.tid_runs
    h = ctx.batch_to_host(b)
    got = ST.batch_records(h, ST.names_to_host(ctx, ctx.samdec_names(), b.n))
    assert got == [dict(ST.expected(r), flag=r["flag"] | (4 if r["cigar"] == "*" else 0)) for r in recs]
    assert h["seq_off"].tolist() == np.cumsum([0] + [(len(r["seq"]) + 1) // 2 + len(r["seq"]) for r in recs])[:-1].tolist()
    with pytest.raises(SeeksvError, match="ssv_samdec_lists"):
        ctx.samdec_lists()


def test_arguments():
    """ssv_samdec_sorted before ssv_samdec_begin or behind the first decode, and a NULL `out`, give SSV_E_ARG"""
    E_ARG = -3
    with Context(0) as c:
        lib, h = c._lib, c._h
        assert lib.ssv_samdec_sorted(h, 0) == E_ARG
        assert lib.ssv_samdec_sorted(None, 0) == E_ARG
        c.samdec_begin(NAMES)
        assert lib.ssv_samdec_sorted(h, 0) == 0
        assert lib.ssv_samdec_sorted(h, 1) == 0      # (again before the first decode: the last call counts)
        assert lib.ssv_samdec_lists(h, None) == E_ARG
        c.samdec_decode(b"", last=False)
        assert lib.ssv_samdec_sorted(h, 0) == E_ARG
        assert c.samdec_lists()["n_records"] == 0
        c.samdec_begin(NAMES)                        # a new file starts with the mode off
        c.samdec_decode(b"", last=True)
        with pytest.raises(SeeksvError):
            c.samdec_lists()
