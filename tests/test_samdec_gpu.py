"""-m gpu: the device SAM-text decoder (ssv_samdec_*, seeksv_amd/csrc/samdec_kernels.h) through the ABI: what it decodes equals what libbam 0.1.16's
text reader decodes (tests/golden/samdec/, recorded through oracle/_ref/sam2bam) and what the host BAM reader gives for the BAM of the same records;
chunks cut anywhere give the records of the one-chunk decode; every form the grammar refuses is refused with its line number."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bamio
import readthrough_inputs as RT
import sam_text as ST
from seeksv_amd import _abi, host
from seeksv_amd.device import Context

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(RT.GOLDEN, "samdec")
NAMES, LENS = RT.NAMES, RT.LENS
TILE = 4096  # SAM_TILE: bytes of text per workgroup of the streaming kernels


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def decode(ctx, text, names=NAMES, first_line=1, **kw):
    """-> (records as sam_text.read_bam_full gives them, cigar_ends, record lines, batches)"""
    recs, ends, lines, nb = [], [], [], 0
    for b, nm in ctx.sam_batches(text, names, first_line, **kw):
        nb += 1
        assert b.mem == _abi.MEM_DEVICE and b.n_tid_runs == 0
        if not b.n:
            continue
        h = ctx.batch_to_host(b)
        recs += ST.batch_records(h, ST.names_to_host(ctx, nm, b.n))
        ends += h["cigar_ends"].tolist()
        lines.append(np.frombuffer(ST.device_to_host(ctx, b.rec, b.n * 64), dtype=_abi.RECORD_DTYPE))
        span = max([sum(l for l, op in r["cigar"] if op in (0, 2, 3, 7, 8)) for r in recs[-b.n:]] + [1])
        assert b.max_ref_span == span  # (the longest reference span of the batch, 1 when no record has one)
    return recs, ends, (np.concatenate(lines) if lines else np.zeros(0, _abi.RECORD_DTYPE)), nb


def check_lines(recs, ends, lines):
    """the 64-byte record lines and the cigar_ends column say what the columns say"""
    assert len(lines) == len(recs) == len(ends)
    for r, e, l in zip(recs, ends, lines):
        assert (int(l["tid"]), int(l["pos"]), int(l["flag"]), int(l["mapq"]), int(l["xc"]), int(l["n_cigar"]), int(l["l_qseq"]), int(l["mtid"]), int(l["mpos"]), int(l["isize"])) == \
               (r["tid"], r["pos"], r["flag"], r["mapq"], r["xc"], len(r["cigar"]), r["l_qseq"], r["mtid"], r["mpos"], r["isize"]), r["qname"]
        head = [(c[0] << 4) | c[1] for c in r["cigar"][:5]]
        assert l["cigar_head"].tolist() == head + [0] * (5 - len(head)), r["qname"]
        assert e == ST.ends_of(r), r["qname"]


def body(recs, **kw):
    return ST.text(recs, NAMES, LENS, with_header=False, **kw).encode("latin-1")


def test_forms_equal_libbam(ctx):
    """one line per well-formed form of the grammar: the batch equals what libbam's text reader decoded (forms.json)"""
    data = open(os.path.join(GOLDEN, "forms.sam"), "rb").read()
    want = json.load(open(os.path.join(GOLDEN, "forms.json")))
    lines = data.split(b"\n")
    n_hdr = sum(1 for l in lines if l.startswith(b"@"))
    assert n_hdr == want["header_lines"]
    text = b"\n".join(lines[n_hdr:])
    recs, ends, rl, _ = decode(ctx, text, want["names"], first_line=n_hdr + 1)
    assert len(recs) == len(want["records"])
    for g, w in zip(recs, want["records"]):
        assert g == w, w["qname"][:20]
    check_lines(recs, ends, rl)
    info = ctx.samdec_last()
    assert info["n_records"] == len(recs) and info["lines_consumed"] == len(recs) and info["carried_bytes"] == 0 and info["refused_line"] == 0


@pytest.fixture(scope="module")
def inputs():
    """the small file and two random seeds with qualities, mate fields and XC tags; per file: generator records, and the host BAM reader's records"""
    import tempfile
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for tag, recs in (("small", RT.small_records()), ("r0", RT.random_records(0)), ("r1", RT.random_records(1, n_names=400))):
            recs = ST.with_extras(ST.clip_positions(recs, LENS), 5)
            for r in recs:
                r["aux"] = ST.bam_aux(r)
            p = os.path.join(d, tag + ".bam")
            bamio.write_bam(p, NAMES, LENS, recs)
            with host.BamReader(p) as rd:
                b = rd.read_batch(1 << 22, keep_all_seq=True)
            ref = ST.batch_records(b, [r["qname"] for r in recs])
            out[tag] = (recs, ref)
    return out


VARIANTS = {"plain": {}, "lower_dot_hex": dict(lower=True, dot_n=True, hex_flags=True), "tags_crlf": dict(tags=True, crlf=True),
            "no_final_newline": dict(final_newline=False), "all": dict(lower=True, dot_n=True, hex_flags=True, tags=True, crlf=True, final_newline=False)}


@pytest.mark.parametrize("tag,variant", [("small", v) for v in VARIANTS] + [("r0", "plain"), ("r1", "all")])
def test_text_equals_bam_reader(ctx, inputs, tag, variant):
    """field by field against host.BamReader.read_batch(keep_all_seq=True) of the BAM of the same records: hot columns, flag, mapq, mate fields, isize,
    every CIGAR operation, cigar_ends, bases, qualities, names; xc against the generator"""
    recs, ref = inputs[tag]
    got, ends, rl, _ = decode(ctx, body(recs, **VARIANTS[variant]), chunk_bytes=100000)
    assert len(got) == len(ref)
    for g, w, r in zip(got, ref, recs):
        assert g["xc"] == int(r.get("xc", 0) != 0), r["qname"]
        assert {k: v for k, v in g.items() if k != "xc"} == {k: v for k, v in w.items() if k != "xc"}, r["qname"]
        assert g == ST.expected(r), r["qname"]
    assert ends == [ST.ends_of(w) for w in ref]
    check_lines(got, ends, rl)


def five():
    rng = np.random.RandomState(3)
    recs = [RT.rec(rng, "a", 0, 100, "30M20S"), RT.rec(rng, "bb" * 20, 1, 200, "10S5M2D5M", flag=16, mapq=3), RT.rec(rng, "c", 2, 300, "7M"),
            RT.rec(rng, "d_d", 0, 400, "3S40M3S", iupac=True), RT.rec(rng, "e", 1, 500, "12M")]
    recs = ST.with_extras(recs, 1)
    recs[2]["xc"], recs[2]["qual"] = 7, bytes(range(7))
    return recs


def test_one_byte_per_call(ctx):
    """a five-line file handed over one byte per call: the records and names of the one-chunk decode"""
    recs = five()
    for kw in ({}, dict(crlf=True, tags=True), dict(final_newline=False)):
        text = body(recs, **kw)
        whole = decode(ctx, text)
        assert [g for g in whole[0]] == [ST.expected(r) for r in recs]
        piece = decode(ctx, text, cuts=range(1, len(text)))
        assert piece[0] == whole[0] and piece[1] == whole[1] and piece[3] == len(text)
        check_lines(piece[0], piece[1], piece[2])


@pytest.mark.parametrize("crlf", [False, True], ids=["lf", "crlf"])
def test_seam_at_every_offset(ctx, crlf):
    """one seam at every byte offset across two adjacent lines (the lines before and behind them stay whole)"""
    recs = five()
    text = body(recs, crlf=crlf, tags=True)
    eol = b"\r\n" if crlf else b"\n"
    starts = [0]
    for _ in recs:
        starts.append(text.index(eol, starts[-1]) + len(eol))
    want = [ST.expected(r) for r in recs]
    for cut in range(starts[1], starts[3] + 1):
        got = decode(ctx, text, cuts=[cut])
        assert got[0] == want, cut
        info = ctx.samdec_last()
        assert info["lines_consumed"] == 5 and info["carried_bytes"] == 0


def test_chunks_shorter_than_a_line(ctx):
    """chunks of 37 bytes against lines of ~300: lines are carried over many calls, names survive the carry"""
    recs = ST.with_extras(ST.clip_positions(RT.random_records(2, n_names=60), LENS), 2)
    text = body(recs, tags=True)
    got = decode(ctx, text, chunk_bytes=37)
    assert got[0] == [ST.expected(r) for r in recs]
    check_lines(got[0], got[1], got[2])


def simple(k, name=None, seq_len=50):
    rng = np.random.RandomState(k)
    return RT.rec(rng, name or f"s{k}", k % 3, 100 + k, f"{seq_len - 10}M10S", flag=16 * (k & 1), mapq=k % 61)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_line_counts(ctx, n):
    """numbers of lines around the wavefront and workgroup sizes of the per-line kernels"""
    recs = [simple(k) for k in range(n)]
    got = decode(ctx, body(recs))
    assert got[0] == [ST.expected(r) for r in recs]
    check_lines(got[0], got[1], got[2])
    assert ctx.samdec_last()["n_records"] == n


def padded_to(length, first=0):
    """record text of exactly `length` bytes: short records, the last one's name stretched to fit"""
    last = simple(first + 999, name="p")
    recs, k = [], first
    while length - len(body(recs + [last])) > 250:
        recs.append(simple(k))
        k += 1
    room = length - len(body(recs + [last]))
    assert 0 <= room <= 250
    last["qname"] = "p" * (1 + room)
    recs.append(last)
    text = body(recs)
    assert len(text) == length
    return recs, text


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_file_length_around_the_tile(ctx, delta):
    """a file as long as the streaming tile and one byte either side: its last newline is the tile's last byte (0) or the next tile's first (1); with and
    without the final newline, whole and cut at the tile's edge"""
    recs, text = padded_to(TILE + delta)
    want = [ST.expected(r) for r in recs]
    for t in (text, text[:-1]):
        for cuts in (None, [TILE - 1], [TILE]):
            got = decode(ctx, t, cuts=[c for c in cuts if c < len(t)] if cuts else None)
            assert got[0] == want, (len(t), cuts)


def test_newline_first_and_last_byte_of_a_tile(ctx):
    """a newline as the last byte of the first tile, another as the first byte of the third"""
    r1, t1 = padded_to(TILE)
    r2, t2 = padded_to(TILE + 1, first=2000)
    tail = [simple(5000), simple(5001)]
    text = t1 + t2 + body(tail)
    assert text[TILE - 1:TILE] == b"\n" and text[2 * TILE:2 * TILE + 1] == b"\n"
    got = decode(ctx, text)
    assert got[0] == [ST.expected(r) for r in r1 + r2 + tail]
    check_lines(got[0], got[1], got[2])


def test_long_read_among_short_ones(ctx):
    """one read of 20,000 bases with a 3,000-operation CIGAR among short ones: a line that spans many tiles"""
    rng = np.random.RandomState(9)
    ops = []
    for k in range(1499):
        ops += [(6, 0), (int(rng.randint(1, 4)), 1 if k % 2 else 2)]
    ops += [(5, 0), (0, 4)]
    assert len(ops) == 3000
    q = sum(l for l, op in ops if op in (0, 1, 4))
    ops[-1] = (20000 - q, 4)
    cig = "".join(f"{l}{'MIDNSHP=X'[op]}" for l, op in ops)
    long_rec = RT.rec(rng, "long", 0, 1000, cig, iupac=True)
    long_rec["qual"] = bytes(rng.randint(0, 94, 20000).astype(np.uint8).tolist())
    assert len(long_rec["seq"]) == 20000
    recs = [simple(k) for k in range(30)] + [long_rec] + [simple(k) for k in range(30, 70)]
    text = body(recs)
    want = [ST.expected(r) for r in recs]
    got = decode(ctx, text)
    assert got[0] == want
    check_lines(got[0], got[1], got[2])
    assert decode(ctx, text, chunk_bytes=5000)[0] == want


GOOD = "r\t0\tchrA\t100\t60\t5M\t*\t0\t0\tACGTA\tIIIII"


def bad_line(**f):
    v = dict(name="r", flag="0", rname="chrA", pos="100", mapq="60", cigar="5M", rnext="*", pnext="0", tlen="0", seq="ACGTA", qual="IIIII")
    v.update(f)
    return "\t".join(v[k] for k in ("name", "flag", "rname", "pos", "mapq", "cigar", "rnext", "pnext", "tlen", "seq", "qual"))


REFUSED = [
    ("ten_fields", "r\t0\tchrA\t100\t60\t5M\t*\t0\t0\tACGTA", "fewer than 11 fields"),
    ("one_field", "r", "fewer than 11 fields"),
    ("empty_line", "", "empty line"),
    ("cr_only", "\r", "empty line"),
    ("at_line", "@CO\tlate header line", "header line"),
    ("empty_name", bad_line(name=""), "read name"),
    ("name_255", bad_line(name="n" * 255), "read name"),
    ("flag_text", bad_line(flag="pP"), "number"),
    ("flag_big", bad_line(flag="65536"), "number"),
    ("flag_hex_bad", bad_line(flag="0x1g"), "number"),
    ("flag_leading_zero", bad_line(flag="016"), "number"),   # (octal to libbam's strtol)
    ("pos_text", bad_line(pos="1x"), "number"),
    ("pos_empty", bad_line(pos=""), "number"),
    ("pos_negative", bad_line(pos="-1"), "number"),
    ("pos_big", bad_line(pos="2147483648"), "number"),
    ("mapq_300", bad_line(mapq="300"), "number"),
    ("pnext_text", bad_line(pnext="z"), "number"),
    ("tlen_text", bad_line(tlen="--1"), "number"),
    ("tlen_big", bad_line(tlen="2147483648"), "number"),
    ("cigar_char", bad_line(cigar="5Q"), "invalid CIGAR character"),
    ("cigar_lower", bad_line(cigar="5m"), "invalid CIGAR character"),
    ("cigar_no_len", bad_line(cigar="M"), "without a length"),
    ("cigar_no_len2", bad_line(cigar="3M2IS"), "without a length"),
    ("cigar_no_op", bad_line(cigar="5M3"), "invalid CIGAR character"),
    ("cigar_empty", bad_line(cigar=""), "invalid CIGAR character"),
    ("cigar_len_big", bad_line(cigar="268435456M", seq="*", qual="*"), "number"),
    ("cigar_many", bad_line(cigar="1M" * 65536, seq="*", qual="*"), "more than 65535"),
    ("cigar_seq", bad_line(cigar="4M"), "CIGAR and sequence length are inconsistent"),
    ("seq_qual", bad_line(qual="IIII"), "sequence and quality are inconsistent"),
    ("star_seq_qual", bad_line(seq="*", qual="IIII"), "sequence and quality are inconsistent"),
    ("qual_low", bad_line(qual="II II"), "quality byte below 33"),
    ("nul_byte", bad_line(seq="AC\0TA"), "NUL byte"),
    ("nul_in_tag", bad_line() + "\tXX:Z:a\0b", "NUL byte"),
]


@pytest.mark.parametrize("tag,line,reason", REFUSED, ids=[t for t, _, _ in REFUSED])
def test_refused_forms(ctx, tag, line, reason):
    """every refused form once in the middle of a chunk and once as the first line of a second chunk: SSV_E_ARG, 'Parse error at line N: reason' with N
    counted across chunks and the header, and the context takes a new file afterwards"""
    lib = _abi.hip_lib()
    good = [GOOD.replace("r\t", f"g{k}\t") for k in range(6)]
    first_line = 4  # (a header of three lines)
    for where in ("inside", "second_chunk"):
        lines = good[:3] + [line] + good[3:]
        text = ("\n".join(lines) + "\n").encode("latin-1")
        cut = len(("\n".join(lines[:3]) + "\n").encode("latin-1"))
        ctx.samdec_begin(NAMES, first_line)
        b = _abi.Batch()
        parts = [text] if where == "inside" else [text[:cut], text[cut:]]
        rcs = []
        for k, part in enumerate(parts):
            buf = C.create_string_buffer(part, len(part))
            rcs.append(lib.ssv_samdec_decode(ctx._h, buf, len(part), _abi.MEM_HOST, int(k == len(parts) - 1), C.byref(b)))
        assert rcs == ([-3] if where == "inside" else [0, -3]), (where, rcs)
        err = lib.ssv_last_error(ctx._h).decode()
        assert err.startswith(f"Parse error at line {first_line + 3}: "), err
        assert reason in err, err
        info = ctx.samdec_last()
        assert info["refused_line"] == first_line + 3 and reason in info["refused_reason"]
        assert lib.ssv_samdec_decode(ctx._h, None, 0, _abi.MEM_HOST, 1, C.byref(b)) == -4  # (only a new file is accepted now)
        got = decode(ctx, ("\n".join(good) + "\n").encode())
        assert [g["qname"] for g in got[0]] == [f"g{k}" for k in range(6)]


def test_refused_line_is_the_first_of_several(ctx):
    """two malformed lines far apart (different workgroups, different kernels): the message names the first"""
    lines = [GOOD] * 700
    lines[650] = bad_line(pos="x")
    lines[300] = bad_line(qual="II\x1fII")
    lines[500] = "short\tline"
    with pytest.raises(Exception, match="Parse error at line 301: quality byte below 33"):
        decode(ctx, ("\n".join(lines) + "\n").encode("latin-1"))
    lines[300] = GOOD
    with pytest.raises(Exception, match="Parse error at line 501: fewer than 11 fields"):
        decode(ctx, ("\n".join(lines) + "\n").encode("latin-1"))


def test_unfinished_last_line_without_last_is_carried(ctx):
    """without `last` a final line without its newline is not a record yet; bytes == 0 with last flushes it"""
    text = (GOOD + "\n" + GOOD.replace("r\t", "tail\t")).encode()
    ctx.samdec_begin(NAMES, 1)
    b = ctx.samdec_decode(text, last=False)
    assert b.n == 1
    info = ctx.samdec_last()
    assert info["carried_bytes"] == len(GOOD) + 3 and info["lines_consumed"] == 1
    b = ctx.samdec_decode(b"", last=True)
    assert b.n == 1 and ST.names_to_host(ctx, ctx.samdec_names(), 1) == ["tail"]
    assert ctx.samdec_last()["lines_consumed"] == 2


def test_device_memory_input(ctx):
    """text that lies in device memory already (SSV_MEM_DEVICE) decodes like host text"""
    recs = [simple(k) for k in range(40)]
    text = body(recs)
    hip = ST.hip_runtime()
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), len(text) + 3) == 0
    try:
        # (an odd address: the decoder copies the text behind its carried line, wherever it comes from)
        assert hip.hipMemcpy(dev.value + 3, C.create_string_buffer(text, len(text)), len(text), 1) == 0
        lib = _abi.hip_lib()
        ctx.samdec_begin(NAMES, 1)
        b = _abi.Batch()
        assert lib.ssv_samdec_decode(ctx._h, dev.value + 3, len(text), _abi.MEM_DEVICE, 1, C.byref(b)) == 0
        got = ST.batch_records(ctx.batch_to_host(b), ST.names_to_host(ctx, ctx.samdec_names(), b.n))
    finally:
        hip.hipFree(dev)
    assert got == [ST.expected(r) for r in recs]


def test_state_and_arguments():
    """calls out of sequence return SSV_E_STATE, bad arguments SSV_E_ARG"""
    lib = _abi.hip_lib()
    with Context(0) as c:
        b, nm, info = _abi.Batch(), _abi.Names(), _abi.SamdecInfo()
        buf = C.create_string_buffer(b"x\n", 2)
        assert lib.ssv_samdec_decode(c._h, buf, 2, 0, 1, C.byref(b)) == -4
        assert lib.ssv_samdec_names(c._h, C.byref(nm)) == -4
        assert lib.ssv_samdec_last(c._h, C.byref(info)) == -4
        assert lib.ssv_samdec_prefetch(c._h, buf, 2) == -4
        assert lib.ssv_samdec_begin(c._h, None) == -3
        assert lib.ssv_samdec_begin(None, None) == -3
        p = _abi.SamdecParams(2, 0, None, 1)
        assert lib.ssv_samdec_begin(c._h, C.byref(p)) == -3          # names missing
        arr = (C.c_char_p * 1)(b"chrA")
        assert lib.ssv_samdec_begin(c._h, C.byref(_abi.SamdecParams(1, 0, arr, 0))) == -3   # lines count from 1
        assert lib.ssv_samdec_begin(c._h, C.byref(_abi.SamdecParams(-1, 0, arr, 1))) == -3
        assert lib.ssv_samdec_begin(c._h, C.byref(_abi.SamdecParams(1, 0, arr, 1))) == 0
        assert lib.ssv_samdec_names(c._h, C.byref(nm)) == -4           # nothing decoded yet
        assert lib.ssv_samdec_decode(c._h, buf, 2, 0, 0, None) == -3
        assert lib.ssv_samdec_decode(c._h, None, 2, 0, 0, C.byref(b)) == -3
        assert lib.ssv_samdec_decode(c._h, buf, 2, 7, 0, C.byref(b)) == -3
        assert lib.ssv_samdec_prefetch(c._h, None, 2) == -3
        assert lib.ssv_samdec_last(c._h, None) == -3
        assert lib.ssv_samdec_decode(c._h, None, 0, 0, 1, C.byref(b)) == 0 and b.n == 0   # an empty file
        assert lib.ssv_samdec_names(c._h, C.byref(nm)) == 0
        assert lib.ssv_samdec_decode(c._h, None, 0, 0, 1, C.byref(b)) == -4                # behind the file's end
        assert lib.ssv_samdec_begin(c._h, C.byref(_abi.SamdecParams(0, 0, None, 1))) == 0  # no contigs: every RNAME is unknown
        line = (GOOD + "\n").encode()
        assert lib.ssv_samdec_decode(c._h, C.create_string_buffer(line, len(line)), len(line), 0, 1, C.byref(b)) == 0 and b.n == 1
        assert c.batch_to_host(b)["tid"].tolist() == [-1]


def test_prefetch_overlaps_and_equals(ctx):
    """chunks announced ahead (ssv_samdec_prefetch) decode to the same records"""
    lib = _abi.hip_lib()
    recs = [simple(k) for k in range(300)]
    text = body(recs)
    want = [ST.expected(r) for r in recs]
    step = 7001
    parts = [C.create_string_buffer(text[a:a + step], len(text[a:a + step])) for a in range(0, len(text), step)]
    ctx.samdec_begin(NAMES, 1)
    got = []
    assert lib.ssv_samdec_prefetch(ctx._h, parts[0], len(parts[0]) - 1) == 0   # (announced with another size: given up, not decoded)
    assert lib.ssv_samdec_prefetch(ctx._h, parts[0], len(parts[0])) == 0
    for k, part in enumerate(parts):
        for ahead in parts[k + 1:k + 3]:
            assert lib.ssv_samdec_prefetch(ctx._h, ahead, len(ahead)) == 0
        b = _abi.Batch()
        assert lib.ssv_samdec_decode(ctx._h, part, len(part), 0, int(k == len(parts) - 1), C.byref(b)) == 0
        if b.n:
            got += ST.batch_records(ctx.batch_to_host(b), ST.names_to_host(ctx, ctx.samdec_names(), b.n))
    assert got == want
