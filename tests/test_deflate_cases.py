"""CPU: the catalogue of hand-written DEFLATE streams (tests/deflate_cases.py, written by tests/deflate_writer.py) is what it claims to be, and the CPU build of
the device decoder (inflate_core.h) takes it.  zlib is the reference: it inflates every valid case to exactly the expanded bytes and refuses every malformed one;
then tests/native/inflate_streams_check.cpp runs the decoder's three forms over the same streams, plain and under AddressSanitizer + UBSan.  The `*_present`
tests hold the catalogue itself to the ranges the kernels branch on, so that a later edit of the catalogue cannot quietly drop one; the carrier tests hold the BAM
files the GPU module decodes (test_bamdec_streams_gpu.py) against gzip's view of the same bytes and against the host reader."""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bamio
import deflate_cases as D
from deflate_writer import Bits, Dynamic, Fixed, Stored, deflate, distance_symbol, equal_lengths, kraft_sum, ladder, length_symbol, stream_bits
from seeksv_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAT = D.catalogue()
BY_NAME = {c.name: c for c in CAT}


def _matches(case):
    """(o, len, dist, alt, literals since the previous match, index in its block, block index, kinds of block the run's literals came from)"""
    run, kinds = 0, set()
    for o, t, ti, bi, stored in D.tokens_with_positions(case):
        if type(t) is int:
            run += 1
            kinds.add("stored" if stored else "huffman")
        elif type(t) is not Bits:
            yield o, t[0], t[1], len(t) > 2, run, ti, bi, frozenset(kinds)
            run, kinds = 0, set()


ALL_MATCHES = {c.name: list(_matches(c)) for c in CAT}


# ---- the writer and the catalogue against zlib ----
def test_zlib_inflates_every_valid_case_to_the_expanded_tokens():
    for c in CAT:
        z = zlib.decompressobj(-15)
        got = z.decompress(D.payload(c))
        assert z.eof and not z.unused_data and got == D.expected(c), c.name
        assert 1 <= len(got) <= 65536
    assert len(CAT) >= 400


ZLIB_SAYS = {"fixed_distance_code_30": "invalid distance code", "fixed_length_code_286": "invalid literal/length code", "distance_1_at_output_0": "invalid distance too far back",
             "distance_32768_at_output_32767": "invalid distance too far back", "hlit_30": "too many length or distance symbols", "hdist_31": "too many length or distance symbols",
             "oversubscribed_literal_code": "invalid literal/lengths set", "incomplete_literal_code": "invalid literal/lengths set", "incomplete_two_symbol_distance_code": "invalid distances set",
             "single_distance_code_of_2_bits": "invalid distances set", "unused_pattern_of_one_bit_distance_code": "invalid distance code", "single_symbol_code_length_code": "invalid code lengths set",
             "repeat_16_as_first_length": "invalid bit length repeat", "run_past_hlit_plus_hdist": "invalid bit length repeat", "no_end_of_block_code": "missing end-of-block",
             "stored_len_nlen_mismatch": "invalid stored block lengths", "btype_3": "invalid block type"}


def test_zlib_refuses_every_malformed_case_for_the_reason_it_was_built_for():
    bad = D.malformed()
    assert len(bad) == 21
    for b in bad:
        ok, _ = D.zlib_verdict(b.data, b.isize)
        assert not ok, b.name
        if b.name in ZLIB_SAYS:
            with pytest.raises(zlib.error, match=ZLIB_SAYS[b.name]):
                zlib.decompressobj(-15).decompress(b.data)
        else:   # the structure is fine: the stream is too short, not final, or inflates to another size than the container says
            z = zlib.decompressobj(-15)
            got = z.decompress(b.data)
            assert (not z.eof) or len(got) != b.isize, b.name
    assert {"stored_len_past_the_payload", "output_one_more_than_isize", "output_one_less_than_isize", "last_block_not_final"} == {b.name for b in bad} - set(ZLIB_SAYS)


# ---- the CPU build of the decoder ----
@pytest.fixture(scope="module")
def stream_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("streams") / "catalogue.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(CAT) + len(D.malformed())))
        for c in CAT:
            nm, p, e = c.name.encode(), D.payload(c), D.expected(c)
            f.write(struct.pack("<I", len(nm)) + nm + struct.pack("<III", 1, len(p), len(e)) + p + e)
        for b in D.malformed():
            nm = b.name.encode()
            f.write(struct.pack("<I", len(nm)) + nm + struct.pack("<III", 0, len(b.data), b.isize) + b.data)
    return path


def _build_and_run(tmp_path, stream_file, flags, env=None, n_valid=len(CAT), n_bad=len(D.malformed()), more=()):
    exe = str(tmp_path / "inflate_streams_check")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "seeksv_amd", "csrc"), os.path.join(ROOT, "tests", "native", "inflate_streams_check.cpp"), "-o", exe] + flags)
    r = subprocess.run([exe, stream_file] + list(more), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{n_valid} valid streams decoded, {n_bad} malformed streams refused, 0 bad" in r.stdout, r.stdout
    return r


def test_cpu_decoder_takes_the_catalogue_and_refuses_the_malformed(tmp_path, stream_file):
    """inflate_core.h in its three forms - DirectOut / PlainTab, TokenOut / PlainTabLim + resolve_tokens at four output misalignments, RingReader at four input
    misalignments: the bytes, guard bytes on both sides of the output, to.n <= token_capacity; every malformed stream refused by every form"""
    _build_and_run(tmp_path, stream_file, ["-O2"])


def test_cpu_decoder_is_clean_under_asan_and_ubsan(tmp_path, stream_file):
    """the same stand-alone program with -fsanitize=address,undefined: no read or write outside a buffer, no undefined shift, on the valid and the malformed streams"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")   # (the runtimes linked statically: nothing to preload)
    r = _build_and_run(tmp_path, stream_file, ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"], env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.parametrize("level,period", [(1, 32700), (6, 32741), (12, 32767)])
def test_libdeflate_fixtures_hold_what_zlib_never_writes(tmp_path, level, period):
    """tests/golden/bamdec/libdeflate.*.bam (made by tests/golden/make_libdeflate_bam.py): every block's payload through the decoder's CPU build, and the largest match
    distance among its tokens is at least the period of the long record's qualities - above zlib's 32,506"""
    data = open(os.path.join(ROOT, "tests", "golden", "bamdec", f"libdeflate.{level}.bam"), "rb").read()
    assert 100_000 < len(data) < 1 << 20
    items, at = [], 0
    while at < len(data):
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        pl = data[at + 18:at + bsize - 8]
        raw = zlib.decompressobj(-15).decompress(pl)
        assert len(raw) == struct.unpack_from("<I", data, at + bsize - 4)[0] and zlib.crc32(raw) == struct.unpack_from("<I", data, at + bsize - 8)[0]
        if raw:
            items.append((pl, raw))
        at += bsize
    path = str(tmp_path / "blocks.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for i, (pl, raw) in enumerate(items):
            nm = b"block%d" % i
            f.write(struct.pack("<I", len(nm)) + nm + struct.pack("<III", 1, len(pl), len(raw)) + pl + raw)
    r = _build_and_run(tmp_path, path, ["-O2"], n_valid=len(items), n_bad=0, more=["dist"])
    far = int(r.stdout.split("largest match distance ")[1].split()[0])
    assert 32506 < period <= far <= 32767, r.stdout   # (libdeflate's own limit is 32,767; the period is the nearest source of the long record's qualities)


# ---- what the catalogue holds ----
def _dynamic_blocks():
    for c in CAT:
        for b in c.blocks:
            if isinstance(b, Dynamic):
                yield c, b


def _symbol_counts(b):
    fl, fd = {}, {}
    for t in b.tokens:
        if type(t) is int:
            fl[t] = fl.get(t, 0) + 1
        elif type(t) is not Bits:
            s = length_symbol(t[0], len(t) > 2)[0]
            fl[s] = fl.get(s, 0) + 1
            s = distance_symbol(t[1])[0]
            fd[s] = fd.get(s, 0) + 1
    return fl, fd


def test_code_lengths_present():
    top_lit, top_len, top_dist, ll_used, d_used = set(), set(), set(), [], []
    for c, b in _dynamic_blocks():
        fl, fd = _symbol_counts(b)
        lits, lens = {s: n for s, n in fl.items() if s < 256}, {s: n for s, n in fl.items() if s > 256}
        if lits:
            top_lit.add(b.ll[max(lits, key=lits.get)])
        if lens:
            top_len.add(b.ll[max(lens, key=lens.get)])
        if fd:
            top_dist.add(b.dd[max(fd, key=fd.get)])
        ll_used.append({b.ll[s] for s in fl})
        d_used.append({b.dd[s] for s in fd})
    assert set(range(D.WV_LT + 1, 16)) <= top_lit, "a block's MOST frequent literal on a code of 11..15 bits"
    assert set(range(D.WV_LT + 1, 16)) <= top_len, "... and its most frequent length symbol"
    assert set(range(D.WV_DT + 1, 16)) <= top_dist, "a block's most frequent distance symbol on a code of 9..15 bits"
    assert any({D.WV_LT, D.WV_LT + 1} <= u for u in ll_used) and any({D.WV_DT, D.WV_DT + 1} <= u for u in d_used), "codes of exactly the look-up's bits and one more, side by side"
    dyn = [b for _, b in _dynamic_blocks()]
    assert any(sorted(l for l in b.dd if l) == [1] and _symbol_counts(b)[1] for b in dyn), "a single distance code of one bit, in use"
    assert any(not any(b.dd) for b in dyn), "no distance code at all"
    assert {257, 286} <= {b.hlit for b in dyn} and {1, 30} <= {b.hdist for b in dyn}
    assert any(sorted(l for l in b.ll if l) == ladder() for b in dyn) and any(sorted(l for l in b.ll if l) == equal_lengths(256) for b in dyn)
    for b in dyn:   # every valid block's codes are complete, but for the distance codes of one 1-bit symbol or none
        assert kraft_sum(b.ll) == 32768 and (kraft_sum(b.dd) == 32768 or [l for l in b.dd if l] in ([1], []))
    assert 19 in {b.n_cl() for b in dyn} and min(b.n_cl() for b in dyn) < 19 and any(b.hclen == "min" for b in dyn)


def test_code_length_runs_present():
    ops_all = [(b, b.ops) for _, b in _dynamic_blocks()]
    assert any((18, 127, 7) in ops for _, ops in ops_all), "a run of 138 zeros"
    assert any((16, 3, 2) in ops for _, ops in ops_all), "six repeats"
    crossing_zero = crossing_repeat = after17 = after18 = False
    for b, ops in ops_all:
        at = 0
        for i, (s, xv, xb) in enumerate(ops):
            n = 1 if s < 16 else 3 + xv if s in (16, 17) else 11 + xv
            if at < b.hlit < at + n:
                crossing_zero |= s in (17, 18)
                crossing_repeat |= s == 16 and b.ll[at - 1] != 0
            if s == 16 and i:
                after17 |= ops[i - 1][0] == 17
                after18 |= ops[i - 1][0] == 18
            at += n
        assert at == b.hlit + b.hdist
    assert crossing_zero and crossing_repeat, "runs that cross from the literal/length lengths into the distance lengths"
    assert after17 and after18, "a 16 directly behind a 17 and behind an 18"


def test_longest_header_and_uniform_codes_present():
    c = BY_NAME["longest_header_at_bit_31"]
    starts = []
    deflate(c.blocks, starts)
    assert c.blocks[1].header_bits() == 17 + 19 * 3 + 316 * 7 == 2286 and starts[1] % 32 == 31
    seen = {}
    for c in CAT:
        if c.family != "uniform":
            continue
        starts = []
        deflate(c.blocks, starts)
        b = c.blocks[-1]
        lens = {8 if t < 144 else 9 for t in b.tokens} if isinstance(b, Fixed) else {b.ll[t] for t in b.tokens}
        assert len(lens) == 1, "one code length for every symbol of the block: a decoder that starts at a wrong bit stays wrong"
        kind = ("fixed" if isinstance(b, Fixed) else "dynamic", lens.pop())
        seen.setdefault(kind, set()).add(starts[-1] % 8)
        assert len(D.payload(c)) >= 2.5 * D.WV_WINDOW_BYTES, "several windows of pass 1"
    assert seen == {("fixed", 9): set(range(8)), ("fixed", 8): set(range(8)), ("dynamic", 8): set(range(8))}


def test_lengths_and_distances_present():
    lens, alts, dsyms, first_legal, at_end, overlaps = set(), 0, set(), set(), set(), set()
    for c in CAT:
        total = len(D.expected(c))
        for o, n, d, alt, run, ti, bi, kinds in ALL_MATCHES[c.name]:
            lens.add(n)
            alts += alt
            s, xv, xb = distance_symbol(d)
            if xv == 0:
                dsyms.add((s, "min"))
            if xv == (1 << xb) - 1:
                dsyms.add((s, "max"))
            if o == d:
                first_legal.add(d)
            if o + n == total:
                at_end.add(d)
            overlaps.add((d, n))
    assert lens == set(range(3, 259)) and alts >= 3
    assert dsyms == {(s, w) for s in range(30) for w in ("min", "max")}
    assert set(D.FAR_DISTS) <= first_legal and set(D.FAR_DISTS) <= at_end and max(D.FAR_DISTS) == 32768
    assert {(d, n) for d in range(1, 81) for n in D.OVERLAP_LENS} <= overlaps
    assert all((n, n) in overlaps and (n - 1, n) in overlaps and (n + 1, n) in overlaps for n in D.OVERLAP_LENS if n <= 79)


def test_chains_runs_and_capacity_present():
    for n in (3, 16, 258):
        m = ALL_MATCHES[f"chain_{n}_{n}"]
        assert len(m) > 64 and all(x[1] == n and x[2] == n and x[4] == 0 for x in m[1:])
    # a source that spans two or more earlier holes and the literals between them, within the 64 tokens before it
    m = ALL_MATCHES["chain_sources_span_holes"]
    spans = 0
    for i, (o, n, d, *_rest) in enumerate(m):
        lo, hi = o - d, o - d + min(n, d)
        holes = [x for x in m[max(0, i - 63):i] if x[0] < hi and x[0] + x[1] > lo]
        if len(holes) >= 2 and any(a[0] + a[1] < b[0] for a, b in zip(holes, holes[1:])):
            spans += 1
    assert spans >= 200
    # literal runs in front of a match
    seen = set()
    for c in CAT:
        if c.family != "literal_runs":
            continue
        for o, n, d, alt, run, ti, bi, kinds in ALL_MATCHES[c.name]:
            where = "payload_start" if o == run else "block_start" if ti == run or ti == 0 else "mid_block"
            for k in kinds or {"none"}:
                seen.add((run, k, where))
    for r in D.LITERAL_RUNS[1:] + (D.LONG_RUN,):
        assert (r, "huffman", "payload_start") in seen and (r, "stored", "payload_start") in seen, r
    for r in D.LITERAL_RUNS[1:]:
        assert (r, "huffman", "block_start") in seen and (r, "huffman", "mid_block") in seen and (r, "stored", "block_start") in seen, r
    assert (0, "none", "block_start") in seen and (0, "none", "mid_block") in seen
    for k in ("huffman", "stored"):
        assert any(run >= D.LONG_RUN and o > run and k in kinds for c in CAT for o, n, d, alt, run, ti, bi, kinds in ALL_MATCHES[c.name]), "the long run behind a match, too"
    # the token count at token_capacity
    c = BY_NAME["all_3_byte_matches_65535"]
    m = ALL_MATCHES[c.name]
    assert len(D.expected(c)) == 65535 and all(x[1] == 3 and x[4] == 0 for x in m[1:]) and len(m) == 65535 // 3 - 1
    assert D.token_capacity(65535) - len(m) < 65535 // 510 + 6
    # the largest symbols: 15 + 5 + 15 + 13 bits, more of them in a row than a segment holds, in a block longer than a window
    c = BY_NAME["largest_symbols_48_bits"]
    b = c.blocks[-1]
    big = [b.ll[length_symbol(t[0])[0]] + length_symbol(t[0])[2] + b.dd[distance_symbol(t[1])[0]] + distance_symbol(t[1])[2] for t in b.tokens if type(t) is tuple]
    assert big.count(48) >= 64 and stream_bits([b]) > 64 * D.WV_SEG_BITS


def test_window_sweep_present():
    by_setting = {}
    for c in CAT:
        if c.family == "window_sweep":
            s = by_setting.setdefault(c.name.rsplit("_", 1)[0], set())
            s.update((n, d) for o, n, d, *_ in ALL_MATCHES[c.name])
    assert len(by_setting) == 3
    full = {(n, d) for n in D.SWEEP_LENS for d in D.SWEEP_DISTS}
    assert full <= by_setting["window_sweep_plain"]
    for name, s in by_setting.items():
        assert {d for n, d in s if n in D.SWEEP_LENS} >= set(D.SWEEP_DISTS), name
        for n in D.SWEEP_LENS:
            assert len({d for m, d in s if m == n}) >= len(D.SWEEP_DISTS) // 3, (name, n)
    assert min(D.SWEEP_DISTS) < D.RW_KEEP < D.RW_WIN < max(D.SWEEP_DISTS) and {D.RW_SMALL, D.RW_SMALL + 1, 16, 17} <= set(D.SWEEP_LENS)


def test_block_structure_present():
    stored_phase, empty_stored, empty_fixed, one_symbol, back_over_border, into_stored, last_bits, sizes = set(), set(), 0, 0, 0, 0, set(), set()
    for c in CAT:
        starts = []
        deflate(c.blocks, starts)
        kinds = {type(b).__name__ for b in c.blocks}
        for i, b in enumerate(c.blocks):
            if isinstance(b, Stored):
                if i and not isinstance(c.blocks[i - 1], Stored):
                    stored_phase.add(starts[i] % 8)
                if not b.data:
                    empty_stored.add(b.final)
            elif isinstance(b, Fixed) and not b.tokens:
                empty_fixed += 1
            elif len(b.tokens) == 1:
                one_symbol += 1
        block_start, o_start = {}, 0
        for o, t, ti, bi, stored in D.tokens_with_positions(c):
            if ti == 0:
                block_start[bi] = o
            if type(t) is tuple and len(c.blocks) > 1 and o - t[1] < block_start[bi]:
                back_over_border += 1
                src_block = max(k for k, s in block_start.items() if s <= o - t[1])
                into_stored += isinstance(c.blocks[src_block], Stored)
        last_bits.add(stream_bits(c.blocks) % 8)
        sizes.add(len(D.expected(c)))
        if c.name.startswith("stored_at_phase"):
            assert kinds == {"Stored", "Fixed", "Dynamic"}
    assert stored_phase == set(range(8)), "a stored block's header at every bit phase behind a Huffman block"
    assert empty_stored == {True, False} and empty_fixed >= 1000 and one_symbol >= 50
    assert max(sum(1 for b in c.blocks if not b.tokens) for c in CAT) >= 2000
    assert back_over_border >= 100 and into_stored >= 20
    assert {0, 1} <= last_bits, "the stream's last bit on a byte edge, and followed by seven pad bits"
    assert set(D.SIZES) <= sizes


# ---- the carrier files ----
@pytest.fixture(scope="module")
def carriers(tmp_path_factory):
    return D.write_carriers(str(tmp_path_factory.mktemp("carriers")))


def test_carriers_are_valid_bam_around_the_payloads(carriers):
    aligns_all, sweep = set(), {}
    assert 4 <= len(carriers) <= 10
    for fname, (path, names, aligns) in carriers.items():
        assert os.path.getsize(path) < 8 << 20
        raw = gzip.open(path, "rb").read()   # (every block's CRC32 and ISIZE are checked by gzip)
        tnames, recs = bamio.read_bam_records(path)
        assert tnames == D.NAMES and len([r for r in recs if r["qname"][0] == "c"]) == len(names) and len(recs) >= len(names) * 5 // 4 - 1
        at, recs = len(D.bam_header_bytes()), iter(recs)
        for nm in names:
            r = next(recs)
            if r["qname"][0] == "u":   # (the small unmapped record in front of every fourth one)
                assert r["flag"] & 12
                at += 4 + struct.unpack_from("<i", raw, at)[0]
                r = next(recs)
            e = D.expected(BY_NAME[nm])
            bs, = struct.unpack_from("<i", raw, at)
            assert raw[at + 4 + bs - len(e):at + 4 + bs] == e, nm   # the record's seq + qual end with the case's bytes
            assert r["l_qseq"] + (r["l_qseq"] + 1) // 2 in (len(e), len(e) + 1)
            at += 4 + bs
        assert at == len(raw)
        aligns_all.update(aligns)
        for nm, a in zip(names, aligns):
            if BY_NAME[nm].family == "window_sweep":
                sweep.setdefault(nm, set()).add(a)
    assert aligns_all == set(range(16)), "every output alignment mod 16 at a payload block's start"
    assert len(sweep) == sum(1 for c in CAT if c.family == "window_sweep") and all(len(a) >= 2 for a in sweep.values())
    assert set().union(*sweep.values()) == set(range(16))


def _host_seqs(path):
    """-> (number of records that carry a payload, their seq + qual bytes, the unmapped side channel)"""
    seqs, n, unm = [], 0, []
    with host.BamReader(path) as r:
        while True:
            b = r.read_batch(1 << 20, True)
            if b is None:
                break
            unm += r.unmapped()
            carrying = b["l_qseq"] != 5
            n += int(np.sum(carrying))
            for i in np.nonzero((b["seq_off"] != np.uint64(2 ** 64 - 1)) & carrying)[0]:
                lq, so = int(b["l_qseq"][i]), int(b["seq_off"][i])
                seqs.append(bytes(b["seqqual"][so:so + (lq + 1) // 2 + lq]))
    return n, seqs, unm


def test_host_reader_hands_out_the_payload_bytes(carriers):
    """the host reader (zlib underneath) on the carrier files: every record's bases + qualities end with its case's expanded bytes - the reference the GPU module holds the device decoder to"""
    for fname in ("structure", "codes"):
        path, names, _ = carriers[fname]
        n, seqs, unm = _host_seqs(path)
        assert n == len(names) == len(seqs) and len(unm) >= len(names) // 6 and all(u[1] == "ACGTN" for u in unm)
        for nm, s in zip(names, seqs):
            e = D.expected(BY_NAME[nm])
            assert s[len(s) - len(e):] == e and len(s) - len(e) in (0, 1), nm


def test_container_forms_host_reader_against_gzip(tmp_path):
    """28-byte empty BGZF blocks (between data blocks, several in a row, first behind the header) and gzip extra fields with a second subfield before and after BC:
    the host reader hands out what gzip makes of the same bytes"""
    path = str(tmp_path / "forms.bam")
    D.write_container_forms(path)
    raw = gzip.open(path, "rb").read()
    tnames, recs = bamio.read_bam_records(path)
    n, seqs, unm = _host_seqs(path)
    assert n == len([r for r in recs if r["qname"][0] == "c"]) == len(seqs) and n >= 20 and len(unm) >= 3
    data = open(path, "rb").read()
    assert data.count(bamio.BGZF_EOF) >= 12
    xlens, at = set(), 0
    while at < len(data):
        xlens.add(struct.unpack_from("<H", data, at + 10)[0])
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        extra, off, bsize = data[at + 12:at + 12 + xlen], 0, None
        while off < xlen:
            if extra[off:off + 2] == b"BC":
                bsize = struct.unpack_from("<H", extra, off + 4)[0]
            off += 4 + struct.unpack_from("<H", extra, off + 2)[0]
        at += bsize + 1
    assert xlens == {6, 14}
    at = len(D.bam_header_bytes())
    for s in seqs:
        bs, = struct.unpack_from("<i", raw, at)
        if raw[at + 36:at + 37] == b"u":
            at += 4 + bs
            bs, = struct.unpack_from("<i", raw, at)
        assert raw[at + 4 + bs - len(s):at + 4 + bs] == s
        at += 4 + bs
