"""A named catalogue of DEFLATE streams that zlib never writes, for the device BGZF inflate (inflate_core.h, inflate_wave.h, resolve_wave.h): every case is
one BGZF payload of at most 65,536 inflated bytes, written bit by bit by tests/deflate_writer.py.  Seeded and deterministic.  The numbers below are the
kernels' own: the look-up tables' 10 / 8 / 7 bits and the 384-bit segments of pass 1, the 4,096-byte window with 1,536 bytes of history, the 2,496-byte
round, the 256 literals stepped over, the 32 / 79-byte own-lane copies and the 510-literal token field of pass 2.

    catalogue()  -> [Case(name, family, blocks)]      valid streams:  payload(c) inflates to expected(c)
    malformed()  -> [Bad(name, data, isize)]          streams every decoder must refuse
    carrier files: write_carrier(path, cases)         a valid BAM whose long seq+qual fields are catalogue payloads (test_deflate_cases.py, test_bamdec_streams_gpu.py)
"""
import functools
import random
import struct
import zlib
from collections import namedtuple

import bamio
from deflate_writer import (ALT258, Bits, DIST_BASE, DIST_XB, Dynamic, Fixed, Raw, Stored, assign_lengths, auto_lengths, equal_lengths, canonical_codes, deflate, dynamic_auto, expand,
                            kraft_complete, ladder, length_symbol, stream_bits)

# ---- the kernels' constants (seeksv_amd/csrc/inflate_wave.h, resolve_wave.h, inflate_core.h) ----
WV_SEG_BITS, WV_LT, WV_DT, WV_CT = 384, 10, 8, 7
WV_WINDOW_BYTES = 64 * WV_SEG_BITS // 8          # 3,072 bytes of input per window
RW_WIN, RW_KEEP, RW_SKIP, RW_SMALL, WAVE_SMALL = 4096, 1536, 256, 79, 32
RW_ROUND = RW_WIN - RW_KEEP - 64                 # 2,496
TOKEN_RUN = 510

LITERAL_RUNS = (0, 1, 255, 256, 257, 509, 510, 511, 512, 1020, 1021, 2495, 2496, 2497, 4097)
LONG_RUN = 60000
OVERLAP_LENS = (3, 4, 5, 15, 16, 17, 31, 32, 33, 79, 80, 81, 257, 258)
SWEEP_LENS = (3, 16, 17, 79, 80, 258)
SWEEP_DISTS = range(1300, 4301)
FAR_DISTS = range(32507, 32769)
SIZES = (1, 2, 3, 15, 16, 17, 65535, 65536)

Case = namedtuple("Case", "name family blocks")
Bad = namedtuple("Bad", "name data isize")


def token_capacity(n):
    return n // 3 + n // 510 + 4


def _lits(rng, n, lo=0, hi=256):
    return [rng.randrange(lo, hi) for _ in range(n)]


def _mixing(rng, n):
    """tokens for exactly n bytes that cost few input bytes and still differ at every distance: 259 random bytes, then a new byte and 258 bytes copied from 259 back, again and again"""
    if n < 263:
        return _lits(rng, n)
    t, o = _lits(rng, 259), 259
    while n - o >= 259 + 4:
        t += [rng.randrange(256), (258, 259)]
        o += 259
    r = n - o
    if r > 259:
        t += _lits(rng, 4)
        r -= 4
    if r >= 5:
        t += [rng.randrange(256), (r - 1, 259)]
    else:
        t += _lits(rng, r)
    return t


def _phase_block(phase, mod=8):
    """a fixed block (not final) of 10 + 8 k + 9 j bits == phase (mod `mod`): what follows it starts at that bit phase"""
    for j in range(8):
        for k in range(4):
            if (10 + 8 * k + 9 * j) % mod == phase % mod:
                return Fixed([65 + i for i in range(k)] + [200 + i for i in range(j)])
    raise AssertionError(phase)


def _out_len(tokens):
    return sum(1 if type(t) is int else 0 if type(t) is Bits else t[0] for t in tokens)


# ---------------------------------------------------------------- codes ----
def _codes(rng):
    out = []
    for L in range(11, 16):   # literal/length codes above the 10-bit look-up on the MOST FREQUENT literal and length symbol (both L bits), the next ones a bit shorter each
        alphabet = rng.sample(range(256), 12)
        lens = (258, 3, 4, 10, 35, 131)
        order = []
        for i in range(12):
            order.append(alphabet[i])
            if i < 6:
                order.append(length_symbol(lens[i])[0])
        ll = assign_lengths(286, order + [256], kraft_complete(19, L)[::-1])
        t, o = [alphabet[i % 12] for i in range(40)], 40
        for i in range(2200):
            if i % 3 == 2:
                n = lens[0] if rng.random() < 0.5 else rng.choice(lens)
                t.append((n, rng.randrange(1, min(o, 2000) + 1)))
                o += n
            else:
                t.append(alphabet[0] if rng.random() < 0.5 else rng.choice(alphabet))
                o += 1
            if o > 60000:
                break
        out.append(Case(f"ll_code_{L}_bits", "codes", [Dynamic(t, ll, auto_lengths(t)[1], final=True)]))
    for L in range(9, 16):    # distance codes above the 8-bit look-up, the longest on the most frequent distance symbols
        pre = _mixing(rng, 30000)
        order = rng.sample(range(30), 30)
        dd = assign_lengths(30, order, kraft_complete(30, L)[::-1])
        t, o = [], 30000
        for i in range(700):
            x = rng.random()
            s = order[0] if x < 0.3 else order[1] if x < 0.5 else rng.randrange(30)
            d = min(DIST_BASE[s] + rng.randrange(1 << DIST_XB[s]), o)
            n = rng.choice((3, 5, 9, 30))
            t += [rng.randrange(256), (n, d)]
            o += n + 1
        out.append(Case(f"dist_code_{L}_bits", "codes", [Fixed(pre), Dynamic(t, auto_lengths(t)[0], dd, final=True)]))
    # exactly 10 and 11 bits (literal/length) and 8 and 9 bits (distance) side by side, on the frequent symbols
    ll_syms = [300 - 44, 7, 9, 11, 13, 15, 17, 19] + [65, 66, 67, 68, 257, 260]   # 256 (end of block) gets the 1-bit code
    ll = assign_lengths(286, ll_syms, [1, 2, 3, 4, 5, 6, 7, 8, 10, 10, 11, 11, 11, 11])
    d_syms = [20, 21, 22, 23, 24, 25, 0, 1, 2, 3, 4, 5]
    dd = assign_lengths(30, d_syms, [1, 2, 3, 4, 5, 6, 8, 8, 9, 9, 9, 9])
    t = [65, 66, 67, 68] * 3
    for i in range(1500):
        t += [rng.choice((65, 66, 67, 68)), (rng.choice((3, 6)), rng.choice((1, 2, 3, 4, 5, 6, 7, 8)))]
    out.append(Case("ll_10_11_dist_8_9_bits", "codes", [Dynamic(t, ll, dd, final=True)]))
    # a single distance code of one bit; no distance code at all
    t = _lits(rng, 30)
    for i in range(400):
        t += [rng.randrange(256), (rng.randrange(3, 40), 17 + rng.randrange(8))]
    out.append(Case("one_distance_code_of_one_bit", "codes", [dynamic_auto(t, final=True)]))
    out.append(Case("no_distance_code", "codes", [dynamic_auto(_lits(rng, 3000, 30, 90), final=True)]))
    # HLIT 257 and 286, HDIST 1 and 30, smallest HCLEN and 19
    t = _lits(rng, 500, 0, 64)
    out.append(Case("hlit_257_hdist_1_hclen_min", "codes", [dynamic_auto(t, final=True, hlit=257, hdist=1)]))
    t2 = list(t)
    for i in range(300):
        t2 += [rng.randrange(64), (rng.randrange(3, 259), rng.randrange(1, 400))]
    out.append(Case("hlit_286_hdist_30_hclen_19", "codes", [dynamic_auto(t2, final=True, hlit=286, hdist=30, hclen=19)]))
    out.append(Case("hlit_286_hdist_30_runs", "codes", [dynamic_auto(t2, final=True, hlit=286, hdist=30, runs=True)]))
    # code lengths with maximal runs: 138 zeros, 6 repeats; a run of zeros and a run of nines that cross from the literal/length lengths into the distance lengths
    t = [rng.choice((0, 1, 2, 3, 250, 251, 252, 253)) for _ in range(2000)]
    ll = assign_lengths(286, [0, 1, 2, 3, 250, 251, 252, 253, 256], [3, 3, 3, 3, 3, 3, 3, 4, 4])
    dd = assign_lengths(30, [12, 13, 14, 15], [2, 2, 2, 2])
    out.append(Case("runs_138_zeros_crossing_into_distances", "codes", [Dynamic(t, ll, dd, final=True, hlit=286, runs=True)]))
    ll = [8] * 226 + [9] * 60
    dd = [9, 9, 8, 7, 6, 5, 4, 3, 2, 1]
    t = _lits(rng, 300)
    for i in range(350):
        t += [rng.randrange(256), (rng.randrange(3, 259), rng.choice((1, 2, 3, 4, 5, 7, 9, 13, 17, 25)))]
    out.append(Case("runs_6_repeats_crossing_into_distances", "codes", [Dynamic(t, ll, dd, final=True, runs=True)]))
    # a 16 (repeat the length before) directly behind a 17 and behind an 18: it repeats zero
    ll = assign_lengths(286, [0, 1, 2, 3, 250, 251, 252, 253, 256], [3, 3, 3, 3, 3, 3, 3, 4, 4])
    seq = ll[:257] + [0]
    ops, i = [], 0
    while i < len(seq):
        if seq[i]:
            ops.append((seq[i], 0, 0)); i += 1
            continue
        j = i
        while j < len(seq) and seq[j] == 0:
            j += 1
        r = j - i
        if r >= 14:
            ops += [(18, 0, 7), (16, 0, 2)]; r -= 14
        while r >= 6:
            k = min(r - 3, 6)
            ops += [(17, 0, 3), (16, k - 3, 2)]; r -= 3 + k
        ops += [(0, 0, 0)] * r
        i = j
    t = [rng.choice((0, 1, 2, 3, 250, 251, 252, 253)) for _ in range(800)]
    out.append(Case("repeat_code_16_behind_17_and_18", "codes", [Dynamic(t, ll, [0], final=True, cl_ops=ops)]))
    # the longest header there is - 17 + 19 x 3 + 316 x 7 = 2,286 bits - starting at bit 31 of a dword
    cl = assign_lengths(19, list(range(16)) + [16, 17, 18], [7] * 16 + [1, 2, 3])
    ll = [8] * 226 + [9] * 60
    dd = [4, 4] + [5] * 28
    t = _lits(rng, 200)
    for i in range(300):
        t += [rng.randrange(256), (rng.randrange(3, 259), rng.randrange(1, 200))]
    blk = Dynamic(t, ll, dd, final=True, hclen=19, cl_lengths=cl)
    assert blk.header_bits() == 2286
    pre = _phase_block(31, 32)
    assert stream_bits([pre]) % 32 == 31
    out.append(Case("longest_header_at_bit_31", "codes", [pre, blk]))
    return out


def _uniform(rng):
    """codes of one length: a decoder that starts at a wrong bit never falls into step, the chain of pass 1 takes all 64 rounds; each at each of the 8 bit phases"""
    out = []
    ll8 = [8] * 255 + [9, 9]
    for phase in range(8):
        pre = _phase_block(phase)
        out.append(Case(f"uniform_fixed_9_bits_phase_{phase}", "uniform", [pre, Fixed(_lits(rng, 9000, 144, 256), final=True)]))
        out.append(Case(f"uniform_fixed_8_bits_phase_{phase}", "uniform", [pre, Fixed(_lits(rng, 10000, 0, 144), final=True)]))
        out.append(Case(f"uniform_dynamic_8_bits_phase_{phase}", "uniform", [pre, Dynamic(_lits(rng, 10000, 0, 255), ll8, [0], final=True, runs=True)]))
    return out


# ---------------------------------------------------------------- lengths and distances ----
def _lengths_distances(rng):
    out = []
    for kind in ("fixed", "dynamic"):
        t, o = _lits(rng, 300), 300
        for n in list(range(3, 259)) + [258]:
            t += [rng.randrange(256), (n, rng.randrange(1, o + 1))]
            o += n + 1
        t += [rng.randrange(256), (258, 300, ALT258), (258, 1, ALT258), 7]
        out.append(Case(f"every_length_{kind}", "lengths", [Fixed(t, final=True) if kind == "fixed" else dynamic_auto(t, final=True)]))
        pre = _mixing(rng, 32768)
        t = []
        for s in range(30):
            for d in (DIST_BASE[s], DIST_BASE[s] + (1 << DIST_XB[s]) - 1):
                t += [rng.randrange(256), (rng.choice((3, 9, 40)), d)]
        blocks = [Fixed(pre), Fixed(t, final=True)] if kind == "fixed" else [Fixed(pre), dynamic_auto(t, final=True, hdist=30)]
        out.append(Case(f"every_distance_symbol_{kind}", "distances", blocks))
    for d in FAR_DISTS:   # at the first position where it is legal (o == dist), and again at the payload's end
        n1, n2 = SWEEP_LENS[d % 6], SWEEP_LENS[(d // 6) % 6]
        t = _mixing(rng, d) + [(n1, d)] + _lits(rng, 1 + d % 37) + [(n2, d)]
        kind = d % 3
        out.append(Case(f"distance_{d}", "far_distances", [Fixed(t, final=True)] if kind else [dynamic_auto(t, final=True)]))
    # overlapping copies
    for part, dists in enumerate((range(1, 28), range(28, 55), range(55, 81))):
        t = _lits(rng, 100)
        for d in dists:
            for n in OVERLAP_LENS:
                t += _lits(rng, 2) + [(n, d)]
        out.append(Case(f"overlapping_copies_{part}", "overlap", [Fixed(t, final=True) if part != 1 else dynamic_auto(t, final=True)]))
    # chains: every match copies the match before it; sources across several earlier holes of the round with literals between them
    for n in (3, 16, 258):
        out.append(Case(f"chain_{n}_{n}", "chains", [Fixed(_lits(rng, n) + [(n, n)] * 100, final=True)]))
    t = _lits(rng, 40)
    for i in range(700):
        t += [rng.randrange(256), (3, rng.randrange(1, 6)), rng.randrange(256), (rng.randrange(3, 7), rng.randrange(1, 12)), rng.randrange(256), rng.randrange(256),
              (rng.randrange(8, 40), rng.randrange(6, 30))]
    out.append(Case("chain_sources_span_holes", "chains", [dynamic_auto(t, final=True)]))
    # a 65,535-byte payload of back-to-back 3-byte matches: the token count at token_capacity
    t = _lits(rng, 3) + [(3, 3 * (1 + i % 9) if 3 * (1 + i % 9) <= 3 + 3 * i else 3) for i in range(21844)]
    out.append(Case("all_3_byte_matches_65535", "capacity", [Fixed(t, final=True)]))
    # runs of the largest symbols there are (15 + 5 + 15 + 13 bits) across segment and window ends, behind 15-bit literals
    pre = _mixing(rng, 16500)
    big_l, big_d = [281, 282, 283, 284], [28, 29]
    ls = kraft_complete(20, 15)[::-1]      # 15 15 14 13 ... : the four length symbols and two literals take the longest
    ll = assign_lengths(286, big_l + [1, 2, 256] + list(range(100, 113)), ls)
    dd = assign_lengths(30, big_d + list(range(0, 14)), kraft_complete(16, 15)[::-1])
    t, o = [], 16500
    for i in range(1500):
        t.append(rng.choice((1, 2)))
        o += 1
    for i in range(300):
        n = rng.choice((131, 140, 163, 195, 227, 257))
        if o + n > 65000:
            break
        t.append((n, rng.randrange(16385, min(o, 32768) + 1)))
        o += n
    out.append(Case("largest_symbols_48_bits", "largest_symbols", [Fixed(pre), Dynamic(t, ll, dd, final=True)]))
    return out


def _literal_runs(rng):
    """literal runs in front of a match: at the payload's first byte, as a deflate block's first tokens, and in the middle of a block; supplied by literals and by stored blocks"""
    out = []
    for r in LITERAL_RUNS[1:]:   # (a match cannot be a payload's first token)
        m = (rng.choice((3, 20, 258)), rng.randrange(1, r + 1))
        data = bytes(_lits(rng, r))
        out.append(Case(f"run_{r}_literals_at_payload_start", "literal_runs", [Fixed(list(data) + [m, 9], final=True)]))
        out.append(Case(f"run_{r}_stored_at_payload_start", "literal_runs", [Stored(data), Fixed([m, 9], final=True)]))
    for supply in ("literals", "stored"):
        for where in ("block_start", "mid_block"):
            blocks = [Fixed(_lits(rng, 60) + [(5, 7)])]
            o = 65
            cur = []
            for r in LITERAL_RUNS + LITERAL_RUNS[::-1]:
                m = (rng.choice((3, 20, 80, 258)), rng.randrange(1, min(o + r, 5000) + 1))
                data = _lits(rng, r)
                if supply == "stored":
                    if cur:
                        blocks.append(Fixed(cur)); cur = []
                    blocks.append(Stored(bytes(data)))
                    if where == "mid_block":
                        cur = [m, (4, 2)]
                    else:
                        blocks.append(Fixed([m, (4, 2)]))
                else:
                    if where == "block_start":
                        if cur:
                            blocks.append(Fixed(cur)); cur = []
                        blocks.append(Fixed(data + [m, (4, 2)]))
                    else:
                        cur += data + [m, (4, 2)]
                o += r + m[0] + 4
            blocks.append(Fixed(cur + [1], final=True))
            out.append(Case(f"runs_{supply}_{where}", "literal_runs", blocks))
    data = bytes(_lits(rng, LONG_RUN))
    out.append(Case("run_60000_literals_at_payload_start", "literal_runs", [Fixed(list(data) + [(258, 32768), 3], final=True)]))
    out.append(Case("run_60000_literals_mid_block", "literal_runs", [Fixed([1, 2, 3, (9, 2)] + list(data) + [(258, 32767), 3], final=True)]))
    out.append(Case("run_60000_stored_at_payload_start", "literal_runs", [Stored(data), Fixed([(258, 32768), 3], final=True)]))
    out.append(Case("run_60000_stored_mid", "literal_runs", [Fixed([1, 2, 3, (9, 2)]), Stored(data), dynamic_auto([(258, 1), (3, 32768), 3], final=True)]))
    return out


def _window_sweep(rng):
    """match sources relative to the LDS window of pass 2: inside it, wholly in front of it, across its first byte.  Three settings: plain; right behind a literal run
    that resets the window; behind many short rounds that move it"""
    out = []
    for setting in ("plain", "after_literal_run", "after_short_rounds"):
        pairs = [(n, d) for n in SWEEP_LENS for d in SWEEP_DISTS if setting == "plain" or (d + SWEEP_LENS.index(n)) % 3 == 0]
        rng.shuffle(pairs)
        part, i = 0, 0
        while i < len(pairs):
            t, o, k = _lits(rng, 4400), 4400, 0
            while i < len(pairs) and o < (56000 if setting == "after_literal_run" else 64000):
                n, d = pairs[i]
                if setting == "after_literal_run" and k % 4 == 0:
                    r = rng.choice((RW_SKIP + 17, 300, 700, RW_ROUND + 1))
                    t += _lits(rng, r); o += r
                if setting == "after_short_rounds" and k % 6 == 0:
                    for _ in range(70):
                        t += [rng.randrange(256), (3, rng.randrange(1, 60))]
                    o += 280
                t += [rng.randrange(256), (n, d)]
                o += n + 1
                i += 1; k += 1
            out.append(Case(f"window_sweep_{setting}_{part}", "window_sweep", [dynamic_auto(t, final=True) if part % 2 else Fixed(t, final=True)]))
            part += 1
    return out


# ---------------------------------------------------------------- block structure ----
def _structure(rng):
    out = []
    for phase in range(8):   # a stored block behind a Huffman block that ends at each bit phase; dynamic, fixed and stored blocks with no byte alignment between them
        pre = _phase_block(phase)
        t = _lits(rng, 50) + [(10, 20), (258, 50)]
        blocks = [pre, Stored(bytes(_lits(rng, 100 + phase))), dynamic_auto(t), Stored(b""), Fixed([(7, 120 + phase), 5]), dynamic_auto([(30, 300), 1, 2, (3, 1)]),
                  Stored(bytes(_lits(rng, 7))), Fixed([(100, 107)], final=True)]
        out.append(Case(f"stored_at_phase_{phase}", "structure", blocks))
    out.append(Case("empty_stored_blocks", "structure", [Stored(b""), Stored(b"abc"), Stored(b""), Stored(b""), Fixed([(3, 3)]), Stored(b"", final=True)]))
    out.append(Case("empty_fixed_blocks", "structure", [Fixed([]), Fixed([]), Fixed([7, 8, 9]), Fixed([]), Fixed([(3, 2)]), Fixed([], final=True)]))
    out.append(Case("one_symbol_blocks", "structure", [Fixed([i]) for i in range(40)] + [dynamic_auto([200 + i]) for i in range(10)] + [Fixed([(3, 1)]), Stored(b"z"), Fixed([(4, 50)], final=True)]))
    blocks = []
    for i in range(2000):
        blocks.append(Fixed([]) if i % 3 else Stored(b""))
        if i % 400 == 399:
            blocks.append(Fixed(_lits(rng, 5) + [(4, 3)]))
    blocks.append(Fixed([(9, 9)], final=True))
    out.append(Case("2000_empty_blocks", "structure", blocks))
    data = bytes(_lits(rng, 3000))
    out.append(Case("matches_across_block_borders", "structure", [Stored(data), Fixed([(258, 3000), (100, 2)]), dynamic_auto([(200, 3100), 5, (17, 3300)]), Stored(data[:40]),
                                                                   Fixed([(40, 40), (258, 3500)], final=True)]))
    # the stream's last bit on a byte edge / followed by seven pad bits
    for want in (0, 1):
        for k in range(16):
            blocks = [Fixed(_lits(rng, 20, 0, 144) + _lits(rng, k, 144, 256), final=True)]
            if stream_bits(blocks) % 8 == want:
                break
        assert stream_bits(blocks) % 8 == want
        out.append(Case("last_bit_on_byte_edge" if want == 0 else "seven_pad_bits", "structure", blocks))
    for n in SIZES:
        if n < 20:
            blocks = [dynamic_auto(_lits(rng, n), final=True)] if n % 2 else [Fixed(_lits(rng, n), final=True)]
        else:
            t = _mixing(rng, n)
            blocks = [dynamic_auto(t, final=True)] if n % 2 else [Fixed(t, final=True)]
        out.append(Case(f"inflated_size_{n}", "sizes", blocks))
    # the length shapes of the writer's helpers, whole: 1, 2, ..., 14, 15, 15 with the two 15-bit codes on the most frequent literals; 256 codes of 8 bits
    lits = rng.sample(range(256), 15)
    ll = assign_lengths(286, lits[:2] + [256] + lits[2:], ladder()[::-1])
    t = [lits[0] if rng.random() < 0.4 else lits[1] if rng.random() < 0.5 else rng.choice(lits) for _ in range(3000)]
    out.append(Case("ladder_1_to_15_longest_on_frequent", "codes", [Dynamic(t, ll, [0], final=True)]))
    ll = assign_lengths(286, list(range(255)) + [256], equal_lengths(256))
    out.append(Case("equal_lengths_256_codes_of_8_bits", "codes", [_phase_block(5), Dynamic(_lits(rng, 7000, 0, 255), ll, [0], final=True, runs=True)]))
    return out


@functools.lru_cache(maxsize=None)
def catalogue():
    rng = random.Random(20240607)
    cases = _codes(rng) + _uniform(rng) + _lengths_distances(rng) + _literal_runs(rng) + _window_sweep(rng) + _structure(rng)
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


_PAYLOAD, _EXPECT = {}, {}


def payload(case):
    if case.name not in _PAYLOAD:
        _PAYLOAD[case.name] = deflate(case.blocks)
        assert len(_PAYLOAD[case.name]) <= 65536 - 26 - 8, case.name   # (a BGZF block is at most 64 KB, header and trailer included)
    return _PAYLOAD[case.name]


def expected(case):
    if case.name not in _EXPECT:
        _EXPECT[case.name] = expand(case.blocks)
        assert 1 <= len(_EXPECT[case.name]) <= 65536, case.name
    return _EXPECT[case.name]


def tokens_with_positions(case):
    """every token of the case with the output position it starts at and its place in its block: (o, token, index in block, block index)"""
    o = 0
    for bi, b in enumerate(case.blocks):
        for ti, t in enumerate(b.tokens):
            yield o, t, ti, bi, isinstance(b, Stored)
            o += 1 if type(t) is int else 0 if type(t) is Bits else t[0]


def zlib_verdict(data, isize):
    """does zlib take the payload as a whole stream of exactly isize bytes? -> (ok, bytes or None)"""
    try:
        z = zlib.decompressobj(-15)
        got = z.decompress(data)
        return (len(got) == isize and z.eof), got
    except zlib.error:
        return False, None


# ---------------------------------------------------------------- malformed streams ----
@functools.lru_cache(maxsize=None)
def malformed():
    rng = random.Random(77)
    out = []
    fl, fdc = canonical_codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), canonical_codes([5] * 32)

    def add(name, blocks, isize=None):
        out.append(Bad(name, deflate(blocks), isize if isize is not None else max(1, sum(_out_len(b.tokens) for b in blocks))))

    lits = _lits(rng, 40)
    c30 = fdc[30]
    add("fixed_distance_code_30", [Fixed(lits + [Bits(fl[257][0], 7), Bits(c30[0], 5), 1, 2, 3], final=True)], 46)
    add("fixed_length_code_286", [Fixed(lits + [Bits(fl[286][0], 8), Bits(fdc[0][0], 5), 1, 2, 3], final=True)], 46)
    add("distance_1_at_output_0", [Fixed([Bits(fl[257][0], 7), Bits(fdc[0][0], 5), 1, 2, 3], final=True)], 6)
    pre = _mixing(rng, 32767)
    far = Fixed(pre + [Bits(fl[257][0], 7), Bits(fdc[29][0] | (8191 << 5), 18), 1], final=True)   # distance 32,768 at output 32,767
    add("distance_32768_at_output_32767", [far], 32771)
    ok = _lits(rng, 100, 0, 64)
    ll, dd = auto_lengths(ok + [(3, 1)])
    add("hlit_30", [Dynamic(ok, ll, dd, final=True, raw_hlit=30)], 100)
    add("hdist_31", [Dynamic(ok, ll, dd, final=True, raw_hdist=31)], 100)
    over = list(ll); over[200] = 1
    add("oversubscribed_literal_code", [Dynamic(ok, over, dd, final=True)], 100)
    inc = list(ll); inc[max(i for i, l in enumerate(ll) if l and i != 256)] = 0
    add("incomplete_literal_code", [Dynamic([x for x in ok if inc[x]], inc, dd, final=True)], sum(1 for x in ok if inc[x]))
    t = ok + [(3, 1), (3, 2)]
    add("incomplete_two_symbol_distance_code", [Dynamic(t, ll, [2, 2], final=True)], 106)
    add("single_distance_code_of_2_bits", [Dynamic(ok + [(3, 1)], ll, [2], final=True)], 103)
    # the unused pattern of a one-bit distance code: the code is `0`, the stream says `1`
    lcodes = canonical_codes(ll)
    add("unused_pattern_of_one_bit_distance_code", [Dynamic(ok + [Bits(lcodes[257][0], lcodes[257][1]), Bits(1, 1), 1, 2], ll, [1], final=True)], 105)
    # a code-length code of a single symbol: every literal/length length is 8 (256 literals + the end-of-block code do not make a complete code either, but the
    # code-length code is refused first)
    add("single_symbol_code_length_code", [Dynamic(ok, [8] * 257, [8], final=True, cl_lengths=assign_lengths(19, [8], [1]))], 100)
    seq = ll[:257] + dd[:1]
    add("repeat_16_as_first_length", [Dynamic(ok, ll, dd, final=True, hlit=257, hdist=1, cl_ops=[(16, 0, 2)] + [(v, 0, 0) for v in seq[3:]])], 100)
    add("run_past_hlit_plus_hdist", [Dynamic(ok, ll, dd, final=True, hlit=257, hdist=1, cl_ops=[(v, 0, 0) for v in seq[:-2]] + [(18, 0, 7)])], 100)
    no_eob = [0] * 257
    for s in range(64):
        no_eob[s] = 6
    add("no_end_of_block_code", [Dynamic(ok, no_eob, [0], final=True, end=False)], 100)
    add("stored_len_nlen_mismatch", [Stored(bytes(ok), final=True, nlen_field=0x1234)], 100)
    add("stored_len_past_the_payload", [Stored(bytes(ok), final=True, len_field=5000)], 5000)
    good = [Fixed(ok + [(20, 50)], final=True)]
    add("output_one_more_than_isize", good, 119)
    add("output_one_less_than_isize", good, 121)
    add("last_block_not_final", [Fixed(ok + [(20, 50)])], 120)
    add("btype_3", [Fixed(ok), Raw(7, 3)], 100)
    assert len({b.name for b in out}) == len(out)
    return tuple(out)


# ---------------------------------------------------------------- the carrier: a valid BAM around the payloads ----
NAMES, LENS = ["chr1", "chr2", "chrX"], [10_000_000] * 3


def bgzf_raw(payload_bytes, data, extra=None):
    """a BGZF block around an already deflated payload, with the CRC32 and ISIZE of the bytes it inflates to"""
    extra = b"BC\x02\x00" if extra is None else extra   # (the BC subfield's value is filled in below)
    at = extra.index(b"BC\x02\x00") + 4
    total = 12 + len(extra) + 2 + len(payload_bytes) + 8
    assert total <= 65536
    extra = extra[:at] + struct.pack("<H", total - 1) + extra[at:]
    return struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, len(extra)) + extra + payload_bytes + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def bgzf_zlib(data, extra=None):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return bgzf_raw(c.compress(data) + c.flush(), data, extra)


def bam_header_bytes():
    text = ("@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(NAMES, LENS))).encode()
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(NAMES))
    for n, l in zip(NAMES, LENS):
        nb = n.encode() + b"\0"
        hdr += struct.pack("<i", len(nb)) + nb + struct.pack("<i", l)
    return hdr


def carrier_blocks(items, start_offset, first_align=0, between=None, extra=None):
    """items: [(payload, inflated bytes)] - one BAM record each: a small zlib-written block with the record's 36-byte header, its name, its CIGAR and the first
    bytes of its sequence, then the payload as a block of its own whose bytes are the rest of seq + qual.  The name's length puts the payload's block at output
    alignment (first_align + i) mod 16; the sequence bytes in the small block make the field a whole seq + qual.  -> (blocks, [alignment of every payload block])"""
    blocks, aligns, off = [], [], start_offset
    for i, (pl, data) in enumerate(items):
        want = (first_align + i) & 15
        lead = 0 if (len(data) % 3) != 1 else 1                  # seq + qual of l bases takes l + ceil(l / 2) bytes: 0 or 2 mod 3
        total = lead + len(data)
        l_seq = 2 * (total // 3) + (1 if total % 3 == 2 else 0)
        assert l_seq + (l_seq + 1) // 2 == total
        flag = (99, 147, 83, 163)[i % 4]
        # (an unmapped read's bases and qualities leave as text through the side channel: every fourth record is preceded by a small unmapped one of its own)
        extra_rec = bamio.encode_record(dict(qname="u%d" % i, flag=(77, 141, 69)[i % 3], tid=-1 if i % 3 < 2 else i % 3, pos=-1 if i % 3 < 2 else 50 + i, seq="ACGTN", qual=bytes([30, 2, 41, 0, 17]))) if i % 4 == 2 else b""
        cig = [(5, 4), (l_seq - 5, 0)] if l_seq > 5 else [(l_seq, 0)]
        for pad in range(16):
            name = ("c%d" % i) + "n" * pad
            head_len = len(extra_rec) + 4 + 32 + len(name) + 1 + 4 * len(cig) + lead
            if (off + head_len) & 15 == want:
                break
        nb = name.encode() + b"\0"
        body = struct.pack("<iiBBHHHiiii", i % 3, 100 + i, len(nb), 30, 4680, len(cig), flag, l_seq, i % 3, 200 + i, 0) + nb + b"".join(struct.pack("<I", (l << 4) | op) for l, op in cig)
        head = extra_rec + struct.pack("<i", len(body) + total) + body + bytes([0x11] * lead)
        assert len(head) == head_len
        blocks.append(bgzf_zlib(head, extra(2 * i) if extra else None))
        off += head_len
        aligns.append(off & 15)
        blocks.append(bgzf_raw(pl, data, extra(2 * i + 1) if extra else None))
        off += len(data)
        if between:
            blocks += between(i)
    return blocks, aligns


def write_carrier(path, items, first_align=0, between=None, extra=None, after_header=b""):
    hdr = bam_header_bytes()
    blocks, aligns = carrier_blocks(items, len(hdr), first_align, between, extra)
    with open(path, "wb") as f:
        f.write(bgzf_zlib(hdr))
        f.write(after_header)
        for b in blocks:
            f.write(b)
        f.write(bamio.BGZF_EOF)
    return aligns


def carrier_plan():
    """the catalogue in a handful of files: {file name: [case names]}; the window sweep stands in two files, at different alignments"""
    plan = {"codes": [], "uniform": [], "matches": [], "far": [], "runs": [], "sweep_a": [], "sweep_b": [], "structure": []}
    where = {"codes": "codes", "uniform": "uniform", "lengths": "matches", "distances": "matches", "overlap": "matches", "chains": "matches", "capacity": "matches",
             "largest_symbols": "codes", "far_distances": "far", "literal_runs": "runs", "structure": "structure", "sizes": "structure"}
    for c in catalogue():
        if c.family == "window_sweep":
            plan["sweep_a"].append(c.name); plan["sweep_b"].append(c.name)
        else:
            plan[where[c.family]].append(c.name)
    return plan


FIRST_ALIGN = {"codes": 0, "uniform": 3, "matches": 5, "far": 7, "runs": 9, "sweep_a": 1, "sweep_b": 8, "structure": 11}


def write_carriers(directory):
    """-> {file name: (path, [case names], [alignments])}"""
    import os
    by_name = {c.name: c for c in catalogue()}
    out = {}
    for fname, names in carrier_plan().items():
        path = os.path.join(directory, fname + ".bam")
        aligns = write_carrier(path, [(payload(by_name[n]), expected(by_name[n])) for n in names], FIRST_ALIGN[fname])
        out[fname] = (path, names, aligns)
    return out


def write_container_forms(path):
    """the container's rarer forms around catalogue payloads: 28-byte empty BGZF blocks (what `samtools cat` leaves) first behind the header, between data blocks
    (also between a record's two blocks) and several in a row; gzip extra fields with a second subfield before and after BC (XLEN 14)"""
    by_name = {c.name: c for c in catalogue()}
    names = [c.name for c in catalogue() if c.family in ("structure", "sizes") and len(expected(c)) < 5000] + ["every_length_fixed", "chain_16_16"]
    empty = bamio.BGZF_EOF
    extras = (None, b"XY\x04\x00abcd" + b"BC\x02\x00", b"BC\x02\x00" + b"ZZ\x04\x00\x00\xff\x1f\x8b")

    def between(i):
        return [empty] * (0, 1, 3, 0, 2)[i % 5]

    def extra(j):
        return extras[j % 3]

    items = [(payload(by_name[n]), expected(by_name[n])) for n in names]
    hdr = bam_header_bytes()
    blocks, _ = carrier_blocks(items, len(hdr), 4, between, extra)
    out = []
    for j, b in enumerate(blocks):   # an empty block between a record's small block and its payload block, now and then
        out.append(b)
        if j % 7 == 0 and b != empty:
            out.append(empty)
    with open(path, "wb") as f:
        f.write(bgzf_zlib(hdr) + empty + empty)
        for b in out:
            f.write(b)
        f.write(empty)
    return names
