"""A bit-exact DEFLATE (RFC 1951) WRITER for tests.  Not a compressor: it emits the blocks, codes and tokens it is told to, so that the inflate
kernels can be shown streams no compressor on this machine writes (tests/deflate_cases.py).  The inflated bytes are defined by expanding the tokens;
nothing searches for matches.  Test tooling only.

    tokens   an int 0..255 is a literal; (len, dist) a match; (258, dist, ALT258) codes 258 as symbol 284 with extra bits 31;
             Bits(value, n) puts n raw bits into the symbol stream (malformed streams; no output)
    blocks   Stored(data), Fixed(tokens), Dynamic(tokens, ll_lengths, d_lengths, ...); every block carries its own `final` bit
    deflate(blocks) -> the stream's bytes;  expand(blocks) -> the bytes it inflates to
"""
from collections import namedtuple

ALT258 = "alt258"
Bits = namedtuple("Bits", "value n")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_XB = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_XB = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)

_LEN_SYM = [0] * 259
for _s in range(28):
    for _l in range(LEN_BASE[_s], LEN_BASE[_s] + (1 << LEN_XB[_s])):
        if _l <= 258:
            _LEN_SYM[_l] = _s
_LEN_SYM[258] = 28
_DIST_SYM = [0] * 32769
for _s in range(30):
    for _d in range(DIST_BASE[_s], DIST_BASE[_s] + (1 << DIST_XB[_s])):
        _DIST_SYM[_d] = _s


def length_symbol(length, alt=False):
    """-> (literal/length symbol, extra value, extra bits)"""
    if length == 258 and alt:
        return 284, 31, 5
    s = _LEN_SYM[length]
    return 257 + s, length - LEN_BASE[s], LEN_XB[s]


def distance_symbol(dist):
    s = _DIST_SYM[dist]
    return s, dist - DIST_BASE[s], DIST_XB[s]


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32   # (30 and 31 have codes and no meaning)


def canonical_codes(lengths):
    """code lengths -> {symbol: (the code's bits reversed for an LSB-first writer, length)}; nothing is checked: over-subscribed and incomplete sets are written as they are"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            c = nxt[l] & ((1 << l) - 1)   # (an over-subscribed set runs out of codes: keep the low bits)
            nxt[l] += 1
            out[s] = (int(format(c, "0%db" % l)[::-1], 2), l)
    return out


def kraft_sum(lengths):
    """sum of 2^-l in units of 2^-15 (32768 = complete)"""
    return sum(1 << (15 - l) for l in lengths if l)


def kraft_complete(n, maxlen):
    """n code lengths of a complete code whose longest code has exactly maxlen bits (n > maxlen), ascending: split the deepest leaf until maxlen is reached, then the shallowest"""
    assert maxlen < n <= (1 << maxlen)
    leaves = [0]
    while len(leaves) < n:
        leaves.sort()
        if leaves[-1] < maxlen:
            l = leaves.pop()
        else:
            l = leaves.pop(0)
            assert l < maxlen
        leaves += [l + 1, l + 1]
    return sorted(leaves)


def ladder():
    """1, 2, ..., 14, 15, 15: a complete code of 16 symbols with every length"""
    return list(range(1, 16)) + [15]


def equal_lengths(n):
    """n codes of one length (n a power of two): complete"""
    assert n & (n - 1) == 0 and 2 <= n <= 256
    return [n.bit_length() - 1] * n


def assign_lengths(n_symbols, symbols, lengths):
    """a length table of n_symbols entries: symbols[i] gets lengths[i], everything else 0"""
    out = [0] * n_symbols
    for s, l in zip(symbols, lengths):
        out[s] = l
    return out


class BitWriter:
    """LSB-first; a small integer accumulator flushed to a bytearray eight bytes at a time"""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def bits(self):
        return 8 * len(self.buf) + self.n

    def align(self):
        self.put(0, -self.bits() & 7)

    def raw(self, data):
        assert self.bits() & 7 == 0
        k = self.n >> 3
        self.buf += self.acc.to_bytes(k, "little") if k else b""
        self.acc, self.n = 0, 0
        self.buf += data

    def done(self):
        self.align()
        k = self.n >> 3
        return bytes(self.buf + (self.acc.to_bytes(k, "little") if k else b""))


class Stored:
    def __init__(self, data, final=False, len_field=None, nlen_field=None):
        self.data, self.final, self.len_field, self.nlen_field = bytes(data), final, len_field, nlen_field
        self.tokens = list(self.data)

    def write(self, w):
        w.put(int(self.final), 1)
        w.put(0, 2)
        w.align()
        n = len(self.data) if self.len_field is None else self.len_field
        w.put(n, 16)
        w.put((n ^ 0xffff) if self.nlen_field is None else self.nlen_field, 16)
        w.raw(self.data)


class Raw:
    """n bits as they are, where a block would start (malformed streams)"""

    def __init__(self, value, n):
        self.value, self.n, self.tokens, self.final = value, n, [], True

    def write(self, w):
        w.put(self.value, self.n)


def _put_tokens(w, tokens, ll, dd, end=True):
    put = w.put
    for t in tokens:
        if type(t) is int:
            c, l = ll[t]
            put(c, l)
        elif type(t) is Bits:
            put(t.value, t.n)
        else:
            s, xv, xb = length_symbol(t[0], len(t) > 2 and t[2] == ALT258)
            c, l = ll[s]
            put(c | (xv << l), l + xb)
            s, xv, xb = distance_symbol(t[1])
            c, l = dd[s]
            put(c | (xv << l), l + xb)
    if end:
        c, l = ll[256]
        put(c, l)


class Fixed:
    def __init__(self, tokens, final=False, end=True):
        self.tokens, self.final, self.end = list(tokens), final, end

    def write(self, w):
        w.put(int(self.final), 1)
        w.put(1, 2)
        _put_tokens(w, self.tokens, _FIXED_LL_CODES, _FIXED_D_CODES, self.end)


_FIXED_LL_CODES = canonical_codes(FIXED_LL)
_FIXED_D_CODES = canonical_codes(FIXED_D)


def run_length_ops(seq, runs):
    """the code-length alphabet's symbols for the length sequence seq: [(symbol, extra value, extra bits)]; runs: False = one by one, True = the
    longest runs (18: up to 138 zeros, 17: 3..10 zeros, 16: 3..6 repeats of the length before) - over the whole sequence, so a run crosses from the
    literal/length lengths into the distance lengths wherever the values allow it"""
    if not runs:
        return [(v, 0, 0) for v in seq]
    ops, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        j = i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                ops.append((18, k - 11, 7))
                run -= k
            if run >= 3:
                ops.append((17, run - 3, 3))
                run = 0
            ops += [(0, 0, 0)] * run
        else:
            ops.append((v, 0, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                ops.append((16, k - 3, 2))
                run -= k
            ops += [(v, 0, 0)] * run
        i = j
    return ops


class Dynamic:
    """ll_lengths: up to 286 literal/length code lengths, d_lengths: up to 30 distance code lengths (shorter lists are padded with zeros up to hlit / hdist).
    hlit / hdist: how many are written (default: up to the last one in use, at least 257 / 1); hclen: "min" or 19 (or a number);
    runs: write the lengths with the 16/17/18 run codes; cl_ops: the code-length symbols given outright [(sym, extra value, extra bits)];
    cl_lengths: the code-length code's own 19 lengths (default: a complete code over the symbols in use); raw_hlit / raw_hdist: the 5-bit fields as they are."""

    def __init__(self, tokens, ll_lengths, d_lengths, final=False, hlit=None, hdist=None, hclen="min", runs=False, cl_ops=None, cl_lengths=None, end=True, raw_hlit=None, raw_hdist=None):
        self.tokens, self.final, self.end = list(tokens), final, end
        ll, dd = list(ll_lengths), list(d_lengths)
        if hlit is None:
            hlit = max(257, max([i + 1 for i, l in enumerate(ll) if l] or [0]))
        if hdist is None:
            hdist = max(1, max([i + 1 for i, l in enumerate(dd) if l] or [0]))
        self.hlit, self.hdist = hlit, hdist
        self.ll = (ll + [0] * hlit)[:hlit]
        self.dd = (dd + [0] * hdist)[:hdist]
        self.ops = list(cl_ops) if cl_ops is not None else run_length_ops(self.ll + self.dd, runs)
        if cl_lengths is None:
            used = sorted({o[0] for o in self.ops})
            if len(used) == 1:   # (a code of one symbol is incomplete: zlib refuses it for the code-length code)
                used.append(0 if used[0] else 1)
            k = len(used).bit_length() - 1
            short = (1 << (k + 1)) - len(used)
            cl_lengths = assign_lengths(19, used, [k] * short + [k + 1] * (len(used) - short))
        self.cl = list(cl_lengths)
        self.hclen = hclen
        self.raw_hlit, self.raw_hdist = raw_hlit, raw_hdist

    def header_bits(self):
        w = BitWriter()
        self._header(w)
        return w.bits()

    def n_cl(self):
        n_cl = max([i + 1 for i, s in enumerate(CL_ORDER) if self.cl[s]] + [4])
        if self.hclen != "min":
            assert self.hclen >= n_cl
            n_cl = self.hclen
        return n_cl

    def _header(self, w):
        n_cl = self.n_cl()
        w.put(int(self.final), 1)
        w.put(2, 2)
        w.put(self.hlit - 257 if self.raw_hlit is None else self.raw_hlit, 5)
        w.put(self.hdist - 1 if self.raw_hdist is None else self.raw_hdist, 5)
        w.put(n_cl - 4, 4)
        for s in CL_ORDER[:n_cl]:
            w.put(self.cl[s], 3)
        codes = canonical_codes(self.cl)
        for s, xv, xb in self.ops:
            c, l = codes[s]
            w.put(c | (xv << l), l + xb)

    def write(self, w):
        self._header(w)
        _put_tokens(w, self.tokens, canonical_codes(self.ll), canonical_codes(self.dd), self.end)


def deflate(blocks, start_bits=None):
    """-> the stream; start_bits, when given, receives every block's first bit position"""
    w = BitWriter()
    for b in blocks:
        if start_bits is not None:
            start_bits.append(w.bits())
        b.write(w)
    return w.done()


def stream_bits(blocks):
    """bits of the stream before the padding of its last byte"""
    w = BitWriter()
    for b in blocks:
        b.write(w)
    return w.bits()


def expand(blocks):
    out = bytearray()
    for b in blocks:
        if isinstance(b, Stored):
            out += b.data
            continue
        for t in b.tokens:
            if type(t) is int:
                out.append(t)
            elif type(t) is Bits:
                continue
            else:
                n, d = t[0], t[1]
                assert 3 <= n <= 258 and 1 <= d <= len(out), (n, d, len(out))
                if d >= n:
                    at = len(out) - d
                    out += out[at:at + n]
                else:
                    unit = bytes(out[-d:])
                    out += (unit * (n // d + 1))[:n]
    return bytes(out)


def auto_lengths(tokens, ll_max=None, d_max=None, long_on_frequent=False):
    """code lengths for the symbols the tokens use (+ the end-of-block code): balanced by default; with ll_max / d_max a complete code whose longest code
    has that many bits (symbols that never occur are added when there are too few); long_on_frequent: the MOST frequent symbols get the longest codes"""
    fl, fd = {256: 1}, {}
    for t in tokens:
        if type(t) is int:
            fl[t] = fl.get(t, 0) + 1
        elif type(t) is not Bits:
            s = length_symbol(t[0], len(t) > 2 and t[2] == ALT258)[0]
            fl[s] = fl.get(s, 0) + 1
            s = distance_symbol(t[1])[0]
            fd[s] = fd.get(s, 0) + 1

    def shape(freq, n_all, maxlen, single_ok):
        syms = sorted(freq, key=lambda s: (-freq[s], s))
        if not syms:
            return [0] * n_all
        if len(syms) == 1 and maxlen is None and single_ok:
            return assign_lengths(n_all, syms, [1])
        want = max(len(syms), 2, (maxlen or 0) + 1)
        for s in range(n_all):
            if len(syms) >= want:
                break
            if s not in freq:
                syms.append(s)
        if maxlen is None:
            k = len(syms).bit_length() - 1
            short = (1 << (k + 1)) - len(syms)
            ls = [k] * short + [k + 1] * (len(syms) - short)
        else:
            ls = kraft_complete(len(syms), maxlen)
        if long_on_frequent:
            ls = ls[::-1]
        return assign_lengths(n_all, syms, ls)

    return shape(fl, 286, ll_max, False), shape(fd, 30, d_max, True)


def dynamic_auto(tokens, final=False, ll_max=None, d_max=None, long_on_frequent=False, **kw):
    ll, dd = auto_lengths(tokens, ll_max, d_max, long_on_frequent)
    return Dynamic(tokens, ll, dd, final=final, **kw)
