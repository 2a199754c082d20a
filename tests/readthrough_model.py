"""`getsv -F` in plain Python: FindJunction (process_bwasw.cpp:5-227) restated record by record from the reference's behaviour, the insert-or-count
rule that folds its pairs into the junction map (:198-216), and a generator of split-alignment files with far more variety per record than bwasw
writes.  Slow and obvious on purpose - loops over records, a dict of held records walked in file order - and it shares no code with the HIP kernels
(seeksv_amd/csrc/readthrough_kernels.h) or with seeksv_amd/device.py: tests/test_readthrough_differential_gpu.py holds ssv_rt_* against it pair for
pair, tests/test_readthrough_model.py holds it against what the real reference printed.

Where the reference leaves the behaviour undefined the model states the LIBRARY's documented rule (include/seeksv_hip.h, the comments in
readthrough_kernels.h); each such place is marked `library rule` below and reference_undefined() names the records it concerns, so that the
reference-anchored checks can leave them out."""
import numpy as np

OPS = "MIDNSHP=X"
NT16 = "=ACMGRSVTWYHKDBN"
NO_SEQ = (1 << 64) - 1
F_REVERSE, F_UNMAP, F_DUP = 16, 4, 1024
M, I, D, N, S, H, P, EQ, X = range(9)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the record loop
# ---------------------------------------------------------------------------------------------------------------------------------------------
def record_ops(b, i):
    """record i's CIGAR as [(length, code)]"""
    o, n = int(b["cigar_off"][i]), int(b["n_cigar"][i])
    return [(int(x) >> 4, int(x) & 15) for x in b["cigar"][o:o + n]]


def record_bases(b, i):
    """record i's bases in ASCII (bam_nt16_rev_table; GetSeq upper-cases them, the table is upper case already)"""
    lq = max(int(b["l_qseq"][i]), 0)
    so = int(b["seq_off"][i])
    if lq == 0:
        return ""
    out = []
    for byte in bytes(b["seqqual"][so:so + (lq + 1) // 2]):    # two bases a byte, the earlier one in the high nibble
        out.append(NT16[byte >> 4])
        out.append(NT16[byte & 15])
    return "".join(out[:lq])


def reference_undefined(b, i, n_targets, name):
    """why the reference's behaviour for record i is undefined (None: it is defined).  Only records that reach the place in question count."""
    ops = record_ops(b, i)
    if not ops:
        return "no CIGAR (the reference reads cigar[-1])"
    if len(name.encode()) > 254:
        return "name longer than BAM allows"
    lq = int(b["l_qseq"][i])
    tid = int(b["tid"][i])
    unmapped = bool(int(b["flag"][i]) & F_UNMAP)
    if (tid < 0 or tid >= n_targets) and not unmapped:
        return "tid outside the header (target_name[tid])"
    clip = ops[0][0] if ops[0][1] == S else ops[-1][0]
    if clip > lq:
        return "clip longer than the read (GetSeq reads past the bases)"
    return None


def selected(b, i, min_mapq, n_targets):
    """process_bwasw.cpp:47-51: __g_skip_aln (MAPQ), unmapped, the shape of the CIGAR's two ends, duplicate"""
    ops = record_ops(b, i)
    if not ops:
        return False                                    # library rule: a record without CIGAR is skipped
    flag = int(b["flag"][i])
    if int(b["mapq"][i]) < min_mapq:
        return False
    if flag & F_UNMAP:
        return False
    op1, op2 = ops[0][1], ops[-1][1]
    if op1 == H or op2 == H or (op1 == S and op2 == S) or (op1 == M and op2 == M) or (flag & F_DUP):
        return False
    tid = int(b["tid"][i])
    if tid < 0 or tid >= n_targets:
        return False                                    # library rule: a tid outside the header is dropped
    return True


def generate_cigar(ops):
    """GenerateCigar (clip_reads.cpp:309-329): the operations without S and H, and the reference length l over M, D, = and N (not X, not P)"""
    vec, l = [], 0
    for length, op in ops:
        if op == H or op == S:
            continue
        if op in (M, D, EQ, N):
            l += length
        vec.append((length, op))
    return vec, l


def alignment_of(b, i, name, rec_index):
    """process_bwasw.cpp:53-82: one kept record as the reference's Alignment"""
    ops = record_ops(b, i)
    vec, ref_len = generate_cigar(ops)
    lq = max(int(b["l_qseq"][i]), 0)
    if ops[0][1] == S:
        side = "5"
        left = min(ops[0][0], lq)                       # library rule: clip lengths are clamped to l_qseq
        right = lq - left
        pos = int(b["pos"][i]) + 1
    else:                                               # every other record goes through the 3' branch, whatever its last operation is
        side = "3"
        right = min(ops[-1][0], lq)                     # library rule: clamped
        left = lq - right
        pos = int(b["pos"][i]) + ref_len
    bases = record_bases(b, i)
    return dict(tid=int(b["tid"][i]), pos=pos, left_seq=bases[:left], right_seq=bases[left:left + right], cigar=vec, side=side,
                strand="-" if int(b["flag"][i]) & F_REVERSE else "+", rec=rec_index, name=name)


def reverse_complement(seq):
    """GetReverseComplementSeq (clip_reads.cpp:414-466): reversed; A C G T swapped, every other letter stays"""
    comp = {"A": "T", "T": "A", "C": "G", "G": "C"}
    out = []
    for ch in reversed(seq):
        out.append(comp.get(ch, ch))
    return "".join(out)


def junction_of(held, new, contigs):
    """process_bwasw.cpp:90-197 for a held Alignment and the one that completes the pair -> the pair dict, or None when the two do not pair"""
    same_strand = held["strand"] == new["strand"]
    same_side = held["side"] == new["side"]
    if not ((same_strand and not same_side) or (not same_strand and same_side)):
        return None
    clipped = [0, 0, 0, 0]      # up left / right, down left / right clipped lengths of the two SeqInfo values
    edits = [0, 0]              # 1: MinusCigarRight(up CIGAR, microhomology), 2: AddCigarLeft(down CIGAR, microhomology)
    mh = 0
    if same_strand:
        if held["side"] == "5":
            up, down = new, held
        else:
            up, down = held, new
        up_seq, down_seq = down["left_seq"], down["right_seq"]
        if len(up["left_seq"]) >= len(down["left_seq"]):
            kind = 0
            mh = len(up["left_seq"]) - len(down["left_seq"])
            key = (up["tid"], up["pos"] - mh, "+", down["tid"], down["pos"], "+")
            edits[0] = 1
        else:
            kind = 1
            key = (up["tid"], up["pos"], "+", down["tid"], down["pos"], "+")
            clipped[1] = len(down["left_seq"]) - len(up["left_seq"])
    else:
        # make_pair(chr, pos) < make_pair(chr, pos): contig NAMES compared as strings (bytes), then positions; not less -> the new record is up
        if (contigs[held["tid"]].encode(), held["pos"]) < (contigs[new["tid"]].encode(), new["pos"]):
            up, down = held, new
        else:
            up, down = new, held
        if new["side"] == "5":
            if len(up["right_seq"]) >= len(down["left_seq"]):
                kind = 2
                mh = len(up["right_seq"]) - len(down["left_seq"])
                key = (up["tid"], up["pos"], "-", down["tid"], down["pos"] + mh, "+")
                up_seq, down_seq = reverse_complement(up["right_seq"]), reverse_complement(up["left_seq"])
                edits[1] = 2
            else:
                kind = 3
                key = (up["tid"], up["pos"], "-", down["tid"], down["pos"], "+")
                up_seq, down_seq = down["left_seq"], down["right_seq"]
                clipped[1] = len(down["left_seq"]) - len(up["right_seq"])
        else:
            if len(up["left_seq"]) >= len(down["right_seq"]):
                kind = 4
                mh = len(up["left_seq"]) - len(down["right_seq"])
                key = (up["tid"], up["pos"] - mh, "+", down["tid"], down["pos"], "-")
                up_seq, down_seq = reverse_complement(down["right_seq"]), reverse_complement(down["left_seq"])
                edits[0] = 1
            else:
                kind = 5
                key = (up["tid"], up["pos"], "+", down["tid"], down["pos"], "-")
                up_seq, down_seq = up["left_seq"], up["right_seq"]
                clipped[2] = len(down["right_seq"]) - len(up["left_seq"])
    key = (contigs[key[0]], key[1], key[2], contigs[key[3]], key[4], key[5])
    pack = lambda vec: [(length << 4) | op for length, op in vec]  # noqa: E731
    return dict(key=key, microhomology=mh, kind=kind, up_seq=up_seq, down_seq=down_seq, clipped=tuple(clipped),
                up_cigar=pack(up["cigar"]), down_cigar=pack(down["cigar"]), edits=tuple(edits), records=(held["rec"], new["rec"]))


def find_junction(batches, names, min_mapq, contigs):
    """FindJunction over batches in file order.  batches: dicts of arrays (tid, pos, flag, mapq, n_cigar, cigar, cigar_off, l_qseq, seq_off,
    seqqual); names[k]: the read names of batch k; contigs: the header's names.  -> (pairs, n_candidates): one dict per pair with the keys
    Context.readthrough returns, in the order of the completing record; the number of kept records."""
    held = {}                   # the reference's std::map<string, Alignment> read_id2align
    pairs, n_candidates, rec_index = [], 0, 0
    for b, nm in zip(batches, names):
        for i in range(len(b["tid"])):
            this = rec_index
            rec_index += 1
            if not selected(b, i, min_mapq, len(contigs)):
                continue
            n_candidates += 1
            name = nm[i].encode()[:255]                 # library rule: a name is read up to 255 bytes
            a = alignment_of(b, i, name, this)
            if name not in held:
                held[name] = a
                continue
            p = junction_of(held[name], a, contigs)
            if p is None:
                continue                                # the new record is dropped, the held one stays
            pairs.append(p)
            del held[name]
    return pairs, n_candidates


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the fold into the junction map
# ---------------------------------------------------------------------------------------------------------------------------------------------
def minus_cigar_right(vec, length):
    """MinusCigarRight (clip_reads.cpp:507-546) on [(length, op letter)]: the M / I bases shortened by `length` from the right; what follows the
    operation that ends the kept part goes"""
    total = sum(l for l, op in vec if op in "MI")
    if total <= length:
        return list(vec)
    keep = total - length
    out = []
    for l, op in vec:
        if op in "MI":
            if l >= keep:
                out.append((keep, op))
                return out
            keep -= l
        out.append((l, op))
    return out


def add_cigar_left(vec, length):
    """AddCigarLeft (clip_reads.cpp:548-558)"""
    if vec and vec[0][1] == "M":
        return [(vec[0][0] + length, "M")] + list(vec[1:])
    return [(length, "M")] + list(vec)


def cigar_text(vec, left_clipped=0, right_clipped=0):
    """DisplayCigarVector (clip_reads.h:489-505)"""
    return (f"{left_clipped}S" if left_clipped > 0 else "") + "".join(f"{l}{op}" for l, op in vec) + (f"{right_clipped}S" if right_clipped > 0 else "")


def parse_cigar_text(text):
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num), ch))
            num = ""
    return out


def seq_infos(p):
    """the two SeqInfo values of a pair (process_bwasw.cpp:109-197) as dicts: seq, cigar [(length, letter)], left / right clipped, support"""
    unpack = lambda ops: [(x >> 4, OPS[x & 15]) for x in ops]  # noqa: E731
    uc, dc = unpack(p["up_cigar"]), unpack(p["down_cigar"])
    if p["edits"][0] == 1:
        uc = minus_cigar_right(uc, p["microhomology"])
    if p["edits"][1] == 2:
        dc = add_cigar_left(dc, p["microhomology"])
    up = dict(seq=p["up_seq"], cigar=uc, left_clipped=p["clipped"][0], right_clipped=p["clipped"][1], support=0)
    down = dict(seq=p["down_seq"], cigar=dc, left_clipped=p["clipped"][2], right_clipped=p["clipped"][3], support=1)
    return up, down


def seed_rows(text):
    """-B rows (ReadBreakpoint, getsv.cpp:1292-1323) as the map they leave: key -> entry; a key that comes twice keeps its first row (find()
    returns the first entry of a multimap's range)"""
    jmap = {}
    for line in text.splitlines():
        f = line.split("\t")
        if not f or f[0].startswith("@"):
            continue
        key = (f[0], int(f[1]), f[2], f[4], int(f[5]), f[6])
        if key in jmap:
            continue
        jmap[key] = dict(up=dict(seq=f[21], cigar=parse_cigar_text(f[19]), left_clipped=0, right_clipped=0, support=int(f[3])),
                         down=dict(seq=f[22], cigar=parse_cigar_text(f[20]), left_clipped=0, right_clipped=0, support=int(f[7])),
                         microhomology=int(f[8]), seeded=True)
    return jmap


def apply(pairs, jmap=None):
    """process_bwasw.cpp:198-216: every pair in order - no entry under its junction: insert (up, down, microhomology); an entry whose up or
    down seq length differs from the pair's: its down support + 1.  -> the map (dict in insertion order)"""
    jmap = {} if jmap is None else jmap
    for p in pairs:
        up, down = seq_infos(p)
        e = jmap.get(p["key"])
        if e is None:
            jmap[p["key"]] = dict(up=up, down=down, microhomology=p["microhomology"], seeded=False)
        elif len(e["up"]["seq"]) != len(up["seq"]) or len(e["down"]["seq"]) != len(down["seq"]):
            e["down"]["support"] += 1
    return jmap


def row_columns(key, e):
    """the columns of a .sv / stdout row that the -F pass decides"""
    return dict(key=key, microhomology=e["microhomology"], left_cigar=cigar_text(e["up"]["cigar"], e["up"]["left_clipped"], e["up"]["right_clipped"]),
                right_cigar=cigar_text(e["down"]["cigar"], e["down"]["left_clipped"], e["down"]["right_clipped"]), left_seq=e["up"]["seq"],
                right_seq=e["down"]["seq"], left_support=e["up"]["support"], right_support=e["down"]["support"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------------------------------
NAME_ALPHABET = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_:/.-#"
MAPQS = [60, 60, 60, 60, 254, 255, 255, 20, 20, 19, 1, 0]
_OP_POOL = [M, M, M, M, I, D, N, P, EQ, X]
_NT16_BYTES = np.frombuffer(NT16.encode(), np.uint8)
_PLAIN_CODES, _PLAIN_P = np.array([1, 2, 4, 8, 15]), np.r_[np.full(4, 0.96 / 4), [0.04]]
_IUPAC_CODES, _IUPAC_P = np.array([1, 2, 4, 8, 0, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]), np.r_[np.full(4, 0.8 / 4), np.full(12, 0.2 / 12)]
N_OPS_TARGETS = [1, 2, 2, 2, 3, 3, 4, 5, 5, 6, 6, 9, 20, 64, 65, 130]


def _length(rng, least=1, long_reads=True):
    """a part of a read: mostly tens of bases, sometimes one or two, sometimes many hundreds"""
    r = rng.rand()
    if r < 0.08:
        return int(rng.randint(least, least + 3))
    if r < 0.9 or not long_reads:
        return int(rng.randint(max(least, 10), 160))
    return int(rng.randint(200, 750))


def _body(rng, q, n_ops, first_not=(), last_not=()):
    """n_ops operations (about) out of M I D N P = X that consume exactly q query bases; the first / last operation not among first_not /
    last_not.  S and H are put around it by the caller."""
    query, other = [M, I, EQ, X], [D, N, P]
    n_ops = max(1, n_ops)
    kinds, n_query = [], 0
    draws, di = rng.randint(0, 1 << 30, 4 * n_ops + 16).tolist(), 0   # (one call for the whole body: a draw per operation is slow)
    for k in range(n_ops):
        pool = _OP_POOL if n_query < q else other       # (no query base left for another M / I / = / X)
        while True:
            if di == len(draws):
                draws, di = rng.randint(0, 1 << 30, 64).tolist(), 0
            op = pool[draws[di] % len(pool)]
            di += 1
            if (k == 0 and op in first_not) or (k == n_ops - 1 and op in last_not) or (kinds and op == kinds[-1]):
                continue
            break
        kinds.append(op)
        n_query += op in query
    qi = [k for k, op in enumerate(kinds) if op in query]
    if q > 0 and not qi:                                # the query bases need a place: one more operation in front of the last
        op = M if (len(kinds) > 1 or M not in first_not) else I
        kinds.insert(max(0, len(kinds) - 1), op)
        if kinds[0] in first_not:
            kinds[0] = I
        qi = [k for k, op in enumerate(kinds) if op in query]
    lens = [0] * len(kinds)
    other_lens = rng.randint(1, 12, len(kinds)).tolist()
    for k, op in enumerate(kinds):
        if op in other:
            lens[k] = other_lens[k]
    if qi:
        cut = np.sort(rng.choice(np.arange(1, q), len(qi) - 1, replace=False)) if len(qi) > 1 else np.zeros(0, int)
        parts = np.diff(np.concatenate(([0], cut, [q])))
        for k, l in zip(qi, parts):
            lens[k] = int(l)
    return [(l, op) for l, op in zip(lens, kinds)]


def _make_record(rng, side, left, right, strand, tid, cand_pos, n_ops, clip_op=S):
    """one record whose Alignment is (side, |left_seq|, |right_seq|, strand, tid, pos == cand_pos).  clip_op: the operation that makes the 3'
    branch's right part (S, or any of M I D N P = X: records without S go through that branch too)."""
    lq = left + right
    if side == "5":
        body = _body(rng, right, n_ops - 1, last_not=(S, H))
        ops = [(left, S)] + body
    else:
        if clip_op in (D, N, P):                        # the last operation consumes no base: the ones in front of it consume the whole read
            body = _body(rng, lq, n_ops - 1, first_not=(S, H))
        else:
            first_not = (S, H, M) if clip_op == M else (S, H)
            body = _body(rng, left, n_ops - 1, first_not=first_not) if (left > 0 or n_ops > 1) else []
            if body and body[-1][1] == clip_op and clip_op != S:
                body[-1] = (body[-1][0], I if clip_op != I else EQ)
                if body[0][1] == M and clip_op == M:
                    body[0] = (body[0][0], EQ)
        ops = body + [(right, clip_op)]
    _, ref_len = generate_cigar(ops)
    pos0 = cand_pos - 1 if side == "5" else cand_pos - ref_len
    return dict(tid=tid, pos=pos0, flag=F_REVERSE if strand == "-" else 0, mapq=60, ops=ops, lq=lq, seq=None)


def _pair_records(rng, kind, mh_class, contigs_by_rank, lens, n_ops_of, single=True, long_reads=True):
    """two records (held, completing) that make construction case `kind` with the given class of its comparison: 'eq' (the >= boundary),
    'one', 'large'.  Kinds 1, 3, 5 are the < branches: 'eq' is not possible there, 'one' / 'large' say by how much the comparison fails."""
    nt = len(lens)
    x = _length(rng, 2, long_reads)
    delta = {"eq": 0, "one": 1, "large": int(rng.randint(2, 260))}[mh_class]
    if kind in (1, 3, 5):
        delta = -min(delta if delta else 1, x - 1)
    y = x + delta                                        # up's length in the comparison, x: down's
    free = lambda: (0 if rng.rand() < 0.03 else _length(rng, 1, long_reads))  # noqa: E731  (the part of a read that is not the clip)
    clip = lambda: _length(rng, 1, long_reads)                 # noqa: E731
    where = lambda t: int(rng.randint(6000, lens[t] - 6000))   # noqa: E731
    clip_op = S if rng.rand() < 0.8 else int(rng.choice([M, I, D, N, P, EQ, X]))
    if kind in (0, 1):
        strand = "+-"[int(rng.randint(0, 2))]
        tu, td = int(rng.randint(0, nt)), int(rng.randint(0, nt))
        if rng.rand() < 0.5:
            td = tu
        up = _make_record(rng, "3", y, clip(), strand, tu, where(tu), n_ops_of(), clip_op)
        down = _make_record(rng, "5", x, free(), strand, td, where(td), n_ops_of(), S)
        return (up, down) if rng.rand() < 0.5 else (down, up)
    su = "+-"[int(rng.randint(0, 2))]
    sd = "-" if su == "+" else "+"
    r = rng.rand()
    if r < 0.3:                                          # one contig, equal positions: the tie - the completing record is up
        tu = td = int(rng.randint(0, nt))
        pu = pd = where(tu)
        tie = True
    elif r < 0.6:                                        # one contig
        tu = td = int(rng.randint(0, nt))
        pu, pd = sorted([where(tu), where(tu)])
        tie = pu == pd
    else:                                                # two contigs: up is the one whose NAME is smaller
        a, b = sorted(rng.choice(nt, 2, replace=False).tolist())
        tu, td = contigs_by_rank[a], contigs_by_rank[b]
        pu, pd = where(tu), where(td)
        tie = False
    if kind in (2, 3):
        up = _make_record(rng, "5", clip(), y, su, tu, pu, n_ops_of(), S)
        down = _make_record(rng, "5", x, free(), sd, td, pd, n_ops_of(), S)
    else:
        up = _make_record(rng, "3", y, clip(), su, tu, pu, n_ops_of(), clip_op)
        clip2 = S if rng.rand() < 0.8 else int(rng.choice([M, I, D, N, P, EQ, X]))
        if single and rng.rand() < 0.1:                  # a CIGAR of one operation: the whole read is the right part
            down = _make_record(rng, "3", 0, x, sd, td, pd, 1, int(rng.choice([I, EQ, X])))
        else:
            down = _make_record(rng, "3", free(), x, sd, td, pd, n_ops_of(), clip2)
    if tie or rng.rand() < 0.5:
        return down, up                                  # (held, completing): with a tie the completing record is up
    return up, down


def _junk_record(rng, nt, lens, safe):
    """a record every min_mapq drops: unmapped, duplicate, H at an end, S..S, M..M, clips only - and, not safe: no CIGAR, a tid outside the header"""
    lq = _length(rng, 2)
    tid = int(rng.randint(0, nt))
    what = int(rng.randint(0, 8 if safe else 12))
    flag = F_REVERSE if rng.rand() < 0.5 else 0
    a = int(rng.randint(1, lq))
    ops = [(a, S), (lq - a, M)]
    no_seq = rng.rand() < 0.5
    if what == 0:
        flag |= F_UNMAP
        if rng.rand() < 0.5:
            tid = -1
    elif what == 1:
        flag |= F_DUP
    elif what == 2:
        ops = [(int(rng.randint(1, 50)), H), (lq - a, M), (a, S)]
    elif what == 3:
        ops = [(a, S), (lq - a, M), (int(rng.randint(1, 50)), H)]
    elif what == 4:
        b = int(rng.randint(1, lq - a + 1)) if lq - a > 1 else 1
        ops = [(a, S), (max(lq - a - b, 0), M), (b, S)] if lq - a - b > 0 else [(a, S), (lq - a, S)]
    elif what == 5:
        ops = [(a, M), (int(rng.randint(1, 9)), D), (lq - a, M)]
    elif what == 6:
        ops = [(lq, S)]
    elif what == 7:
        ops = [(lq, M)]
    elif what == 8:
        ops = []                                         # no CIGAR at all
    elif what == 9:
        tid = nt                                         # tid == n_targets
    elif what == 10:
        tid = nt + int(rng.randint(1, 1000))
    else:
        tid = -1                                         # mapped by its flag, yet without a contig
    return dict(tid=tid, pos=int(rng.randint(0, lens[max(0, min(tid, nt - 1))] - 3000)), flag=flag, mapq=int(rng.choice(MAPQS)), ops=ops, lq=lq, seq=None,
                no_seq=bool(no_seq))


def random_contigs(rng):
    """2 to 40 contigs whose byte-wise name order is not their tid order"""
    nt = int(rng.choice([2, 3, 3, 5, 8, 17, 40]))
    while True:
        names = []
        while len(names) < nt:
            n = "".join(rng.choice(list("chrXYM0123456789_Zab"), int(rng.randint(1, 9))))
            if n not in names:
                names.append(n)
        if [n.encode() for n in names] != sorted(n.encode() for n in names):
            break
    return names, [int(x) for x in rng.randint(20000, 60000, nt)]


def random_rt_sample(seed, safe=False, n_records=3000, contigs=None, big_name=300, long_cigars=False, long_reads=True):
    """A -F file as one batch + read names, no BAM needed: dict(contigs, lens, batch, qnames, cuts).  safe: only inputs for which the reference's
    behaviour is defined (every record has a CIGAR, clips fit the read, tids inside the header, names of at most 254 bytes).  contigs:
    (names, lens) to use instead of random ones.  big_name: records of the one name that comes hundreds of times.  long_cigars: every record
    has more than five operations once S is dropped.  long_reads: parts of many hundred bases among the others."""
    rng = np.random.RandomState(7000 + seed)
    names, lens = random_contigs(rng) if contigs is None else (list(contigs[0]), [int(x) for x in contigs[1]])
    nt = len(names)
    by_rank = sorted(range(nt), key=lambda t: names[t].encode())
    n_ops_of = (lambda: int(rng.choice([7, 8, 12, 30, 66, 67, 131]))) if long_cigars else (lambda: int(rng.choice(N_OPS_TARGETS)))
    groups, used = [], set()

    def new_name(form=None):
        form = rng.rand() if form is None else form
        while True:
            if form < 0.04:
                n = str(rng.choice(list(NAME_ALPHABET)))                              # one byte
            elif form < 0.10:
                n = "".join(rng.choice(list(NAME_ALPHABET), 254))                     # the longest a BAM holds
            elif form < 0.2:
                n = f"r{seed}." + "".join(rng.choice(list(NAME_ALPHABET), int(rng.randint(1, 80))))
            else:
                n = f"read{int(rng.randint(0, 10 ** 7))}"
            if n not in used:
                used.add(n)
                return n
            form = 0.1 + 0.9 * rng.rand()                # (the one-byte names run out)

    def sibling(n):
        """a name that differs from n in its last byte only, or has n as a prefix"""
        for _ in range(50):
            m = n[:-1] + str(rng.choice(list(NAME_ALPHABET))) if (rng.rand() < 0.5 or len(n) >= 254) else n + str(rng.choice(list(NAME_ALPHABET)))
            if m not in used:
                used.add(m)
                return m
        return new_name(0.5)

    def pair(kind=None, mh_class=None):
        kind = int(rng.randint(0, 6)) if kind is None else kind
        mh_class = str(rng.choice(["eq", "one", "large", "large"])) if mh_class is None else mh_class
        return list(_pair_records(rng, kind, mh_class, by_rank, lens, n_ops_of, single=not long_cigars, long_reads=long_reads))

    def blocker(held):
        """a record the held one does not pair with: same strand and side (or opposite strand, other side) - it is dropped"""
        strand = "-" if held["flag"] & F_REVERSE else "+"
        side = "5" if held["ops"][0][1] == S else "3"
        if rng.rand() < 0.5:
            strand, side = ("-" if strand == "+" else "+"), ("3" if side == "5" else "5")
        t = int(rng.randint(0, nt))
        return _make_record(rng, side, _length(rng, 1, long_reads), _length(rng, 1, long_reads), strand, t, int(rng.randint(6000, lens[t] - 6000)), n_ops_of(), S)

    total, last_name, geometries = 0, None, []
    while total < n_records - big_name:
        r = rng.rand()
        name = sibling(last_name) if (last_name and rng.rand() < 0.15) else new_name()
        last_name = name
        if r < 0.50:
            recs = pair()
            if geometries and rng.rand() < 0.12:         # the geometry of an earlier pair again: the same junction from another read
                recs = [dict(x, seq=None) for x in geometries[int(rng.randint(0, len(geometries)))]]
                if rng.rand() < 0.5 and recs[0]["ops"][-1][1] in (M, EQ, X, I) and len(recs[0]["ops"]) > 1:
                    l, op = recs[0]["ops"][-1]           # ... with other seq lengths
                    recs[0] = dict(recs[0], ops=recs[0]["ops"][:-1] + [(l + 3, op)], lq=recs[0]["lq"] + 3)
            else:
                geometries.append(recs)
        elif r < 0.58:
            recs = pair()
            recs = [recs[0], blocker(recs[0]), recs[1]]  # hold, drop, pair
        elif r < 0.66:
            recs = pair() + pair()                       # four records, two pairs: the name is held anew
        elif r < 0.74:
            first = pair()[0]
            recs = [first] + [blocker(first) for _ in range(int(rng.randint(0, 3)))]   # a held name that never pairs
        elif r < 0.80:
            recs = []                                    # 5 to 12 records of any shape
            for _ in range(int(rng.randint(5, 13))):
                recs.append(pair()[int(rng.randint(0, 2))])
        else:
            recs = pair()
            recs.insert(int(rng.randint(0, 3)), _junk_record(rng, nt, lens, safe))
        for x in recs:
            x["qname"] = name
        groups.append(recs)
        total += len(recs)
    if big_name:
        name = new_name(0.5)
        recs = [pair()[int(rng.randint(0, 2))] for _ in range(big_name)]
        for x in recs:
            x["qname"] = name
        groups.append(recs)
    # per record: MAPQ, the flags no rule looks at, bases
    for g in groups:
        for x in g:
            if "no_seq" not in x:
                x["mapq"] = int(rng.choice(MAPQS))
                x["no_seq"] = False
                if rng.rand() < 0.04:
                    x["flag"] |= int(rng.choice([F_UNMAP, F_DUP]))
                    x["no_seq"] = rng.rand() < 0.5
            for bit in (256, 2048, 1, 64):
                if rng.rand() < 0.08:
                    x["flag"] |= bit
            if not safe and rng.rand() < 0.02 and x["ops"]:
                # the read shorter than its CIGAR says: a first S longer than the read, l_qseq 0 or 1 (the clamps)
                x["lq"] = int(rng.choice([0, 0, 1, max(0, x["ops"][0][0] - 1)]))
                if x["lq"] == 0:
                    x["no_seq"] = rng.rand() < 0.5
            iupac = rng.rand() < 0.15                    # all sixteen base codes, or A C G T with a few N
            x["codes"] = (rng.choice(_IUPAC_CODES, x["lq"], p=_IUPAC_P) if iupac else rng.choice(_PLAIN_CODES, x["lq"], p=_PLAIN_P)).astype(np.uint8)
            x["seq"] = _NT16_BYTES[x["codes"]].tobytes().decode()
    # file order: the records of a name keep their order; half of the names lie close together, the others anywhere in the file
    keyed = []
    for g in groups:
        keys = np.sort(rng.rand(len(g))) if rng.rand() < 0.5 else np.sort(np.clip(rng.rand() + rng.rand(len(g)) * 0.01, 0, 1))
        keyed += list(zip(keys.tolist(), g))
    order = sorted(range(len(keyed)), key=lambda k: (keyed[k][0], k))
    recs = [keyed[k][1] for k in order]
    n = len(recs)
    cig, coff, soff, blob, nbytes = [], [], [], [], 0
    for x in recs:
        coff.append(len(cig))
        cig += [(l << 4) | op for l, op in x["ops"]]
        if x["no_seq"]:
            soff.append(NO_SEQ)
            continue
        soff.append(nbytes)
        c = np.concatenate((x["codes"], np.zeros(x["lq"] & 1, np.uint8)))
        packed = (c[0::2] << 4) | c[1::2]               # the even base in the high nibble
        blob += [packed, np.full(x["lq"], 30, np.uint8)]
        nbytes += len(packed) + x["lq"]
    span = max([1] + [generate_cigar(x["ops"])[1] for x in recs])
    batch = dict(tid=np.array([x["tid"] for x in recs], np.int32), pos=np.array([x["pos"] for x in recs], np.int32),
                 flag=np.array([x["flag"] for x in recs], np.uint16), mapq=np.array([x["mapq"] for x in recs], np.uint8),
                 n_cigar=np.array([len(x["ops"]) for x in recs], np.uint16), l_qseq=np.array([x["lq"] for x in recs], np.int32),
                 mtid=np.full(n, -1, np.int32), mpos=np.full(n, -1, np.int32), isize=np.zeros(n, np.int32), xc=np.zeros(n, np.uint8),
                 cigar=np.array(cig, np.uint32), cigar_off=np.array(coff, np.uint32), seq_off=np.array(soff, np.uint64),
                 seqqual=np.concatenate(blob + [np.zeros(16, np.uint8)]), max_ref_span=int(span), no_tid_runs=True)
    cuts = sorted(set(int(c) for c in rng.randint(1, n, 3)))
    return dict(contigs=names, lens=lens, batch=batch, qnames=[x["qname"] for x in recs], cuts=cuts, records=recs)


def cut_batch(b, a, e):
    """records [a, e) of a batch: the per-record columns sliced, the CIGAR and base pools whole"""
    n = len(b["tid"])
    return {k: (v[a:e] if isinstance(v, np.ndarray) and k not in ("cigar", "seqqual") and len(v) == n else v) for k, v in b.items()}


def split(sample, cuts):
    """-> (batches, names) cut at the record indices `cuts` (an empty piece stays: a batch with n == 0)"""
    bounds = [0] + list(cuts) + [len(sample["qnames"])]
    return ([cut_batch(sample["batch"], bounds[k], bounds[k + 1]) for k in range(len(bounds) - 1)],
            [sample["qnames"][bounds[k]:bounds[k + 1]] for k in range(len(bounds) - 1)])


def sample_records(sample):
    """the sample as the record dicts tests/bamio.py writes"""
    out = []
    for x in sample["records"]:
        out.append(dict(qname=x["qname"], flag=x["flag"], tid=x["tid"], pos=x["pos"], mapq=x["mapq"], cigar=list(x["ops"]), mtid=-1, mpos=-1, isize=0,
                        seq=x["seq"], qual=None))
    return out


def batch_from_records(recs):
    """record dicts as tests/bamio.py writes them (qname, flag, tid, pos, mapq, cigar as text or [(length, code)], seq) -> (batch, names)"""
    cig, coff, soff, blob, nbytes = [], [], [], [], 0
    for r in recs:
        ops = r["cigar"]
        if isinstance(ops, str):
            ops = [(l, OPS.index(ch)) for l, ch in parse_cigar_text(ops)]
        coff.append(len(cig))
        cig += [(l << 4) | op for l, op in ops]
        soff.append(nbytes)
        packed = [0] * ((len(r["seq"]) + 1) // 2)
        for k, ch in enumerate(r["seq"]):
            packed[k // 2] |= NT16.index(ch) << (4 if k % 2 == 0 else 0)
        blob += packed + [255] * len(r["seq"])
        nbytes += len(packed) + len(r["seq"])
    n = len(recs)
    batch = dict(tid=np.array([r["tid"] for r in recs], np.int32), pos=np.array([r["pos"] for r in recs], np.int32),
                 flag=np.array([r["flag"] for r in recs], np.uint16), mapq=np.array([r["mapq"] for r in recs], np.uint8),
                 n_cigar=np.diff(np.array(coff + [len(cig)])).astype(np.uint16), l_qseq=np.array([len(r["seq"]) for r in recs], np.int32),
                 mtid=np.full(n, -1, np.int32), mpos=np.full(n, -1, np.int32), isize=np.zeros(n, np.int32), xc=np.zeros(n, np.uint8),
                 cigar=np.array(cig, np.uint32), cigar_off=np.array(coff, np.uint32), seq_off=np.array(soff, np.uint64),
                 seqqual=np.array(blob + [0] * 16, np.uint8), max_ref_span=1, no_tid_runs=True)
    return batch, [r["qname"] for r in recs]


# the wider anchor (tests/golden/readthrough/model_anchor.json, written by tests/golden/make_readthrough_reference.py from the real reference):
# safe samples of some hundred records each (the recorded rows carry every pair's bases: their number keeps the file small), under min_mapq (-w) 0 / 1 / 20
ANCHOR_SEEDS = (0, 1, 2)
ANCHOR_RUNS = (("w0", 0), ("w1", 1), ("w20", 20))


def anchor_sample(seed):
    """(the first one with reads of many hundred bases, the others without: the recorded rows carry every pair's bases)"""
    return random_rt_sample(540 + seed, safe=True, n_records=120, big_name=20, long_reads=seed == 0)
