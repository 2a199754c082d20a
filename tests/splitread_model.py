"""`seeksv run -A` in plain Python: the split-read rule over an aligner's own output, record by record.  The rule as include/seeksv_hip.h states it at
ssv_rt_begin_original:

A record takes part when all of these hold:
  - it has a CIGAR;
  - tid is a contig of the header;
  - mapq >= min_mapq;
  - none of 0x4, 0x100, 0x400 is set, as the input has them;
  - exactly one of its two ends is clipped.  An end is clipped when its outermost operation is S or H.
S..S, H..S, H..H and records with no clipped end are not taken, 10I90M and 100= included (FindJunction sends those last two through its 3' branch).

Lengths come from the CIGAR alone:
  - R is the sum of M I S = X H;
  - the clip length of the clipped end is the sum of the run of S / H operations at that end (5H10S85M: 15);
  - a 5' clipped record (first operation a clip): side '5', left = clip, right = R - left, pos = pos0 + 1;
  - otherwise: side '3', right = clip, left = R - right, pos = pos0 + ref_len, with GenerateCigar's ref_len (M D = N, not X).

A record carries the read when it has no H, its bases are present (seq_off != SSV_NO_SEQ) and l_qseq == R.

The key is (read name, flag & 0xC0) in the place of the read name alone: mates never meet; single-end reads have 0 there.

Hold / pair / drop runs in input order per key.  A held A and a new B pair when all of these hold, looked at in this order:
  - same strand and different sides, or opposite strands and the same side;
  - R_A == R_B (else B counts as dropped_length);
  - at least one of the two carries the read (else B counts as dropped_no_carrier).
Otherwise B is dropped and A stays held.

Junction, microhomology, kind, clipped lengths, CIGAR sources and edits are FindJunction's case analysis unchanged (readthrough_model.junction_of).  The
two seqs are the slices (source record, begin, len, rc) that case analysis names; when the source carries the read they are read from it, when it does not
the same bases are read from its partner: (begin, len, rc) on the same strand, (R - begin - len, len, !rc) on opposite strands.  Complementing swaps
A C G T only.

Slow and obvious on purpose; it shares nothing with seeksv_amd/device.py or the kernels (seeksv_amd/csrc/splitread_kernels.h).  The geometry is
readthrough_model.junction_of, which tests/test_readthrough_model.py holds to the real reference: it is called here with left_seq / right_seq of the
right LENGTHS (placeholders where a record does not carry the read), and the seqs are cut afterwards by the slice rule above."""
import readthrough_model as RM

M, I, D, N, S, H, P, EQ, X = range(9)
F_UNMAP, F_REVERSE, F_MATE, F_SECONDARY, F_DUP, F_SUPPLEMENTARY = 4, 16, 0xC0, 0x100, 0x400, 0x800
COUNTS = ("candidates", "hard_clipped", "pairs", "pairs_borrowed", "dropped_no_carrier", "dropped_length")


def clipped(op):
    return op == S or op == H


def takes_part(b, i, min_mapq, n_targets):
    ops = RM.record_ops(b, i)
    if not ops:
        return False
    tid = int(b["tid"][i])
    if tid < 0 or tid >= n_targets:
        return False
    if int(b["mapq"][i]) < min_mapq:
        return False
    if int(b["flag"][i]) & (F_UNMAP | F_SECONDARY | F_DUP):
        return False
    return clipped(ops[0][1]) != clipped(ops[-1][1])


def lengths(ops):
    """(R, side, left, right, ref_len) of a record that takes part"""
    R = sum(l for l, op in ops if op in (M, I, S, EQ, X, H))
    ref_len = sum(l for l, op in ops if op in (M, D, EQ, N))
    if clipped(ops[0][1]):
        clip = 0
        for l, op in ops:
            if not clipped(op):
                break
            clip += l
        return R, "5", clip, R - clip, ref_len
    clip = 0
    for l, op in reversed(ops):
        if not clipped(op):
            break
        clip += l
    return R, "3", R - clip, clip, ref_len


def carries_read(b, i, ops, R):
    if any(op == H for _, op in ops):
        return False
    if int(b["seq_off"][i]) == RM.NO_SEQ:
        return False
    return int(b["l_qseq"][i]) == R


def candidate_of(b, i, name, rec_index):
    ops = RM.record_ops(b, i)
    R, side, left, right, ref_len = lengths(ops)
    flag = int(b["flag"][i])
    carries = carries_read(b, i, ops, R)
    return dict(tid=int(b["tid"][i]), pos=int(b["pos"][i]) + (1 if side == "5" else ref_len), side=side, left=left, right=right, R=R,
                strand="-" if flag & F_REVERSE else "+", cigar=[(l, op) for l, op in ops if not clipped(op)], carries=carries,
                hard=any(op == H for _, op in ops), bases=RM.record_bases(b, i) if carries else None, rec=rec_index, key=(name, flag & F_MATE))


def _slices(held, new, kind, up, down):
    """the two seqs of construction case `kind` as (source, begin, len, rc): readthrough_model.junction_of's up_seq / down_seq, by position"""
    if kind in (0, 1, 3):
        return (down, 0, down["left"], False), (down, down["left"], down["right"], False)
    if kind == 2:
        return (up, up["left"], up["right"], True), (up, 0, up["left"], True)
    if kind == 4:
        return (down, down["left"], down["right"], True), (down, 0, down["left"], True)
    return (up, 0, up["left"], False), (up, up["left"], up["right"], False)


def _read_slice(sl, other_of):
    """-> (the bases, borrowed?)"""
    src, begin, length, rc = sl
    borrowed = not src["carries"]
    if borrowed:
        other = other_of(src)
        if other["strand"] != src["strand"]:
            begin, rc = src["R"] - begin - length, not rc
        src = other
    seq = src["bases"][begin:begin + length]
    return (RM.reverse_complement(seq) if rc else seq), borrowed


def pair_of(held, new, contigs):
    """a held candidate and the one that completes the pair -> (row, borrowed?), a row as Context.readthrough_original gives it"""
    as_alignment = lambda c: dict(tid=c["tid"], pos=c["pos"], left_seq="?" * c["left"], right_seq="?" * c["right"], cigar=c["cigar"], side=c["side"],  # noqa: E731
                                  strand=c["strand"], rec=c["rec"], name=c["key"][0])
    p = RM.junction_of(as_alignment(held), as_alignment(new), contigs)
    # which of the two is up: junction_of's CIGAR sources are (up, down)
    same_strand = held["strand"] == new["strand"]
    if same_strand:
        up, down = (new, held) if held["side"] == "5" else (held, new)
    elif (contigs[held["tid"]].encode(), held["pos"]) < (contigs[new["tid"]].encode(), new["pos"]):
        up, down = held, new
    else:
        up, down = new, held
    other_of = lambda c: new if c is held else held  # noqa: E731
    s_up, s_down = _slices(held, new, p["kind"], up, down)
    (p["up_seq"], b1), (p["down_seq"], b2) = _read_slice(s_up, other_of), _read_slice(s_down, other_of)
    assert len(p["up_seq"]) == s_up[2] and len(p["down_seq"]) == s_down[2]
    return p, b1 or b2


def find_pairs(batches, names, min_mapq, contigs):
    """the rule over batches in input order (dicts of arrays as readthrough_model.find_junction takes them; names[k]: the read names of batch k)
    -> (rows in the order of the completing record, counts: a dict of COUNTS)"""
    held, rows, rec_index = {}, [], 0
    counts = dict.fromkeys(COUNTS, 0)
    for b, nm in zip(batches, names):
        for i in range(len(b["tid"])):
            this = rec_index
            rec_index += 1
            if not takes_part(b, i, min_mapq, len(contigs)):
                continue
            c = candidate_of(b, i, nm[i].encode()[:255], this)
            counts["candidates"] += 1
            counts["hard_clipped"] += c["hard"]
            a = held.get(c["key"])
            if a is None:
                held[c["key"]] = c
                continue
            same_strand, same_side = a["strand"] == c["strand"], a["side"] == c["side"]
            if not ((same_strand and not same_side) or (not same_strand and same_side)):
                continue
            if a["R"] != c["R"]:
                counts["dropped_length"] += 1
                continue
            if not (a["carries"] or c["carries"]):
                counts["dropped_no_carrier"] += 1
                continue
            row, borrowed = pair_of(a, c, contigs)
            rows.append(row)
            counts["pairs"] += 1
            counts["pairs_borrowed"] += borrowed
            del held[c["key"]]
    return rows, counts


def find_pairs_by_name_only(batches, names, min_mapq, contigs):
    """the same with the read name alone as the key (what `getsv -F` would pair): only for tests that show the mate bits matter"""
    blind = [dict(b, flag=(b["flag"].astype(int) & (0xFFFF ^ F_MATE)).astype(b["flag"].dtype)) for b in batches]
    return find_pairs(blind, names, min_mapq, contigs)
