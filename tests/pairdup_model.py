"""The duplicate-marking rule of `seeksv run -D` (include/seeksv_hip.h, ssv_pairdup_mark) in plain Python over a list of records in input order.

THE RULE.  The records of all batches are one sequence in input order: batch order first, then record order.  A record's index in it is g.
  takes part  flag & 0x1 set, none of 0x4 | 0x8 | 0x100 | 0x800 | 0x400 set, tid >= 0, mtid >= 0 and n_cigar > 0 (a record that arrives with 0x400 keeps it and
              takes no part); every other record is never touched
  end u       64-bit signed, may be negative.  Forward (!(flag & 0x10)): pos minus the lengths of the leading run of S / H operations.  Reverse: pos + reference
              span (M D N = X) - 1 + the lengths of the trailing run of S / H operations
  name hash   64-bit FNV-1a (offset 1469598103934665603, prime 1099511628211) over the read name's bytes without the NUL; digest_bits=k keeps the low k bits
              (SSV_DUP_DIGEST_BITS in the library's environment)
  mates       the records that take part and have equal name hash form a name group.  A name group is a PAIR iff it has exactly two records, exactly one of them
              has 0x40, each record's (mtid, mpos) equals the other's (tid, pos), and each record's 0x20 agrees with the other's 0x10.  The records of every
              other name group are left untouched and counted as `unpaired`
  key         a = the record with the smaller (tid, u, reverse), on a tie the one with 0x40; b = the other.  key = (tid_a, u_a, rev_a, tid_b, u_b, rev_b),
              compared exactly
  score       the sum over both records of the quality bytes >= 15 (32 bits); a record with l_qseq == 0 or first quality byte 0xff adds 0
  keeper      the group's (pairs of equal key) highest score; among equal scores the pair whose smaller g is smallest.  Both records of every other pair of the
              group get flag |= 0x400
When no two pairs of a group have equal scores, the set of marked records does not depend on the input order.
Limits: libraries are not told apart; which mate is first of pair is not part of the key; single reads and pairs with an unmapped end are never marked; a name
that occurs on more than two primary records is left alone.

A record is a dict as tests/bamio.py's encode_record takes it (qname, flag, tid, pos, cigar as text, mtid, mpos, seq, qual).  Nothing here looks at how the
input is cut into batches or at its order beyond g.  The hand-made answers of tests/pairdup_inputs.py hold this model, and the model holds the kernels."""
import re

from markdup_model import F_DUP, F_MREV, F_MUNMAP, F_PAIRED, F_READ1, F_REV, F_SECONDARY, F_SUPP, F_UNMAP, fnv1a, quals

CIGAR_RE = re.compile(r"(\d+)([MIDNSHP=X])")


def cigar_ops(r):
    c = r.get("cigar") or ""
    return [(int(n), op) for n, op in CIGAR_RE.findall(c)] if c != "*" else []


def takes_part(r):
    f = r["flag"]
    return (bool(f & F_PAIRED) and not f & (F_UNMAP | F_MUNMAP | F_SECONDARY | F_SUPP | F_DUP) and r["tid"] >= 0 and r.get("mtid", -1) >= 0
            and len(cigar_ops(r)) > 0)


def end_u(r):
    """the unclipped 5' end"""
    ops = cigar_ops(r)
    if not r["flag"] & F_REV:
        lead = 0
        for n, op in ops:
            if op not in "SH":
                break
            lead += n
        return r["pos"] - lead
    trail = 0
    for n, op in reversed(ops):
        if op not in "SH":
            break
        trail += n
    span = sum(n for n, op in ops if op in "MDN=X")
    return r["pos"] + span - 1 + trail


def name_hash(r, bits=64):
    return fnv1a(r["qname"].encode()) & ((1 << bits) - 1)


def read_score(r):
    q = quals(r)
    if len(q) == 0 or q[0] == 0xff:
        return 0
    return sum(x for x in q if x >= 15)


def row(r, bits=64):
    """the record's row as ssv_pairdup_retain writes it: (name_hash, u, score, kind); all zero for a record that takes no part"""
    if not takes_part(r):
        return (0, 0, 0, 0)
    return (name_hash(r, bits), end_u(r), read_score(r) & 0xffffffff, 1)


def is_pair(x, y):
    return (bool(x["flag"] & F_READ1) != bool(y["flag"] & F_READ1)
            and (x["mtid"], x["mpos"]) == (y["tid"], y["pos"]) and (y["mtid"], y["mpos"]) == (x["tid"], x["pos"])
            and bool(x["flag"] & F_MREV) == bool(y["flag"] & F_REV) and bool(y["flag"] & F_MREV) == bool(x["flag"] & F_REV))


def pair_key(x, y):
    def half(r):
        return (r["tid"], end_u(r), 1 if r["flag"] & F_REV else 0)
    hx, hy = half(x), half(y)
    if hx != hy:
        a, b = (hx, hy) if hx < hy else (hy, hx)
    else:
        a, b = hx, hy       # (a tie: a is the one with 0x40 - the key is the same either way)
    return a + b


def pairs(records, digest_bits=64):
    """-> ([(g1, g2)] with g1 < g2: the pairs, [g]: the records that take part and belong to no pair)"""
    groups = {}
    for g, r in enumerate(records):
        if takes_part(r):
            groups.setdefault(name_hash(r, digest_bits), []).append(g)
    found, unpaired = [], []
    for members in groups.values():
        if len(members) == 2 and is_pair(records[members[0]], records[members[1]]):
            found.append((members[0], members[1]))
        else:
            unpaired += members
    return sorted(found), sorted(unpaired)


def mark(records, digest_bits=64, stats=None):
    """-> the flags of all records after marking.  stats (a dict, optional) gets the counts of ssv_pairdup_stats."""
    flags = [r["flag"] for r in records]
    found, unpaired = pairs(records, digest_bits)
    groups = {}
    for g1, g2 in found:
        groups.setdefault(pair_key(records[g1], records[g2]), []).append((g1, g2))
    marked = 0
    for members in groups.values():
        keeper = max(members, key=lambda p: ((read_score(records[p[0]]) + read_score(records[p[1]])) & 0xffffffff, -p[0]))
        for p in members:
            if p != keeper:
                flags[p[0]] |= F_DUP
                flags[p[1]] |= F_DUP
                marked += 1
    if stats is not None:
        stats.update(records=len(records), taking_part=sum(takes_part(r) for r in records), unpaired=len(unpaired), pairs=len(found),
                     groups_many=sum(len(m) >= 2 for m in groups.values()), pairs_marked=marked)
    return flags


def score_ties(records, digest_bits=64):
    """does some group hold two pairs of equal score (then, and only then, the marked set may depend on the input order)"""
    found, _ = pairs(records, digest_bits)
    seen = set()
    for g1, g2 in found:
        k = (pair_key(records[g1], records[g2]), (read_score(records[g1]) + read_score(records[g2])) & 0xffffffff)
        if k in seen:
            return True
        seen.add(k)
    return False
