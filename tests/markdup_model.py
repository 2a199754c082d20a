"""The duplicate-marking rule of `seeksv run -M` (include/seeksv_hip.h, ssv_dup_retain) in plain Python over a list of records in file order.

A record is a dict as tests/bamio.py's encode_record takes it: qname, flag, tid, pos, mtid, mpos, seq, qual (None: 0xff bytes; bytes: phred values).  Nothing
here looks at how a stream is cut into batches: the rule is a function of the file.  The hand-made answers of tests/markdup_inputs.py hold this model, and the
model holds the kernels."""
import struct

FNV_OFFSET, FNV_PRIME, M64 = 1469598103934665603, 1099511628211, (1 << 64) - 1
F_PAIRED, F_UNMAP, F_MUNMAP, F_REV, F_MREV, F_READ1, F_SECONDARY, F_DUP, F_SUPP = 0x1, 0x4, 0x8, 0x10, 0x20, 0x40, 0x100, 0x400, 0x800


def fnv1a(data, h=FNV_OFFSET):
    for b in data:
        h = ((h ^ b) * FNV_PRIME) & M64
    return h


def quals(r):
    """the record's quality bytes as BAM stores them"""
    q = r.get("qual")
    if q is None:
        return b"\xff" * len(r.get("seq", ""))
    return bytes(ord(c) - 33 for c in q) if isinstance(q, str) else bytes(q)


def takes_part(r):
    f = r["flag"]
    return bool(f & F_PAIRED) and not f & (F_UNMAP | F_MUNMAP | F_SECONDARY | F_SUPP | F_DUP) and r["tid"] >= 0 and r.get("mtid", -1) >= 0


def is_head(r):
    here, mate = (r["tid"], r["pos"]), (r["mtid"], r["mpos"])
    return here < mate or (here == mate and bool(r["flag"] & F_READ1))


def group_key(r):
    return (r["tid"], r["pos"], r["mtid"], r["mpos"], r["flag"] & F_REV, r["flag"] & F_MREV)


def score(r):
    q = quals(r)
    if len(q) == 0 or q[0] == 0xff:
        return 0
    return sum(x for x in q if x >= 15) & 0xffffffff


def digest(r, bits=64):
    """the pair's digest: a head's from (tid, pos, mtid, mpos), a tail's from (mtid, mpos, tid, pos) - its head's"""
    four = (r["tid"], r["pos"], r["mtid"], r["mpos"]) if is_head(r) else (r["mtid"], r["mpos"], r["tid"], r["pos"])
    return fnv1a(struct.pack("<4i", *four), fnv1a(r["qname"].encode())) & ((1 << bits) - 1)


def runs(records):
    """maximal stretches of consecutive records with equal (tid, pos) -> [(first, end)]"""
    out, s = [], 0
    for i in range(1, len(records) + 1):
        if i == len(records) or (records[i]["tid"], records[i]["pos"]) != (records[s]["tid"], records[s]["pos"]):
            out.append((s, i))
            s = i
    return out if records else []


def mark(records, digest_bits=64, stats=None):
    """-> the flags of all records after marking.  stats (a dict, optional) gets the counts of ssv_dup_stats that are a function of the file."""
    flags = [r["flag"] for r in records]
    in_set = set()          # digests of the marked heads of this run and of the runs before it
    n_groups = n_heads = n_tails = 0
    for s, e in runs(records):
        groups = {}
        for i in range(s, e):
            if takes_part(records[i]) and is_head(records[i]):
                groups.setdefault(group_key(records[i]), []).append(i)
        for members in groups.values():
            keeper = max(members, key=lambda i: (score(records[i]), -i))
            for i in members:
                if i != keeper:
                    flags[i] |= F_DUP
                    in_set.add(digest(records[i], digest_bits))
                    n_heads += 1
        if e - s >= 2:
            n_groups += len(groups)
        for i in range(s, e):
            if takes_part(records[i]) and not is_head(records[i]) and digest(records[i], digest_bits) in in_set:
                flags[i] |= F_DUP
                n_tails += 1
    if stats is not None:
        stats.update(records=len(records), taking_part=sum(takes_part(r) for r in records), groups=n_groups, heads_marked=n_heads, tails_marked=n_tails,
                     set_entries=len(in_set))
    return flags


def sorted_ok(records):
    """(tid, pos) never goes down between two neighbouring records with tid >= 0"""
    return all(not (a["tid"] >= 0 and b["tid"] >= 0 and (b["tid"], b["pos"]) < (a["tid"], a["pos"])) for a, b in zip(records, records[1:]))
