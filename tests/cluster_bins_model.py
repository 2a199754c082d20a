"""A second, independent statement of getclip's record loop and of InsertSeq / ChangeSeqAndQual in plain Python + numpy (no ctypes, nothing
shared with oracle/seeksv_oracle.c or the kernels): the model that tests/test_cluster_bins_*.py hold the consensus clustering walk to.

Input: the record dicts of test_random_differential_gpu.random_sample(..., want_records=True) - tid, pos, flag, mapq, ops [(len, op char)],
lq, seq (text), qual (uint8 array, all 255 = no qualities), xc.  Output: the cluster table with the keys of test_hip_golden.TABLE_KEYS in the
reference's flush order, and a per-bin report (events, clusters, which cluster took each event).

Rules restated (file:line of the reference, seeksv v1.2.3):
  record loop        clip_reads.h:407-446   - last_tid starts at 0; the first record of another contig only flushes, it is not looked at
  GetSClipReads      clip_reads.cpp:112-192 - H at either end, MAPQ, duplicate, XC; one-end and both-end clips; a lone nS is both ends at once
  InsertSeq          clip_reads.cpp:260-283 - the first cluster of the (side, pos) bin whose both sides pass takes the event
  CompareString*     clip_reads.cpp:194-217 - left sides from their ends, right sides from their starts, (double) m / n >= rate, 0 / 0 fails
  ChangeSeqAndQual   clip_reads.cpp:57-108  - signed quality compare; prepend when len1 <= len2, append when len1 < len2; the CIGAR carrier
"""
import numpy as np

F_UNMAP, F_MUNMAP, F_REV, F_DUP = 4, 8, 16, 1024
REF_OPS = "MD=N"       # GenerateCigar's length (clip_reads.cpp:309-329): X is not counted
OPS = "MIDNSHP=X"


def rate_ok(m, n, rate):
    """(double) m / (double) n >= rate with Python floats (IEEE doubles); n == 0 never passes (0 / 0 is NaN in the reference)"""
    return n > 0 and m / n >= rate


def minm(n, rate):
    """the smallest m in 0 .. n that passes for an overlap of n (n + 1: none does), by that very division"""
    for m in range(n + 1):
        if rate_ok(m, n, rate):
            return m
    return n + 1


class _Cluster:
    __slots__ = ("sl", "ql", "sr", "qr", "support", "rec", "qmiss", "pos", "order")


def _events_of(r, min_mapq, save_low_quality):
    """the clip events of one record: [(side 0 / 1, pos, begin, left length, right length)]"""
    ops = r["ops"]
    if not ops or r["tid"] < 0:
        return []
    (l1, o1), (l2, o2) = ops[0], ops[-1]
    if o1 == "H" or o2 == "H" or r["mapq"] < min_mapq or r["flag"] & F_DUP:
        return []
    s1, s2 = o1 == "S", o2 == "S"
    if not s1 and not s2:
        return []
    lq, pos0 = r["lq"], r["pos"]
    ref_len = sum(l for l, op in ops if op in REF_OPS)
    low = r["xc"] != 0 and not save_low_quality
    if s1 != s2:
        if low:
            return []
        if s1:
            return [(0, pos0 + 1, 0, l1, lq - l1)] if lq - l1 >= 0 else []
        return [(1, pos0 + ref_len, 0, lq - l2, l2)] if lq - l2 >= 0 else []
    if l1 > lq or l2 > lq:
        return []
    mid = lq - l1 - l2
    midc = max(mid, 0)
    out = []
    if not (low and r["flag"] & F_REV):
        out.append((0, pos0 + 1, 0, l1, midc))
    if not (low and not r["flag"] & F_REV):
        out.append((1, pos0 + ref_len, l1 + mid - midc, midc, l2))
    return out


def _strings(r, begin, ll, lr):
    s = np.frombuffer(r["seq"].encode(), np.uint8)
    q = np.asarray(r["qual"], np.uint8)
    qmiss = r["lq"] > 0 and int(q[0]) == 255
    qa = np.full(r["lq"], ord("*"), np.uint8) if qmiss else (q + np.uint8(33))
    a, b, c = begin, begin + ll, begin + ll + lr
    return s[a:b].copy(), qa[a:b].copy(), s[b:c].copy(), qa[b:c].copy(), qmiss


def getclip_model(recs, match_rate=0.9, min_mapq=1, save_low_quality=False, initial_last_tid=0):
    """-> (table, bins).  bins: per (contig visit, side, pos) bin in the table's order, dict(tid, side ('5' / '3'), pos, n_events, n_clusters,
    recs [record index of every event, in order], assign [its cluster's number within the bin], row0 [table row of the bin's first cluster])"""
    maps = [{}, {}]    # side -> pos -> dict(clusters, recs, assign)
    rows, bins = [], []
    n_events = 0
    created = 0

    def flush(tid):
        for side in (0, 1):
            for pos in sorted(maps[side]):
                b = maps[side][pos]
                bins.append(dict(tid=tid, side="53"[side], pos=pos, n_events=len(b["recs"]), n_clusters=len(b["clusters"]), recs=b["recs"],
                                 assign=b["assign"], row0=len(rows)))
                for c in b["clusters"]:   # (a bin's clusters: insertion order)
                    rows.append((tid, side, c))
            maps[side].clear()

    last_tid = initial_last_tid
    for i, r in enumerate(recs):
        if r["flag"] & (F_UNMAP | F_MUNMAP):
            continue
        if r["tid"] != last_tid:
            flush(last_tid)
            last_tid = r["tid"]
            continue
        for side, pos, begin, ll, lr in _events_of(r, min_mapq, save_low_quality):
            sl, ql, sr, qr, qmiss = _strings(r, begin, ll, lr)
            n_events += 1
            b = maps[side].setdefault(pos, dict(clusters=[], recs=[], assign=[]))
            b["recs"].append(i)
            for k, c in enumerate(b["clusters"]):
                n1 = min(ll, len(c.sl))
                if not rate_ok(int(np.count_nonzero(sl[ll - n1:] == c.sl[len(c.sl) - n1:])), n1, match_rate):
                    continue
                n2 = min(lr, len(c.sr))
                if not rate_ok(int(np.count_nonzero(sr[:n2] == c.sr[:n2])), n2, match_rate):
                    continue
                # the left sides meet at their ends
                len1 = len(c.sl)
                better = c.ql[len1 - n1:].view(np.int8) < ql[ll - n1:].view(np.int8)
                c.ql[len1 - n1:][better] = ql[ll - n1:][better]
                c.sl[len1 - n1:][better] = sl[ll - n1:][better]
                if len1 <= ll:
                    c.sl = np.concatenate([sl[:ll - len1], c.sl])
                    c.ql = np.concatenate([ql[:ll - len1], c.ql])
                    if side == 1:
                        c.rec = i
                # the right sides at their starts
                len1 = len(c.sr)
                better = c.qr[:n2].view(np.int8) < qr[:n2].view(np.int8)
                c.qr[:n2][better] = qr[:n2][better]
                c.sr[:n2][better] = sr[:n2][better]
                if len1 < lr:
                    c.sr = np.concatenate([c.sr, sr[len1:]])
                    c.qr = np.concatenate([c.qr, qr[len1:]])
                    if side == 0:
                        c.rec = i
                c.support += 1
                b["assign"].append(k)
                break
            else:
                c = _Cluster()
                c.sl, c.ql, c.sr, c.qr, c.support, c.rec, c.qmiss, c.pos, c.order = sl, ql, sr, qr, 1, i, qmiss, pos, created
                created += 1
                b["assign"].append(len(b["clusters"]))
                b["clusters"].append(c)
    flush(last_tid)

    n = len(rows)
    t = dict(n_clusters=n, n_events=n_events)
    t["tid"] = np.array([x[0] for x in rows], np.int32)
    t["pos"] = np.array([x[2].pos for x in rows], np.int32)
    t["side"] = np.array([ord("53"[x[1]]) for x in rows], np.uint8)
    t["support"] = np.array([x[2].support for x in rows], np.int32)
    t["left_len"] = np.array([len(x[2].sl) for x in rows], np.int32)
    t["right_len"] = np.array([len(x[2].sr) for x in rows], np.int32)
    t["qual_missing"] = np.array([1 if x[2].qmiss else 0 for x in rows], np.uint8)
    t["n_cigar"] = np.array([len(recs[x[2].rec]["ops"]) for x in rows], np.int32)
    blocks = (2 * (t["left_len"].astype(np.int64) + t["right_len"]) + 3) & ~3     # a cluster's strings: a block of whole dwords, zero filled
    t["str_off"] = np.concatenate([[0], np.cumsum(blocks)[:-1]]).astype(np.uint64) if n else np.zeros(0, np.uint64)
    t["cigar_off"] = np.concatenate([[0], np.cumsum(t["n_cigar"])[:-1]]).astype(np.uint64) if n else np.zeros(0, np.uint64)
    s = np.zeros(int(blocks.sum()), np.uint8)
    cig = []
    for k, (_, _, c) in enumerate(rows):
        o = int(t["str_off"][k])
        cat = np.concatenate([c.sl, c.ql, c.sr, c.qr])
        s[o:o + len(cat)] = cat
        cig += [(l << 4) | OPS.index(op) for l, op in recs[c.rec]["ops"]]
    t["str"] = s
    t["cigar"] = np.array(cig, np.uint32)
    return t, bins
