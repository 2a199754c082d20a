"""The event stage of getclip, stated plainly in Python + numpy: which clip events a list of batches gives, in BAM order and in the cluster
table's order, and a report of where they fall against the sizes the kernels work in.  It builds on tests/cluster_bins_model.py - _events_of
restates GetSClipReads, its record loop the contig rule - and shares nothing with oracle/seeksv_oracle.c or the kernels.

Input: a pass = a list of batches, each (record dicts, (rec_begin, rec_end) or None), the record dicts being those of
test_random_differential_gpu.random_sample(..., want_records=True).  Two rules are restated here beyond cluster_bins_model's:
  ownership   an event is kept iff own_lo <= (tid << 32 | pos1) < own_hi, with own = ((lo_tid, lo_pos), (hi_tid, hi_pos))
  the range   records before rec_begin give no event and still count as the previous mapped-pair record of the contig rule
              (clip_reads.h:423-438); records from rec_end on do not exist for the pass: they neither give events nor move that state
The table: every input of tests/clip_events_inputs.py makes each event a cluster of its own, so a table row is an event's own strings.  table()
does not trust that: it fails where two events of one bin would pass InsertSeq's comparison (clip_reads.cpp:260-283) at the run's match rate.
"""
import collections

import numpy as np

from cluster_bins_model import F_MUNMAP, F_UNMAP, OPS, _events_of, _strings, rate_ok

Event = collections.namedtuple("Event", "batch rec side tid pos begin ll lr l_qseq n_cigar")


def own_key(tid, pos):
    return (tid << 32) | (pos & 0xFFFFFFFF)


def sort_key(e):
    """the key the pass sorts by: contig, side, position"""
    return (e.tid << 33) | (e.side << 32) | e.pos


def clip_events(batches, min_mapq=1, save_low_quality=False, own=None, initial_last_tid=0):
    """(a) the events of one pass in BAM order, and the contig of the last mapped-pair record the pass saw"""
    out = []
    last_tid = initial_last_tid
    lo_hi = None if own is None else (own_key(*own[0]), own_key(*own[1]))
    for bi, (recs, rng) in enumerate(batches):
        r0, r1 = (0, len(recs)) if rng is None else rng
        for i in range(r1):
            r = recs[i]
            if r["flag"] & (F_UNMAP | F_MUNMAP):
                continue
            prev, last_tid = last_tid, r["tid"]
            if i < r0 or r["tid"] != prev:
                continue
            for side, pos, begin, ll, lr in _events_of(r, min_mapq, save_low_quality):
                if lo_hi is not None and not lo_hi[0] <= own_key(r["tid"], pos) < lo_hi[1]:
                    continue
                out.append(Event(bi, i, side, r["tid"], pos, begin, ll, lr, r["lq"], len(r["ops"])))
    return out, last_tid


def table_order(events):
    """(b) by contig, '5' before '3', by position, BAM order inside a bin (a stable sort of the BAM order)"""
    return sorted(events, key=sort_key)


def table(events, batches, match_rate=0.9):
    """the cluster table of a pass whose events are clusters of their own (checked), with the keys of test_hip_golden.TABLE_KEYS"""
    ev = table_order(events)
    strs = [_strings(batches[e.batch][0][e.rec], e.begin, e.ll, e.lr) for e in ev]
    k = 0
    while k < len(ev):
        j = k
        while j + 1 < len(ev) and sort_key(ev[j + 1]) == sort_key(ev[k]):
            j += 1
        for a in range(k, j + 1):
            for b in range(a + 1, j + 1):
                (sl1, _, sr1, _, _), (sl2, _, sr2, _, _) = strs[a], strs[b]
                n1, n2 = min(len(sl1), len(sl2)), min(len(sr1), len(sr2))
                joins = (rate_ok(int(np.count_nonzero(sl1[len(sl1) - n1:] == sl2[len(sl2) - n1:])), n1, match_rate)
                         and rate_ok(int(np.count_nonzero(sr1[:n2] == sr2[:n2])), n2, match_rate))
                assert not joins, ("two events of one bin would share a cluster", ev[a], ev[b])
        k = j + 1
    n = len(ev)
    t = dict(n_clusters=n, n_events=n)
    t["tid"] = np.array([e.tid for e in ev], np.int32)
    t["pos"] = np.array([e.pos for e in ev], np.int32)
    t["side"] = np.array([ord("53"[e.side]) for e in ev], np.uint8)
    t["support"] = np.ones(n, np.int32)
    t["left_len"] = np.array([e.ll for e in ev], np.int32)
    t["right_len"] = np.array([e.lr for e in ev], np.int32)
    t["qual_missing"] = np.array([1 if s[4] else 0 for s in strs], np.uint8)
    t["n_cigar"] = np.array([e.n_cigar for e in ev], np.int32)
    blocks = (2 * (t["left_len"].astype(np.int64) + t["right_len"]) + 3) & ~3
    t["str_off"] = np.concatenate([[0], np.cumsum(blocks)[:-1]]).astype(np.uint64) if n else np.zeros(0, np.uint64)
    t["cigar_off"] = np.concatenate([[0], np.cumsum(t["n_cigar"])[:-1]]).astype(np.uint64) if n else np.zeros(0, np.uint64)
    s = np.zeros(int(blocks.sum()), np.uint8)
    cig = []
    for k, e in enumerate(ev):
        o = int(t["str_off"][k])
        cat = np.concatenate(strs[k][:4])
        s[o:o + len(cat)] = cat
        cig += [(l << 4) | OPS.index(op) for l, op in batches[e.batch][0][e.rec]["ops"]]
    t["str"] = s
    t["cigar"] = np.array(cig, np.uint32)
    return t


def concat(tables):
    """the tables of passes that follow each other"""
    if len(tables) == 1:
        return tables[0]
    t = dict(n_clusters=sum(x["n_clusters"] for x in tables), n_events=sum(x["n_events"] for x in tables))
    for k in ("tid", "pos", "side", "support", "left_len", "right_len", "qual_missing", "n_cigar", "str", "cigar"):
        t[k] = np.concatenate([x[k] for x in tables])
    for k, size in (("str_off", "str"), ("cigar_off", "cigar")):
        base, parts = 0, []
        for x in tables:
            parts.append(x[k] + np.uint64(base))
            base += len(x[size])
        t[k] = np.concatenate(parts).astype(np.uint64)
    return t


def is_candidate(r):
    """what the streaming pass lets through: an S at either end of the CIGAR"""
    return bool(r["ops"]) and (r["ops"][0][1] == "S" or r["ops"][-1][1] == "S")


def largest_inversion(keys):
    """the largest j - i over pairs i < j with keys[i] > keys[j] (0: the list ascends)"""
    keys = np.asarray(keys, np.int64)
    if len(keys) < 2:
        return 0
    top = np.maximum.accumulate(keys)
    first_greater = np.searchsorted(top, keys, side="right")   # the first place whose running maximum exceeds keys[j]
    return int(max(0, (np.arange(len(keys)) - first_greater).max()))


def report(events, batches, tile, sub_tile, seg=16, wave=64, block=256):
    """(c) where the pass's candidates and events fall.  Per batch (over the records the scan sees, [0, rec_end)): candidates per scan tile and
    per sub-tile, events per `seg`, `wave` and `block` candidates (in candidate order), the events of every candidate; for the pass: whether the
    '5' keys ascend, the largest distance in places between an inverted pair of the '3' list, the largest key and its bit length"""
    per_batch = []
    for bi, (recs, rng) in enumerate(batches):
        r1 = len(recs) if rng is None else rng[1]
        cand = [i for i in range(r1) if is_candidate(recs[i])]
        n_ev = collections.Counter(e.rec for e in events if e.batch == bi)
        per_cand = [n_ev.get(i, 0) for i in cand]
        group = lambda n: [sum(per_cand[k:k + n]) for k in range(0, len(per_cand), n)]
        count = lambda n: [sum(1 for i in cand if k <= i < k + n) for k in range(0, r1, n)]
        per_batch.append(dict(n=r1, cand=cand, per_cand=per_cand, tiles=count(tile), sub_tiles=count(sub_tile),
                              per_seg=group(seg), per_wave=group(wave), per_block=group(block)))
    k5 = [sort_key(e) for e in events if e.side == 0]
    k3 = [sort_key(e) for e in events if e.side == 1]
    top = max(k5 + k3) if events else 0
    return dict(batches=per_batch, n5=len(k5), n3=len(k3), ascend5=all(a <= b for a, b in zip(k5, k5[1:])), inversion3=largest_inversion(k3),
                max_key=top, key_bits=max(1, int(top).bit_length()), max5=max(k5) if k5 else 0, max3=max(k3) if k3 else 0)
