"""The coordinate-sort rule of `seeksv run -u` (include/seeksv_hip.h, ssv_batch_sort) in plain Python: records in, the order out.

A record is anything with r["tid"], r["pos"], r["flag"].  Its key is (t, p): t = n_targets for tid < 0 (unplaced records come last), else tid;
p = (pos + 1) as an unsigned 32-bit number (position -1 in front of position 0).  Records with equal keys keep their input order.  This is the comparison of
libbam 0.1.x's sorter; no external sorter was run or matched.  The sort below is a merge sort written out, so that tests/test_coordsort_inputs.py can hold it
against Python's own `sorted` on the same key."""


def key(r, n_targets):
    if r["tid"] >= n_targets:
        raise ValueError(f"contig id {r['tid']} is not below n_targets {n_targets}")
    return (n_targets if r["tid"] < 0 else r["tid"], (r["pos"] + 1) & 0xffffffff)


def order(records, n_targets):
    """-> the input indices in output order (a stable merge sort: of two equal keys the left run's goes first)"""
    keys = [key(r, n_targets) for r in records]
    runs = [[i] for i in range(len(records))]
    while len(runs) > 1:
        merged = []
        for k in range(0, len(runs) - 1, 2):
            a, b, out, i, j = runs[k], runs[k + 1], [], 0, 0
            while i < len(a) and j < len(b):
                if keys[b[j]] < keys[a[i]]:
                    out.append(b[j]); j += 1
                else:
                    out.append(a[i]); i += 1
            merged.append(out + a[i:] + b[j:])
        if len(runs) % 2:
            merged.append(runs[-1])
        runs = merged
    return runs[0] if runs else []


def is_sorted(records, n_targets):
    keys = [key(r, n_targets) for r in records]
    return all(keys[i] <= keys[i + 1] for i in range(len(keys) - 1))


def cut(n, max_out_records):
    """-> [(first, count)]: the output batches of n sorted records"""
    return [(f, min(max_out_records, n - f)) for f in range(0, n, max_out_records)]


def changes(records, prev_tid=0):
    """the contig changes among the records without UNMAP|MUNMAP (flag & 12 == 0): -> ([(index, tid)], the contig of the last such record)"""
    out = []
    for i, r in enumerate(records):
        if r["flag"] & 12:
            continue
        if r["tid"] != prev_tid:
            out.append((i, r["tid"]))
            prev_tid = r["tid"]
    return out, prev_tid


def batch_changes(batches):
    """the change lists of consecutive batches (lists of records), continued across them from contig 0"""
    out, prev = [], 0
    for b in batches:
        ch, prev = changes(b, prev)
        out.append(ch)
    return out
