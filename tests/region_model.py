"""The region rule of `seeksv run -L` / `-X` (include/seeksv_hip.h, ssv_regions_set) in plain Python: records and a list of regions in, the kept records out.
It follows `samtools view -L` in outline; the rule is this project's own, no external tool was run or matched.

A record is anything with r["tid"], r["pos"], r["flag"] and r["cigar"] (text, "*" or empty: none).  A region is (tid, s, t), 0-based half-open as in BED.
  interval  [pos, e) with e = pos + max(span, 1), span = the sum of the lengths of the M, D, N, = and X operations (Python integers: no width to overflow).
            pos == -1 gives [-1, 0) whatever the CIGAR says.
  overlap   tid >= 0 and some region of contig tid has s < e and pos < t.  No flag bit takes part.
  keep      include mode: the record overlaps; exclude mode: it does not (unplaced records stay).
overlaps() is a brute-force loop over the regions AS GIVEN - in any order, overlapping, reaching past the contig's end - so that the host's sorting, merging
and clipping (and normalise() below, which makes the lists handed to the library) are held against it and not against themselves."""
import re

CIGAR_RE = re.compile(r"(\d+)([MIDNSHP=X])")
REF_OPS = "MDN=X"


def span(r):
    c = r["cigar"]
    if not c or c == "*":
        return 0
    return sum(int(n) for n, op in CIGAR_RE.findall(c) if op in REF_OPS)


def interval(r):
    if r["pos"] < 0:
        return r["pos"], 0
    return r["pos"], r["pos"] + max(span(r), 1)


def overlaps(r, regions):
    if r["tid"] < 0:
        return False
    pos, e = interval(r)
    for tid, s, t in regions:
        if tid == r["tid"] and s < e and pos < t:
            return True
    return False


def keep(records, regions, exclude=False):
    """-> the indices of the kept records, in order"""
    return [i for i, r in enumerate(records) if overlaps(r, regions) != bool(exclude)]


def normalise(regions, lens):
    """the list as the library takes it: per contig sorted by s, regions that overlap or abut merged, t clipped to the contig's length, a region that the
    clipping leaves empty dropped; contigs in ascending order.  A region with s < 0, t <= s or a contig outside the header is an error here."""
    per = {}
    for tid, s, t in regions:
        if not 0 <= tid < len(lens) or s < 0 or t <= s:
            raise ValueError(f"bad region {(tid, s, t)}")
        t = min(t, lens[tid])
        if s < t:
            per.setdefault(tid, []).append((s, t))
    out = []
    for tid in sorted(per):
        cur = None
        for s, t in sorted(per[tid]):
            if cur is not None and s <= cur[1]:
                cur[1] = max(cur[1], t)
            else:
                if cur is not None:
                    out.append((tid, cur[0], cur[1]))
                cur = [s, t]
        out.append((tid, cur[0], cur[1]))
    return out


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


def tid_runs(records):
    """the tid column as runs: [(first, tid)]"""
    out = []
    for i, r in enumerate(records):
        if i == 0 or records[i - 1]["tid"] != r["tid"]:
            out.append((i, r["tid"]))
    return out
