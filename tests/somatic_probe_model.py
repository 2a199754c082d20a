"""Plain-Python model of `seeksv somatic`'s look-ups among the normal sample's clusters: the case analysis that turns a row of the tumor's SV table
into two probes (reference somatic.cpp:58-427; the project's probe_normal_clusters / build_cluster_probes, seeksv_amd/host/somatic_stage.cpp), and the rule by
which a probe finds its cluster in the cluster tables of consecutive getclip passes (the kernel k_somatic_probe, seeksv_amd/csrc/probe_kernels.h).  Written from
the rule's words, not from either implementation; tests/test_somatic_probe_model.py anchors it on the real reference's output.

A cluster is (tid, pos, side, seq_left, seq_right, support), side '5' or '3'; a pass is the list of its clusters in table order.
A probe is a dict: tid, lo, hi, side, mode (0 exact, 1 anchored with the cluster first, 2 anchored with the probe first), a, b."""
import numpy as np

from seeksv_amd import host

_COMP = {"A": "T", "a": "T", "T": "A", "t": "A", "C": "G", "c": "G", "G": "C", "g": "C", "N": "N", "n": "N"}


def revcomp(s):
    """GetReverseComplementSeq, clip_reads.cpp:414: every other character stays what it is"""
    return "".join(_COMP.get(c, c) for c in reversed(s))


# ---- the rule ----

def begin(x, y, rate):
    n = min(len(x), len(y))
    if n == 0:
        return False  # 0 / 0 is NaN on the host: never a match
    m = sum(1 for i in range(n) if x[i] == y[i])
    return m / n >= rate  # (int / int in Python is the correctly rounded quotient: the reference's (double)m / n)


def end(x, y, rate):
    return begin(x[::-1], y[::-1], rate)


def anchored(s1, s2, s3, s4, rate):
    """Compare, clip_reads.cpp:333-370"""
    if len(s2) < 10:
        return False
    h = s4.find(s2[:10])
    if h < 0:
        return False
    return end(s1, s3 + s4[:h], rate) and begin(s2, s4[h:], rate)


def matches(p, left, right, rate):
    if p["mode"] == 0:
        return begin(p["b"], right, rate) and end(p["a"], left, rate)
    if p["mode"] == 1:
        return anchored(left, right, p["a"], p["b"], rate)
    return anchored(p["a"], p["b"], left, right, rate)


def probe_pass(p, clusters, rate, min_clipped_len):
    """the first matching cluster of one pass's table -> (support, pos, index in the table) or None"""
    if p["tid"] < 0:
        return None
    min_len = min_clipped_len & 0xFFFFFFFF  # unsigned compare, somatic.h:54
    cand = [(c[1], k) for k, c in enumerate(clusters) if c[0] == p["tid"] and c[2] == p["side"] and p["lo"] <= c[1] <= p["hi"]]
    cand.sort()  # by position, ties in table (creation) order
    for pos, k in cand:
        _, _, side, left, right, support = clusters[k]
        if len(left if side == "5" else right) < min_len:
            continue
        if matches(p, left, right, rate):
            return support, pos, k
    return None


def probe_passes(probes, passes, rate=0.9, min_clipped_len=10):
    """-> per probe (support, pos, pass, cluster), (0, 0, 0, 0) = no cluster matched.  Over passes the order is the reference's multimap's: smaller
    position first, equal positions in pass order - a later pass's match replaces the stored one only at a strictly smaller position."""
    out = []
    for p in probes:
        hit = None
        for n, clusters in enumerate(passes):
            h = probe_pass(p, clusters, rate, min_clipped_len)
            if h is not None and (hit is None or h[1] < hit[1]):
                hit = (h[0], h[1], n, h[2])
        out.append(hit or (0, 0, 0, 0))
    return out


# ---- a row's case analysis ----

def parse_tumor_rows(text):
    """the junction rows of a tumor SV table as the reference's stream extraction reads them -> list of dicts (lines starting with '@' are headers)"""
    rows = []
    for line in text.splitlines():
        if not line.strip() or line.startswith("@"):
            continue
        c = line.split()
        rows.append(dict(up_chr=c[0], up_pos=int(c[1]), up_strand=c[2], up_reads=int(c[3]), down_chr=c[4], down_pos=int(c[5]), down_strand=c[6], down_reads=int(c[7]),
                         mh=int(c[8]), up_seq=c[21], down_seq=c[22], text="\t".join(c[:23])))
    return rows


def row_kind(r):
    """'junction', or why the reference writes no output row for it"""
    pair = r["up_strand"] + r["down_strand"]
    if pair not in ("++", "+-", "-+"):
        return "strands"
    if r["mh"] == -1 and r["up_reads"] != 0 and r["down_reads"] != 0:
        return "tandem"
    return "junction"


def row_probes(r, offset):
    """(left probe, right probe) of a junction row, tid left as the contig's NAME under 'chr'; None = no look-up, the count stays 0"""
    up, down, mh = r["up_seq"], r["down_seq"], r["mh"]
    rc_up, rc_down = revcomp(up), revcomp(down)
    pair = r["up_strand"] + r["down_strand"]

    def exact(side, chrom, pos, a, b):
        return dict(side=side, chr=chrom, lo=pos, hi=pos, mode=0, a=a, b=b)

    def rng(side, chrom, lo, hi, cluster_first, a, b):
        return dict(side=side, chr=chrom, lo=lo, hi=hi, mode=1 if cluster_first else 2, a=a, b=b)
    uc, dc, upos, dpos = r["up_chr"], r["down_chr"], r["up_pos"], r["down_pos"]
    if mh != -1:
        umh = mh & 0xFFFFFFFFFFFFFFFF  # (size_t)mh
        if pair == "++":
            right = exact("5", dc, dpos, up, down)
            left = exact("3", uc, upos + mh, up + down[:umh], down[umh:]) if len(down) >= umh else None
        elif pair == "+-":
            left = exact("3", uc, upos + mh, up + down[:umh], down[umh:])
            right = exact("3", dc, dpos, rc_down, rc_up)
        else:
            left = exact("5", uc, upos, rc_down, rc_up)
            cut = len(up) - mh
            right = exact("5", dc, dpos - mh, up[:cut], up[cut:] + down)
    elif r["up_reads"] == 0:
        if pair == "++":
            right, left = exact("5", dc, dpos, up, down), rng("3", uc, upos, upos + offset, True, up, down)
        elif pair == "+-":
            right, left = exact("3", dc, dpos, rc_down, rc_up), rng("3", uc, upos, upos + offset, True, up, down)
        else:
            right, left = exact("5", dc, dpos, up, down), rng("5", uc, upos - offset, upos, False, rc_up, rc_down)
    else:
        if pair == "++":
            left, right = exact("3", uc, upos, up, down), rng("5", dc, dpos - offset, dpos, False, up, down)
        elif pair == "+-":
            left, right = exact("3", uc, upos, up, down), rng("3", dc, dpos, dpos + offset, True, rc_down, rc_up)
        else:
            left, right = exact("5", uc, upos, rc_down, rc_up), rng("5", dc, dpos - offset, dpos, False, up, down)
    return left, right


def with_tid(p, names):
    """the probe with its contig's id in `names` (the first of equal names; -1: not there)"""
    q = dict(p)
    q["tid"] = names.index(p["chr"]) if p["chr"] in names else -1
    return q


def somatic_counts(rows, names, passes, offset=30, rate=0.9, min_clipped_len=10):
    """per junction row of `rows` (parse_tumor_rows) its (normal_left_reads, normal_right_reads)"""
    probes, where = [], []
    for r in rows:
        if row_kind(r) != "junction":
            continue
        pr = row_probes(r, offset)
        where.append(tuple(len(probes) + sum(1 for q in pr[:k] if q is not None) if pr[k] is not None else -1 for k in (0, 1)))
        probes += [with_tid(q, names) for q in pr if q is not None]
    hits = probe_passes(probes, passes, rate, min_clipped_len)
    return [(hits[a][0] if a >= 0 else 0, hits[b][0] if b >= 0 else 0) for a, b in where]


# ---- tables ----

def table_clusters(d):
    """a cluster table dict (seeksv_amd.host.table_to_dict; the oracle's or the library's, either format) -> the pass's clusters in table order"""
    out = []
    for k in range(int(d["n_clusters"])):
        sl, _, sr, _, _ = host.cluster_strings(d, k)
        out.append((int(d["tid"][k]), int(d["pos"][k]), chr(int(d["side"][k])), sl, sr, int(d["support"][k])))
    return out


def hits_array(hits):
    """model hits as the structured array Context.clip_probe_get returns (without the padding)"""
    return np.array(hits, dtype=[("support", "<i4"), ("pos", "<i4"), ("pass", "<i4"), ("cluster", "<i8")])
