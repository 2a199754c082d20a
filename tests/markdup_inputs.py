"""Hand-made record sets for the duplicate-marking rule of `seeksv run -M`, each with the answer written beside it: `dup` lists the records (by index in file
order) that the rule marks, worked out by hand from the rule's text (include/seeksv_hip.h), not by running tests/markdup_model.py.  The model is held to these
(tests/test_markdup_model.py), the kernels to the model (tests/test_markdup_gpu.py).  `claim` states what a set is about; tests/test_markdup_inputs.py asserts it.

Records are dicts as tests/bamio.py's encode_record takes them.  Every set is coordinate sorted."""

TARGETS = ["c0", "c1", "c2"]
TARGET_LENS = [100000, 100000, 100000]
Q30 = bytes([30] * 10)
HEAD, TAIL = 0x41 | 0x20, 0x81 | 0x10    # a usual pair: first read forward with its mate reversed, second read reversed


def rec(qname, tid, pos, mtid, mpos, flag, qual=Q30, cigar=None, seq=None):
    n = len(qual) if qual is not None else 10
    seq = "ACGTACGTACGTACGT"[:n] if seq is None else seq
    return dict(qname=qname, flag=flag, tid=tid, pos=pos, mapq=60, cigar=f"{len(seq) or 10}M" if cigar is None else cigar, mtid=mtid, mpos=mpos, isize=0, seq=seq, qual=qual)


def pair(qname, tid, pos, mtid, mpos, qual=Q30, hflag=HEAD, tflag=TAIL):
    """(head, tail) of one pair whose first read lies at (tid, pos) and whose second at (mtid, mpos) > (tid, pos)"""
    return rec(qname, tid, pos, mtid, mpos, hflag, qual), rec(qname, mtid, mpos, tid, pos, tflag)


def in_order(records):
    """stable sort by (tid, pos) with tid -1 last -> (records, where each input record went)"""
    order = sorted(range(len(records)), key=lambda i: ((records[i]["tid"] if records[i]["tid"] >= 0 else 1 << 30), records[i]["pos"]))
    return [records[i] for i in order], {i: k for k, i in enumerate(order)}


def q(n):
    return bytes([n] * 10)


SETS = []


def add(name, records, dup, **claim):
    SETS.append(dict(name=name, records=records, dup=sorted(dup), claim=claim))


# ---- keys that differ in exactly one field: the variant is no duplicate of the base pair, the copy is ----
def _key_set(name, field, variant_head):
    base_h, base_t = pair("base", 0, 100, 1, 300)
    copy_h, copy_t = pair("copy", 0, 100, 1, 300, qual=q(20))
    # file order: base head, variant head, copy head | tails at c1:300 (base, copy) - the variant's tail lies where its mate fields say
    vt = rec("var", variant_head["mtid"], variant_head["mpos"], 0, 100, TAIL)
    recs, at = in_order([base_h, variant_head, copy_h, base_t, copy_t, vt])
    add(name, recs, [at[2], at[4]], differs_in=field, heads_at_first_run=3)


_key_set("key_mtid", "mtid", rec("var", 0, 100, 2, 300, HEAD))
_key_set("key_mpos", "mpos", rec("var", 0, 100, 1, 301, HEAD))
_key_set("key_rev", "0x10", rec("var", 0, 100, 1, 300, HEAD | 0x10))
_key_set("key_mrev", "0x20", rec("var", 0, 100, 1, 300, HEAD & ~0x20))

# ---- head / tail at equal positions: 0x40 decides.  Both reads of both pairs lie at c0:100; q's first read scores lower ----
add("tie_0x40", [rec("p", 0, 100, 0, 100, 0x41), rec("p", 0, 100, 0, 100, 0x81), rec("q", 0, 100, 0, 100, 0x41, q(20)), rec("q", 0, 100, 0, 100, 0x81)],
    [2, 3], heads=[0, 2], tails=[1, 3])

# ---- scores ----
add("score_tie_earlier", [rec("a", 0, 100, 0, 500, HEAD), rec("b", 0, 100, 0, 500, HEAD), rec("c", 0, 100, 0, 500, HEAD),
                           rec("a", 0, 500, 0, 100, TAIL), rec("b", 0, 500, 0, 100, TAIL), rec("c", 0, 500, 0, 100, TAIL)], [1, 2, 4, 5], scores=[300, 300, 300])
# fourteen does not count, fifteen does: the earlier head scores 0 and loses
add("score_14_15", [rec("a", 0, 100, 0, 500, HEAD, q(14)), rec("b", 0, 100, 0, 500, HEAD, bytes([15] * 9 + [0])),
                     rec("a", 0, 500, 0, 100, TAIL), rec("b", 0, 500, 0, 100, TAIL)], [0, 2], scores=[0, 135])
# no qualities (0xff): score 0, loses against one quality of 15 among fourteens
add("score_ff", [rec("a", 0, 100, 0, 500, HEAD, None), rec("b", 0, 100, 0, 500, HEAD, bytes([14] * 9 + [15])),
                  rec("a", 0, 500, 0, 100, TAIL), rec("b", 0, 500, 0, 100, TAIL)], [0, 2], scores=[0, 15])
# l_qseq 0 and 0xff both score 0: the earlier stays
add("score_lq0", [rec("a", 0, 100, 0, 500, HEAD, b"", cigar="10M", seq=""), rec("b", 0, 100, 0, 500, HEAD, None),
                   rec("a", 0, 500, 0, 100, TAIL), rec("b", 0, 500, 0, 100, TAIL)], [1, 3], scores=[0, 0])

# ---- records that take no part: each would win or lose the group if it did.  The real pairs: k (kept), d (its copy) ----
_np = [rec("u4", 0, 100, 0, 500, HEAD | 0x4, q(40)), rec("u8", 0, 100, 0, 500, HEAD | 0x8, q(40)), rec("sec", 0, 100, 0, 500, HEAD | 0x100, q(40)),
       rec("sup", 0, 100, 0, 500, HEAD | 0x800, q(40)), rec("pre", 0, 100, 0, 500, HEAD | 0x400, q(40)), rec("single", 0, 100, 0, 500, HEAD & ~0x1, q(40)),
       rec("nomate", 0, 100, -1, -1, HEAD, q(40)),
       rec("k", 0, 100, 0, 500, HEAD), rec("d", 0, 100, 0, 500, HEAD, q(20)),
       rec("k", 0, 500, 0, 100, TAIL), rec("d", 0, 500, 0, 100, TAIL), rec("pre", 0, 500, 0, 100, TAIL), rec("d", 0, 500, 0, 100, TAIL | 0x400),
       rec("x", -1, -1, -1, -1, 0x4d), rec("x", -1, -1, -1, -1, 0x8d), rec("odd", -1, -1, 0, 100, HEAD)]
add("no_part", _np, [8, 10], no_part=[0, 1, 2, 3, 4, 5, 6, 12, 13, 14, 15], preset=[4, 12])

# ---- tails ----
# a tail before its head inside one run (both reads of a pair at one position): d's second read comes first in the file
add("tail_before_head", [rec("d", 0, 100, 0, 100, 0x81), rec("k", 0, 100, 0, 100, 0x41), rec("d", 0, 100, 0, 100, 0x41, q(20)), rec("k", 0, 100, 0, 100, 0x81)],
    [0, 2], tails=[0, 3])
# a tail whose head is kept; a tail whose mate fields point at a place where no head lies
add("tail_kept_and_stray", [rec("k", 0, 100, 0, 500, HEAD), rec("d", 0, 100, 0, 500, HEAD, q(20)), rec("k", 0, 500, 0, 100, TAIL), rec("d", 0, 500, 0, 100, TAIL),
                             rec("d", 0, 500, 0, 101, TAIL), rec("d", 0, 500, 1, 100, TAIL)], [1, 3], stray=[4, 5])

# ---- names ----
# one name on two pairs: x at 100 -> 500 is a copy of k and is marked with its tail; x at 100 -> 600 is alone in its group, and its tail's digest differs
add("equal_names", [rec("k", 0, 100, 0, 500, HEAD), rec("x", 0, 100, 0, 500, HEAD, q(20)), rec("x", 0, 100, 0, 600, HEAD),
                     rec("k", 0, 500, 0, 100, TAIL), rec("x", 0, 500, 0, 100, TAIL), rec("x", 0, 600, 0, 100, TAIL)], [1, 4], shared_name="x")
_long = "L" * 254
add("name_lengths", [rec("k", 0, 100, 0, 500, HEAD), rec("s", 0, 100, 0, 500, HEAD, q(20)), rec(_long, 0, 100, 0, 500, HEAD, q(10)),
                      rec("k", 0, 500, 0, 100, TAIL), rec("s", 0, 500, 0, 100, TAIL), rec(_long, 0, 500, 0, 100, TAIL)], [1, 2, 4, 5], lengths=[1, 254])


# ---- runs of n heads: all of one key (the best, somewhere in the middle, stays; every other head and its tail is marked), all of distinct keys (none) ----
def _run_one_key(n):
    best = n // 2
    heads = [rec(f"r{k}", 0, 1000, 0, 5000, HEAD, q(31 if k == best else 30 - k % 3)) for k in range(n)]
    tails = [rec(f"r{k}", 0, 5000, 0, 1000, TAIL) for k in range(n)]
    add(f"run_{n}_one_key", heads + tails, [k for k in range(n) if k != best] + [n + k for k in range(n) if k != best], heads=n, groups=1, best=best)


def _run_distinct(n):
    heads = [rec(f"r{k}", 0, 1000, 0, 5000 + k, HEAD) for k in range(n)]
    tails = [rec(f"r{k}", 0, 5000 + k, 0, 1000, TAIL) for k in range(n)]
    add(f"run_{n}_distinct", heads + tails, [], heads=n, groups=n)


for _n in (1, 2, 63, 64, 65, 130, 1000):
    _run_one_key(_n)
    _run_distinct(_n)

# ---- a run of 300 records with two heads (the rest take no part): the second head, of equal score, is marked ----
_filler = [rec(f"f{k}", 0, 2000, 0, 9000, HEAD & ~0x1) for k in range(298)]
add("run_300_two_heads", _filler[:100] + [rec("k", 0, 2000, 0, 9000, HEAD)] + _filler[100:250] + [rec("d", 0, 2000, 0, 9000, HEAD)] + _filler[250:]
    + [rec("k", 0, 9000, 0, 2000, TAIL), rec("d", 0, 9000, 0, 2000, TAIL)], [251, 301], run=300, heads=[100, 251])

# ---- several contigs and positions in one file: what a stream cut anywhere has to get right (a tail far behind its head, runs at the seams) ----
_mixed, _ = in_order(
    list(pair("a", 0, 100, 0, 900)) + list(pair("b", 0, 100, 0, 900, q(20))) + list(pair("c", 0, 100, 2, 50, q(25))) + list(pair("e", 0, 100, 2, 50))
    + list(pair("f", 0, 400, 1, 10)) + list(pair("g", 0, 400, 1, 10, q(35))) + [rec("lone", 1, 10, 1, 10, 0), rec("z", -1, -1, -1, -1, 0x4d), rec("z", -1, -1, -1, -1, 0x8d)])
# file order: c0:100 a b c e | c0:400 f g | c0:900 a' b' | c1:10 f' g' lone | c2:50 c' e' | unplaced z z
add("mixed", _mixed, [1, 2, 4, 7, 8, 11], contigs=3)

# ---- forty places, each with a pair and its copy, the tails ten bases behind their heads: heads of later runs lie behind tails of earlier ones, which matters
# once digests collide (a narrowed digest: a tail may only match a head whose run is not later than its own) ----
_inter = []
for _k in range(40):
    _p = 1000 + 20 * _k
    _inter += [rec(f"k{_k}", 0, _p, 0, _p + 10, HEAD), rec(f"d{_k}", 0, _p, 0, _p + 10, HEAD, q(20)), rec(f"k{_k}", 0, _p + 10, 0, _p, TAIL), rec(f"d{_k}", 0, _p + 10, 0, _p, TAIL)]
add("interleaved", _inter, [4 * k + 1 for k in range(40)] + [4 * k + 3 for k in range(40)], places=40)

BY_NAME = {s["name"]: s for s in SETS}
SMALL = [s for s in SETS if len(s["records"]) <= 20]

UNSORTED = [rec("a", 0, 500, 0, 900, HEAD), rec("b", 0, 100, 0, 900, HEAD)]


def sam_text(records, targets=TARGETS):
    """the records as SAM lines (no header)"""
    out = []
    for r in records:
        name = lambda t: targets[t] if t >= 0 else "*"
        qual = r["qual"]
        seq = r["seq"] or "*"
        qs = "*" if qual is None or not r["seq"] else "".join(chr(33 + x) for x in qual)
        out.append("\t".join([r["qname"], str(r["flag"]), name(r["tid"]), str(r["pos"] + 1), str(r["mapq"]), r["cigar"] or "*", name(r["mtid"]), str(r["mpos"] + 1),
                              str(r["isize"]), seq, qs]) + "\n")
    return "".join(out).encode()
