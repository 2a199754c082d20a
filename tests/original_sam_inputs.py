"""The input sets of tests/test_samdec_sorted_gpu.py: records (dicts as tests/bamio.py and tests/sam_text.py take them) for the device SAM decoder's mode for
coordinate-sorted originals.  tests/test_original_sam_inputs.py asserts, without a GPU, every property the GPU tests claim of them."""
import numpy as np

import readthrough_inputs as RT
import sam_text as ST

NAMES, LENS = RT.NAMES, RT.LENS


def body(recs, names=NAMES, lens=LENS, **kw):
    return ST.text(recs, names, lens, with_header=False, **kw).encode("latin-1")


def cigar_ops(r):
    """[(length, letter)] of a record's CIGAR, [] for '*'"""
    import bamio
    c = r.get("cigar", "")
    return [] if c in ("", "*") else [(l, bamio.CIGAR_OPS[op]) for l, op in bamio.parse_cigar(c)]


def flag_as_decoded(r):
    """libbam's text reader sets UNMAP where the CIGAR is '*'"""
    return r.get("flag", 0) | (0 if cigar_ops(r) else 4)


def ships(r):
    """the BAM decoder's rule (record_fields_of): first or last operation S, and bases to ship"""
    ops = cigar_ops(r)
    return bool(ops) and (ops[0][1] == "S" or ops[-1][1] == "S") and len(r.get("seq", "")) > 0


def side_channel(r):
    return bool(flag_as_decoded(r) & 12)


def changes_model(recs, last=0):
    """getclip's flush sequence (clip_reads.h:423-438): (record, contig) at every change of contig among the records that are not UNMAP|MUNMAP"""
    out = []
    for i, r in enumerate(recs):
        if side_channel(r):
            continue
        if r["tid"] != last:
            out.append((i, r["tid"]))
            last = r["tid"]
    return out


def R(rng, qname, tid, pos, cigar, flag=0, qual=True, **kw):
    r = RT.rec(rng, qname, tid, pos, cigar, flag=flag)
    if qual:
        r["qual"] = bytes(rng.randint(0, 60, len(r["seq"])).astype(np.uint8).tolist())
    r.update(kw)
    return r


def unmapped(rng, qname, n, flag=77, tid=-1, pos=-1, qual=True, **kw):
    r = dict(qname=qname, flag=flag, tid=tid, pos=pos, mapq=0, cigar="*", mtid=-1, mpos=-1, isize=0, seq=RT._seq(rng, n), qual=None)
    if qual and n:
        r["qual"] = bytes(rng.randint(0, 60, n).astype(np.uint8).tolist())
    r.update(kw)
    return r


def shipping_records():
    rng = np.random.RandomState(11)
    recs = [R(rng, "s_first", 0, 100, "7S43M"), R(rng, "s_last", 0, 110, "44M7S", xc=1), R(rng, "s_both", 0, 120, "5S40M6S", xc=0),
            R(rng, "h_s_m", 0, 130, "5H6S40M", xc=3), R(rng, "s_h_last", 0, 135, "40M6S5H"), R(rng, "only_s", 0, 140, "50S"), R(rng, "plain", 0, 150, "50M", xc=5),
            R(rng, "plain_odd", 0, 151, "51M"), R(rng, "s_odd", 0, 160, "8S43M", qual=False), R(rng, "s_even", 0, 161, "8S42M", xc=100),
            unmapped(rng, "star", 33, flag=0, tid=0, pos=170), dict(R(rng, "seq_star", 0, 180, "3S7M"), seq="", qual=None),
            R(rng, "mid_s_only", 0, 190, "10M2I10M"), R(rng, "eq_x", 1, 10, "4S10=2X4S"), R(rng, "s1", 1, 20, "1S1M")]
    return recs


def long_read_records():
    rng = np.random.RandomState(13)
    recs = [R(rng, f"a{k}", 0, 100 + k, "50M" if k % 3 else "10S40M") for k in range(20)]
    recs.insert(7, R(rng, "long", 0, 106, "19000M1000S"))
    recs.insert(12, R(rng, "long_odd", 0, 111, "999S19000M", qual=False))
    return recs


LIST_SIZES = (0, 1, 63, 64, 65, 257)


def list_size_records(k):
    """300 lines of which k ship (spread over the file, the first and the last line among them when k > 1)"""
    rng = np.random.RandomState(20 + k)
    pick = set(np.linspace(0, 299, k).astype(int).tolist()) if k else set()
    return [R(rng, f"r{i}", 0, 10 + i, "6S30M" if i in pick else "36M", xc=i % 3) for i in range(300)]


def side_channel_one():
    rng = np.random.RandomState(30)
    recs = [R(rng, f"m{k}", 0, 100 + k, "30M") for k in range(6)]
    return recs, recs[:3] + [unmapped(rng, "u", 30)] + recs[3:]


def side_channel_forms():
    rng = np.random.RandomState(31)
    return [unmapped(rng, "f", 20), R(rng, "m0", 0, 100, "30M"), unmapped(rng, "a", 1), unmapped(rng, "n" * 254, 31, flag=141),
            R(rng, "m1", 0, 120, "30M", flag=73), R(rng, "mate_gone", 0, 130, "5S20M2D3M1I4M", flag=137, mtid=0, mpos=129, xc=2),
            unmapped(rng, "noseq", 0), unmapped(rng, "noqual", 17, qual=False), R(rng, "m2", 0, 140, "30M"),
            unmapped(rng, "star_mapped_flag", 9, flag=1, tid=0, pos=150), unmapped(rng, "placed", 12, flag=69, tid=0, pos=160, mtid=0, mpos=160), unmapped(rng, "l", 21, flag=133)]


def side_channel_seventy():
    rng = np.random.RandomState(32)
    recs = []
    for k in range(400):
        recs.append(unmapped(rng, f"u{k}", int(rng.randint(0, 70)), flag=77 if k % 2 else 141) if k % 6 == 0 or k in (1, 2, 399) else R(rng, f"m{k}", 0, 100 + k, "4S26M" if k % 7 == 0 else "30M"))
    return recs


def low_quality_sets():
    """-> (three plain lines of which the second has a QUAL byte of 32, [the same with a second line that ships / is UNMAP / is MUNMAP])"""
    rng = np.random.RandomState(33)
    base = [R(rng, "m0", 0, 100, "30M"), R(rng, "m1", 0, 101, "30M"), R(rng, "m2", 0, 102, "30M")]
    low = lambda r: dict(r, qual="I" * (len(r["seq"]) - 3) + " II")  # noqa: E731
    quiet = [base[0], low(base[1]), base[2]]
    refused = [[base[0], low(bad), base[2]] for bad in (R(rng, "clip", 0, 101, "4S26M"), unmapped(rng, "u", 30), R(rng, "mate_gone", 0, 101, "30M", flag=73))]
    return quiet, refused


def change_records():
    """-> (no change: contig 0 throughout; a change on the first record, on the last, two in a row, UNMAP|MUNMAP records of another contig between two of one)"""
    rng = np.random.RandomState(40)
    M = lambda q, t, p, **kw: R(rng, q, t, p, "20M", **kw)  # noqa: E731
    none = [M(f"z{k}", 0, 10 + k) for k in range(4)]
    recs = [M("a", 1, 10), M("b", 1, 11), unmapped(rng, "u0", 10, flag=69, tid=2, pos=5), M("mu", 2, 6, flag=73), M("c", 1, 12), M("d", 2, 1), M("e", 0, 1), M("f", 0, 2), M("g", 2, 3)]
    return none, recs


def across_chunks_records():
    rng = np.random.RandomState(41)
    recs = [R(rng, f"r{k}", t, 10 + k, "20M") for k, t in enumerate([0, 0, 1, 1, 1, 2, 2, 0])]
    recs.insert(5, unmapped(rng, "u", 10, tid=2, pos=3, flag=69))
    return recs


ALTERNATING_LENS = [100000, 100000, 3215]


def alternating(n):
    return [dict(qname=f"q{k}", flag=0, tid=1 - k % 2, pos=k, mapq=9, cigar="1M", mtid=-1, mpos=-1, isize=0, seq="A", qual=None) for k in range(n)]


def twelve():
    rng = np.random.RandomState(50)
    return [unmapped(rng, "u_first", 9), R(rng, "clip5", 1, 10, "3S9M", xc=1), R(rng, "plain", 1, 11, "11M", xc=1), unmapped(rng, "u_a", 7, flag=141), unmapped(rng, "u_b", 0),
            R(rng, "clip3", 2, 5, "8M4S", qual=False), R(rng, "mate_gone", 2, 6, "2S5M1D5M", flag=73), R(rng, "h", 2, 7, "2H10M"), R(rng, "back", 0, 3, "10M"),
            unmapped(rng, "star", 5, flag=0, tid=0, pos=4), R(rng, "both", 0, 5, "1S9M1S"), unmapped(rng, "u_last", 3, qual=False)]
