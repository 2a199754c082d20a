"""-m gpu: two-piece split alignments of whole reads (k_ra_query_t with its split hook on; ssv_realign_query_split; `seeksv realign -P`) against the model
of tests/realign_split_model.py: every field of every primary and mate, none exempt, on the hash index and on the sorted one.  Inputs:
tests/realign_split_inputs.py, held to their properties on the CPU in tests/test_realign_split_inputs.py.  End to end: getclip -> realign -P -> getsv -F
against what the real reference's getsv printed (tests/golden/realign_split)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bamio
import golden_util as G
import realign_model as M
import realign_sorted_model as SRT
import realign_split_inputs as SI
import realign_split_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEKSV = os.environ.get("SSV_CLI") or os.path.join(ROOT, "seeksv_amd", "bin", "seeksv")
E_ARG, E_STATE = -3, -4


@pytest.fixture(scope="module")
def ctx():
    from seeksv_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def index(ctx, contigs, max_occ=None):
    words, off = M.pack_2bit(contigs)
    return ctx.realign_index(words, off) if max_occ is None else ctx.realign_index_sorted(words, off, max_occ)


@functools.lru_cache(maxsize=None)
def model():
    return M.Reference(SI.reference())


@functools.lru_cache(maxsize=None)
def expected(max_occ):
    """the model's results on reference(), computed once per index and shared"""
    return tuple(SM.align_split(model(), s, max_occ) for s in SI.all_queries()[0])


def hit_dict(h):
    return dict({k: int(h[k]) for k in M.FIELDS}, flags=int(h["pad"][0]))


def compare(res, want, labels):
    """res = Context.realign_split(); want = [align_split()]: every field of the primary and of the mate, no query left out"""
    hits, mates = res
    assert len(hits) == len(mates) == len(want) and (hits["pad"][:, 1] == 0).all() and (mates["pad"][:, 1] == 0).all()
    bad = []
    for i, w in enumerate(want):
        p, m = hit_dict(hits[i]), hit_dict(mates[i])
        if p != w["primary"] or m != w["mate"]:
            bad.append((labels[i], (p, w["primary"]), (m, w["mate"])))
    for b in bad[:20]:
        print("kernel / model:", b)
    assert not bad, f"{len(bad)} of {len(want)} queries differ, (kernel, model): {bad[:3]}"


def test_error_codes_come_first():
    """(a context of its own) ssv_realign_query's errors, a NULL mates, n = 0"""
    from seeksv_amd import _abi
    from seeksv_amd.device import Context
    words, off = M.pack_2bit(SI.reference())
    with Context(0) as c:
        fn = c._lib.ssv_realign_query_split
        hits = np.zeros(1, dtype=np.dtype(_abi.REALIGN_HIT))
        mates = np.zeros(1, dtype=np.dtype(_abi.REALIGN_HIT))
        mates["score"] = -7
        qoff = np.array([0, 4], np.uint64)
        seq = C.c_char_p(b"ACGT")
        H, Mt, Q = hits.ctypes.data, mates.ctypes.data, qoff.ctypes.data
        assert fn(c._h, seq, Q, 1, H, Mt) == E_STATE
        assert fn(None, seq, Q, 1, H, Mt) == E_ARG
        assert c._lib.ssv_realign_index(c._h, words.ctypes.data, 0, int(off[-1]), off.ctypes.data, len(off) - 1, None) == 0
        assert fn(c._h, seq, Q, 1, H, None) == E_ARG
        assert fn(c._h, seq, Q, 1, None, Mt) == E_ARG
        assert fn(c._h, seq, Q, -1, H, Mt) == E_ARG
        assert fn(c._h, None, Q, 1, H, Mt) == E_ARG
        assert fn(c._h, seq, None, 1, H, Mt) == E_ARG
        assert fn(c._h, None, None, 0, None, None) == E_ARG
        assert int(mates["score"][0]) == -7                               # nothing was written by a refused call
        assert fn(c._h, None, None, 0, None, Mt) == 0 and int(mates["score"][0]) == -7
        assert fn(c._h, seq, Q, 1, H, Mt) == 0
        assert int(hits["tid"][0]) == -1 and mates.tobytes() == hits.tobytes()   # too short: both unaligned
        assert c._lib.ssv_realign_free(c._h) == 0
        assert fn(c._h, seq, Q, 1, H, Mt) == E_STATE


@pytest.mark.parametrize("max_occ", [None, SI.CAP], ids=["hash", "sorted"])
def test_every_field_of_every_query(ctx, max_occ):
    """the acceptance condition: the planted geometry, boundary, MAPQ and length cases in both orientations and ~2000 queries where split, unsplit,
    unaligned, too short and too long ones take turns; the primaries are the plain call's byte for byte wherever there is no mate, and in every field
    but second / mapq where there is one"""
    queries, labels = SI.all_queries()
    index(ctx, SI.reference(), max_occ)
    res = ctx.realign_split(list(queries))
    want = expected(max_occ)
    compare(res, want, labels)
    hits, mates = res
    assert sum(w["mate"]["tid"] >= 0 for w in want) > 500
    plain = ctx.realign(list(queries))
    none = mates["tid"] < 0
    assert none.any() and (~none).any() and hits[none].tobytes() == plain[none].tobytes()
    same = hits.copy()
    same["second"], same["mapq"] = plain["second"], plain["mapq"]
    assert same.tobytes() == plain.tobytes()
    assert (mates["tid"][none] == -1).all() and (mates["pos"][none] == -1).all() and all((mates[k][none] == 0).all() for k in M.FIELDS[2:])
    assert (mates["pad"][:, 0] == hits["pad"][:, 0]).all()


def test_n_is_zero_or_one(ctx):
    index(ctx, SI.reference())
    hits, mates = ctx.realign_split([])
    assert len(hits) == 0 and len(mates) == 0
    for s in (SI.read("mapq5050"), SI.read("own19"), SI.read("ff")[:25], "ACGT" * 257):
        compare(ctx.realign_split([s]), [SM.align_split(model(), s)], [s[:30]])


def test_flags_travel_with_the_mate(ctx):
    """the sorted index at a cap of 3: SSV_RA_F_OVERFLOW / SSV_RA_F_MASKED on the primary and in mates[].pad[0]"""
    q, lab = SI.flags_set()
    index(ctx, SI.reference(), SI.FLAGS_CAP)
    want = [SM.align_split(model(), s, SI.FLAGS_CAP) for s in q]
    compare(ctx.realign_split(list(q)), want, lab)
    assert {w["mate"]["flags"] for w in want} == {1, 2} and all(w["mate"]["tid"] >= 0 for w in want)


SETS = {"sweep": SI.sweep_set, "tandem": SI.tandem_set}


@pytest.mark.parametrize("max_occ", [None, SI.CAP], ids=["hash", "sorted"])
@pytest.mark.parametrize("name", list(SETS))
def test_more_candidates_than_lanes(ctx, name, max_occ):
    """sweep: the mate's slot is 64 or 128 behind the winner's, in the winner's lane.  tandem: 90 candidate diagonals, the mate among equals by the order"""
    contigs, queries, labels = SETS[name]()
    ref = M.Reference(contigs)
    index(ctx, contigs, max_occ)
    want = [SM.align_split(ref, s, max_occ) for s in queries]
    assert not any(w["overflow"] or w["tie"] for w in want) and all(w["mate"]["tid"] >= 0 for w in want)
    compare(ctx.realign_split(list(queries)), want, labels)


def read_seq_qual(path):
    """[(SEQ, QUAL as text)] of a small BAM file, in order (bamio.read_bam_records leaves these two out)"""
    import gzip
    import struct
    data = gzip.open(path, "rb").read()
    l_text, = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, p)
    p += 4
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", data, p)
        p += 4 + l + 4
    out = []
    while p < len(data):
        bs, _, _, l_rn, _, _, n_cig, _, l_seq = struct.unpack_from("<iiiBBHHHi", data, p)
        q = p + 36 + l_rn + 4 * n_cig
        seq = "".join("=ACMGRSVTWYHKDBN"[(data[q + (i >> 1)] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
        q += (l_seq + 1) // 2
        out.append((seq, "".join(chr(33 + x) for x in data[q:q + l_seq])))
        p += 4 + bs
    return out


def write_inputs(tmp_path, fq):
    fa, fq_path = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq")
    with open(fa, "w") as f:
        for name, c in zip(SI.NAMES, SI.reference()):
            f.write(f">{name}\n" + "\n".join(c[i:i + 60] for i in range(0, len(c), 60)) + "\n")
    with open(fq_path, "w") as f:
        for name, s, q in fq:
            f.write(f"@{name}\n{s}\n+\n{q}\n")
    return fa, fq_path


def summary(r):
    return [l for l in r.stderr.splitlines() if l.startswith("[seeksv realign]")]


@pytest.mark.parametrize("opts", [[], ["-c", str(SI.CAP)]], ids=["hash", "sorted"])
def test_cli_realign_P(tmp_path, opts):
    """`seeksv realign -P`: per read its record and, where it has one, the mate's supplementary record behind it, each the model's row (name, flag, tid, pos,
    MAPQ, CIGAR, SEQ, QUAL); the closing line counts them.  Without -P the output is what the parent wrote: one record per sequence named by the sequence,
    no flag 2048, the old closing line.  -P with -g or -S is refused"""
    fq = [e for e in SI.cli_set() if len(e[1]) <= 254]   # (without -P the sequence is the read name)
    max_occ = SI.CAP if opts else None
    fa, fq_path = write_inputs(tmp_path, fq)
    out = str(tmp_path / "reads.bam")
    r = subprocess.run([SEEKSV, "realign", "-P"] + opts + [fa, fq_path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names, recs = bamio.read_bam_records(out)
    want, n_al, n_split = [], 0, 0
    for name, s, q in fq:
        res = SM.align_split(model(), s, max_occ)
        rows = SM.bam_records(SI.cli_name(name), s, q, res)
        want += [(s, e) for e in rows]
        n_al += res["primary"]["tid"] >= 0
        n_split += len(rows) > 1
    assert names == list(SI.NAMES) and len(recs) == len(want) and n_split > 40
    for rec, sq, (s, e) in zip(recs, read_seq_qual(out), want):
        assert rec["qname"] == e["name"] and rec["l_qseq"] == len(s)
        assert (rec["flag"], rec["tid"], rec["pos"], rec["mapq"], rec["cigar"]) == (e["flag"], e["tid"], e["pos"], e["mapq"], e["cigar"]), (s, rec, e)
        assert sq == (e["seq"], e["qual"]), (s, sq, e)
    line = f"[seeksv realign] {len(fq)} clipped sequences, {n_al} aligned"
    tail = f", {n_split} split reads (mate pieces written)"
    last = summary(r)
    assert len(last) == 1 and last[0].startswith(line) and last[0].endswith(tail), (last, line, tail)
    # without -P: one record per sequence, named by the sequence, the primary's own fields apart from the MAPQ that the mate changes
    plain = str(tmp_path / "plain.bam")
    r = subprocess.run([SEEKSV, "realign"] + opts + [fa, fq_path, plain], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, precs = bamio.read_bam_records(plain)
    assert len(precs) == len(fq) and not any(rec["flag"] & 2048 for rec in precs) and "split" not in r.stderr
    assert summary(r) == [last[0][:-len(tail)]]
    for rec, (name, s, q) in zip(precs, fq):
        e = M.bam_record(s, q, M.align(model(), s) if max_occ is None else SRT.align_sorted(model(), s, max_occ))
        assert rec["qname"] == s and (rec["flag"], rec["tid"], rec["pos"], rec["mapq"], rec["cigar"]) == (e["flag"], e["tid"], e["pos"], e["mapq"], e["cigar"])
    for bad in (["-P", "-g"], ["-P", "-S", "2"], ["-g", "-P"], ["-S", "2", "-P"]):
        x = subprocess.run([SEEKSV, "realign"] + bad + [fa, fq_path, plain], capture_output=True, text=True)
        assert x.returncode == 1 and x.stderr.startswith("Usage: seeksv realign")
    assert "-P " in subprocess.run([SEEKSV, "realign"], capture_output=True, text=True).stderr
    assert subprocess.run([SEEKSV, "run", "-a", "-P", fq_path, fa, str(tmp_path / "x")], capture_output=True, text=True).returncode == 1   # (`seeksv run` has no -P)


def test_cli_getclip_realign_P_getsv_F_finds_the_junction(tmp_path):
    """pairs whose unmapped read crosses a planted inter-contig junction: `seeksv getclip` writes them to prefix.unmapped_2.fq.gz (the reference getclip's
    file, read for read), `seeksv realign -P` aligns them in two pieces, and `seeksv getsv -F` on that file prints the table the real reference's getsv
    printed from the model's records (tests/golden/realign_split), the planted junction in it; without -F the other golden, where it is not"""
    import gzip
    contigs, recs = SI.e2e_sample()
    bam, fa, pre = str(tmp_path / "s.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "s")
    bamio.write_bam(bam, list(SI.E2E_NAMES), list(SI.E2E_LENS), recs)
    with open(fa, "w") as f:
        for name, c in zip(SI.E2E_NAMES, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 70] for i in range(0, len(c), 70)) + "\n")

    def run(args):
        r = subprocess.run([SEEKSV] + args, capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stderr[-600:])
        return r
    run(["getclip", "-o", pre, bam])
    assert gzip.open(pre + ".unmapped_2.fq.gz", "rb").read() == gzip.open(os.path.join(G.GOLDEN, "realign_split", "e2e.unmapped_2.fq.gz"), "rb").read()
    run(["realign", fa, pre + ".clip.fq.gz", pre + ".clip.bam"])
    r = run(["realign", "-P", fa, pre + ".unmapped_2.fq.gz", pre + ".F.bam"])
    assert summary(r)[0].endswith(f", {SI.E2E_READS} split reads (mate pieces written)")
    _, frecs = bamio.read_bam_records(pre + ".F.bam")
    assert [x["flag"] & ~16 for x in frecs] == [0, 2048] * SI.E2E_READS and all(x["mapq"] == 60 for x in frecs) and frecs[0]["qname"] == frecs[1]["qname"] == "jn9/2"
    for tag, extra in (("e2e.F", ["-F", pre + ".F.bam"]), ("e2e", [])):
        sv = str(tmp_path / (tag + ".sv"))
        r = run(["getsv"] + list(SI.E2E_SV_OPTS) + extra + [pre + ".clip.bam", bam, pre + ".clip.gz", sv, str(tmp_path / (tag + ".u.fq"))])
        assert open(sv).read() == G.read_text("realign_split", tag + ".sv")
        assert r.stdout == G.read_text("realign_split", tag + ".stdout")
        assert (SI.e2e_names_both_ends(open(sv).read()) or SI.e2e_names_both_ends(r.stdout)) == (tag == "e2e.F")
