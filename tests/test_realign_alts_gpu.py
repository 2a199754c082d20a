"""-m gpu: the re-aligner's alternate loci (k_ra_query_t with its alternates on, the scan, k_ra_alt_compact; ssv_realign_query_alts; `seeksv realign -S`;
`seeksv run -a "-S INT"`) against the model of tests/realign_alts_model.py: every field of every primary, gap, offset and alternate, none exempt, on the
hash index and on the sorted one, ungapped and gapped.  Inputs: tests/realign_alts_inputs.py (held to their properties on the CPU in
tests/test_realign_alts_inputs.py) and the sets of tests/realign_inputs.py with more candidates than lanes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bamio
import golden_util as G
import realign_alts_inputs as AI
import realign_alts_model as AM
import realign_gapped_model as GM
import realign_inputs as I
import realign_model as M

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
    return M.Reference(AI.reference())


@functools.lru_cache(maxsize=None)
def expected(max_occ, gapped, max_alt):
    """the model's results, computed once per configuration and shared"""
    return tuple(AM.align_alts(model(), s, max_alt, max_occ, gapped) for s in AI.all_queries()[0])


def hit_dict(h):
    return dict({k: int(h[k]) for k in M.FIELDS}, flags=int(h["pad"][0]))


def compare(res, want, labels, gapped):
    """res = Context.realign_alts(); want = [align_alts()]: the primary, its gap, the offsets and every alternate, no query left out"""
    hits, gaps, alt_off, alts = res
    assert len(hits) == len(want) and alt_off.shape == (len(want) + 1,) and int(alt_off[0]) == 0 and len(alts) == int(alt_off[-1])
    assert (np.diff(alt_off) >= 0).all() and (hits["pad"][:, 1] == 0).all() and (len(alts) == 0 or (alts["pad"][:, 1] == 0).all())
    bad = []
    for i, w in enumerate(want):
        got = hit_dict(hits[i])
        if gapped:
            got.update(gap_at=int(gaps["q_at"][i]), gap_len=int(gaps["len"][i]))
        diff = {k: (got[k], w["primary"][k]) for k in got if got[k] != w["primary"][k]}
        mine = [hit_dict(a) for a in alts[int(alt_off[i]):int(alt_off[i + 1])]]
        if mine != w["alts"]:
            diff["alts"] = (mine, w["alts"])
        if diff:
            bad.append((labels[i], diff))
    for b in bad[:20]:
        print("kernel / model:", b)
    assert not bad, f"{len(bad)} of {len(want)} queries differ, (kernel, model): {bad[:4]}"


def test_error_codes_come_first():
    """(a context of its own) the query calls' errors, and: max_alt outside 1..16, no alt_off, no alts, gapped without gaps; n = 0 writes alt_off[0]"""
    from seeksv_amd import _abi
    from seeksv_amd.device import Context
    words, off = M.pack_2bit(AI.reference())
    with Context(0) as c:
        fn = c._lib.ssv_realign_query_alts
        hits = np.zeros(1, dtype=np.dtype(_abi.REALIGN_HIT))
        alts = np.zeros(16, dtype=np.dtype(_abi.REALIGN_HIT))
        gaps = np.zeros(1, dtype=np.dtype(_abi.REALIGN_GAP))
        aoff = np.full(2, -7, np.int64)
        qoff = np.array([0, 4], np.uint64)
        seq = C.c_char_p(b"ACGT")
        H, A, O, Gp, Q = hits.ctypes.data, alts.ctypes.data, aoff.ctypes.data, gaps.ctypes.data, qoff.ctypes.data
        assert fn(c._h, seq, Q, 1, 8, 0, H, None, O, A) == E_STATE
        assert fn(None, seq, Q, 1, 8, 0, H, None, O, A) == E_ARG
        assert c._lib.ssv_realign_index(c._h, words.ctypes.data, 0, int(off[-1]), off.ctypes.data, len(off) - 1, None) == 0
        for max_alt in (0, -1, 17):
            assert fn(c._h, seq, Q, 1, max_alt, 0, H, None, O, A) == E_ARG
        assert fn(c._h, seq, Q, 1, 8, 0, H, None, None, A) == E_ARG
        assert fn(c._h, seq, Q, 1, 8, 0, H, None, O, None) == E_ARG
        assert fn(c._h, seq, Q, 1, 8, 1, H, None, O, A) == E_ARG          # gapped without gaps
        assert fn(c._h, seq, Q, -1, 8, 0, H, None, O, A) == E_ARG
        assert fn(c._h, None, Q, 1, 8, 0, H, None, O, A) == E_ARG
        assert fn(c._h, seq, None, 1, 8, 0, H, None, O, A) == E_ARG
        assert fn(c._h, seq, Q, 1, 8, 0, None, None, O, A) == E_ARG
        assert int(aoff[0]) == -7                                         # nothing was written by a refused call
        assert fn(c._h, None, None, 0, 8, 0, None, None, O, A) == 0 and int(aoff[0]) == 0 and int(aoff[1]) == -7
        aoff[:] = -7
        assert fn(c._h, seq, Q, 1, 16, 1, H, Gp, O, A) == 0
        assert int(hits["tid"][0]) == -1 and list(aoff) == [0, 0] and int(gaps["len"][0]) == 0
        assert c._lib.ssv_realign_free(c._h) == 0
        assert fn(c._h, seq, Q, 1, 8, 0, H, None, O, A) == E_STATE
        assert _abi.RA_F_ALT_CUT == AM.F_ALT_CUT == 4


@pytest.mark.parametrize("gapped", [False, True], ids=["ungapped", "gapped"])
@pytest.mark.parametrize("max_occ", [None, AI.CAP], ids=["hash", "sorted"])
def test_every_field_of_every_query(ctx, max_occ, gapped):
    """the acceptance condition, max_alt 8: more queries than a tile of the scan, with and without alternates in turn, unaligned / too short / too long
    ones between them; and the primaries are the plain calls', bit for bit, apart from SSV_RA_F_ALT_CUT"""
    queries, labels = AI.all_queries()
    index(ctx, AI.reference(), max_occ)
    res = ctx.realign_alts(list(queries), 8, gapped=gapped)
    want = expected(max_occ, gapped, 8)
    compare(res, want, labels, gapped)
    assert sum(len(w["alts"]) > 0 for w in want) > 80 and any(w["primary"]["flags"] & AM.F_ALT_CUT for w in want)
    plain = ctx.realign(list(queries), gapped=gapped)
    hits = res[0].copy()
    hits["pad"][:, 0] &= ~np.uint8(AM.F_ALT_CUT)
    if gapped:
        assert (plain[1] == res[1]).all()
        plain = plain[0]
    assert hits.tobytes() == plain.tobytes()
    assert (plain["pad"][:, 0] & AM.F_ALT_CUT == 0).all()


@pytest.mark.parametrize("max_alt", [1, 2, 16])
@pytest.mark.parametrize("max_occ", [None, AI.CAP], ids=["hash", "sorted"])
def test_max_alt(ctx, max_occ, max_alt):
    """which loci are kept and the flag, at max_alt 1, 2 and 16 (the family has 17): the sets without the mix"""
    q, lab = AI.all_queries()
    n = sum(len(fn()[0]) for name, fn in AI.SETS.items() if name != "gapped")
    index(ctx, AI.reference(), max_occ)
    want = [AM.align_alts(model(), s, max_alt, max_occ) for s in q[:n]]
    compare(ctx.realign_alts(list(q[:n]), max_alt), want, lab[:n], False)
    assert sum(bool(w["primary"]["flags"] & AM.F_ALT_CUT) for w in want) >= 2 and max(len(w["alts"]) for w in want) == max_alt


def test_n_is_zero_or_one(ctx):
    index(ctx, AI.reference())
    hits, gaps, alt_off, alts = ctx.realign_alts([], 8)
    assert len(hits) == 0 and gaps is None and list(alt_off) == [0] and len(alts) == 0
    for s in (AI.element("family"), AI.element("family")[:25], AI.reference()[0][40:100]):
        compare(ctx.realign_alts([s], 16, gapped=True), [AM.align_alts(model(), s, 16, None, True)], [s], True)


def test_flags_travel_with_the_alternates(ctx):
    """the sorted index at a cap of 3: SSV_RA_F_OVERFLOW / SSV_RA_F_MASKED on the primary and on its alternates"""
    q, lab = AI.flags_set()
    index(ctx, AI.reference(), AI.FLAGS_CAP)
    want = [AM.align_alts(model(), s, 16, AI.FLAGS_CAP) for s in q]
    compare(ctx.realign_alts(list(q), 16), want, lab, False)
    assert {w["primary"]["flags"] for w in want} >= {1, 2} and all(w["alts"] for w in want)


SETS = {"sweep": I.sweep_set, "tandem": I.tandem_set, "two-locus": I.two_locus_set}


@pytest.mark.parametrize("max_occ", [None, AI.CAP], ids=["hash", "sorted"])
@pytest.mark.parametrize("name", list(SETS))
def test_more_candidates_than_lanes(ctx, name, max_occ):
    """sweep: the alternate is a candidate the winner's lane scored in another round (slots 0 and 64).  tandem: up to 90 diagonals 36 apart, more
    loci than 16.  two-locus: copies with 0-3 mismatches on either strand, partial copies at a contig's end, two diagonals in and outside one locus"""
    contigs, queries, labels = SETS[name]()
    ref = M.Reference(contigs)
    index(ctx, contigs, max_occ)
    want = [AM.align_alts(ref, s, 16, max_occ) for s in queries]
    assert not any(w["overflow"] or w["tie"] for w in want)
    compare(ctx.realign_alts(list(queries), 16), want, labels, False)
    if name == "tandem":
        assert sum(len(w["alts"]) == 16 for w in want) > 50


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


def write_inputs(tmp_path, names, contigs, fq):
    fa, fq_path = str(tmp_path / "ref.fa"), str(tmp_path / "s.clip.fq")
    with open(fa, "w") as f:
        for name, c in zip(names, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 60] for i in range(0, len(c), 60)) + "\n")
    with open(fq_path, "w") as f:
        for i, (s, q) in enumerate(fq):
            f.write(f"@clip{i}\n{s}\n+\n{q}\n")
    return fa, fq_path


@pytest.mark.parametrize("opts", [["-S", "8"], ["-c", str(AI.CAP), "-g", "-S", "3"]], ids=["hash", "sorted-gapped"])
def test_cli_realign_S(tmp_path, opts):
    """`seeksv realign -S`: behind every sequence's record its alternates as secondary records, each the model's row (flag, tid, pos, MAPQ, CIGAR, SEQ, QUAL);
    the closing line counts them.  Without -S the output is the one it was: one record per sequence, no flag 256, the old closing line"""
    fq = AI.cli_set()
    gapped, max_alt = "-g" in opts, int(opts[-1])
    max_occ = AI.CAP if "-c" in opts else None
    fa, fq_path = write_inputs(tmp_path, AI.NAMES, AI.reference(), fq)
    out = str(tmp_path / "s.clip.bam")
    r = subprocess.run([SEEKSV, "realign"] + opts + [fa, fq_path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names, recs = bamio.read_bam_records(out)
    want, n_al, n_gap, n_with, n_cut = [], 0, 0, 0, 0
    for s, q in fq:
        res = AM.align_alts(model(), s, max_alt, max_occ, gapped)
        rows = AM.bam_records(s, q, res, gapped)
        want += [(s, e) for e in rows]
        n_al += res["primary"]["tid"] >= 0
        n_gap += any(op in "ID" for _, op in rows[0]["cigar"])
        n_with += len(rows) > 1
        n_cut += bool(res["primary"]["flags"] & AM.F_ALT_CUT)
    assert names == list(AI.NAMES) and len(recs) == len(want) > len(fq) + 40
    for rec, sq, (s, e) in zip(recs, read_seq_qual(out), want):
        assert rec["qname"] == s and rec["l_qseq"] == len(s)
        assert (rec["flag"], rec["tid"], rec["pos"], rec["mapq"], rec["cigar"]) == (e["flag"], e["tid"], e["pos"], e["mapq"], e["cigar"]), (s, rec, e)
        assert sq == (e["seq"], e["qual"]), (s, sq, e)
    n_sec = len(want) - len(fq)
    line = f"[seeksv realign] {len(fq)} clipped sequences, {n_al} aligned" + (f", {n_gap} with a gap" if gapped else "")
    tail = f", {n_sec} secondary records for {n_with} sequences ({n_cut} cut at -S)"
    last = [l for l in r.stderr.splitlines() if l.startswith("[seeksv realign]")]
    assert len(last) == 1 and last[0].startswith(line) and last[0].endswith(tail) and n_cut > 0, (last, line, tail)
    # the sequences a piece at a time (37 of them, then the default: all at once): the same file, byte for byte, and the same closing line
    pieces = str(tmp_path / "pieces.clip.bam")
    r2 = subprocess.run([SEEKSV, "realign"] + opts + [fa, fq_path, pieces], capture_output=True, text=True, env=dict(os.environ, SSV_REALIGN_ALT_PIECE="37"))
    assert r2.returncode == 0, r2.stderr
    assert open(pieces, "rb").read() == open(out, "rb").read() and [l for l in r2.stderr.splitlines() if l.startswith("[seeksv realign]")] == last
    # without -S: one record per sequence, every one the primary above in every field, SEQ and QUAL included; the closing line is the one above without its tail
    plain = str(tmp_path / "p.clip.bam")
    r = subprocess.run([SEEKSV, "realign"] + opts[:-2] + [fa, fq_path, plain], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, precs = bamio.read_bam_records(plain)
    assert len(precs) == len(fq) and not any(rec["flag"] & 256 for rec in precs) and "secondary" not in r.stderr
    first = [i for i, rec in enumerate(recs) if not rec["flag"] & 256]
    assert [recs[i] for i in first] == precs
    sq = read_seq_qual(out)
    assert [sq[i] for i in first] == read_seq_qual(plain)
    assert [l for l in r.stderr.splitlines() if l.startswith("[seeksv realign]")] == [last[0][:-len(tail)]]
    if not gapped and max_occ is None:
        assert last[0] == line + tail   # (the hash index on this reference drops nothing: the whole line is known)
    for bad in (["-S", "0"], ["-S", "17"], ["-S", "x"]):
        assert subprocess.run([SEEKSV, "realign"] + bad + [fa, fq_path, plain], capture_output=True, text=True).returncode == 1
    assert "-S " in subprocess.run([SEEKSV, "realign"], capture_output=True, text=True).stderr


def test_cli_run_S_finds_the_copy_the_reads_came_from(tmp_path):
    """`seeksv run -a "-c 500 -S 8"` on the sample whose breakpoint's far side lies in copy 3 of a 5-copy element: table and stdout are the ones the real
    reference's getsv makes from the model's records with the secondary ones (tests/golden/realign_alts), and the planted junction is among them;
    without -S they are the ones it makes from the primaries alone, where the junction points at copy 1 only"""
    contigs, recs = AI.e2e_sample()
    bam, fa = str(tmp_path / "s.bam"), str(tmp_path / "ref.fa")
    bamio.write_bam(bam, list(AI.E2E_NAMES), list(AI.E2E_LENS), recs)
    with open(fa, "w") as f:
        for name, c in zip(AI.E2E_NAMES, contigs):
            f.write(f">{name}\n" + "\n".join(c[i:i + 70] for i in range(0, len(c), 70)) + "\n")
    planted = ("tA", str(AI.E2E_A + 1), "tB", str(AI.E2E_B + 1))

    def names_both_ends(text):
        for l in text.splitlines():
            f = l.split("\t")
            pairs = set(zip(f, f[1:]))
            if planted[:2] in pairs and planted[2:] in pairs:
                return True
        return False

    for tag, aln in (("e2e", f"-c {AI.CAP} -S 8"), ("e2e.primary", f"-c {AI.CAP}")):
        pre = str(tmp_path / tag)
        r = subprocess.run([SEEKSV, "run"] + (["-v", " ".join(AI.E2E_SV_OPTS)] if AI.E2E_SV_OPTS else []) + ["-a", aln, bam, fa, pre], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert open(pre + ".sv.txt").read() == G.read_text("realign_alts", tag + ".sv")
        assert r.stdout == G.read_text("realign_alts", tag + ".stdout")
        seen = names_both_ends(open(pre + ".sv.txt").read()) or names_both_ends(r.stdout)
        summary = [l for l in r.stderr.splitlines() if l.startswith("[seeksv realign]")]
        if tag == "e2e":
            assert seen and summary and summary[0].endswith(", 4 secondary records for 1 sequences (0 cut at -S)")
        else:
            assert not seen and summary and "secondary" not in summary[0]
