"""-m gpu: the split-read session with virtual candidates from SA tags (`seeksv run -A -S`: ssv_rt_begin_original_sa, seeksv_amd/csrc/splitread_sa_kernels.h)
against the plain model (tests/splitread_sa_model.py) and the answers written out in tests/splitread_sa_inputs.py: every field of every pair, the seqs, the
CIGAR sources, the six counts of the -A mode and the seven of this one - as one host batch with a host descriptor in both encodings, cut at every record,
through both device decoders and their descriptors, with the hashes cut to a few bits, with 70,000 contigs; the error sequence; which kernel groups run."""
import contextlib
import ctypes as C
import os

import pytest

import bamio
import sam_text as ST
import splitread_inputs as SI
import splitread_model as SM
import splitread_sa_inputs as SAI
import splitread_sa_model as SAM
from seeksv_amd import _abi, host
from seeksv_amd.device import Context, SeeksvError

pytestmark = pytest.mark.gpu

SETS = SAI.all_sets()
CASES = [(s, enc) for s in SETS for enc in s.get("encodings", (SAI.BAM, SAI.SAM))]
CASE_IDS = [f"{s['name']}-{'sam' if enc else 'bam'}" for s, enc in CASES]


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@contextlib.contextmanager
def environment(**values):
    saved = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def parts_of(records, cuts):
    bounds = [0] + list(cuts) + [len(records)]
    return [records[a:b] for a, b in zip(bounds, bounds[1:])]


def session(ctx, records, enc, cuts=(), min_mapq=1, contigs=SAI.CONTIGS):
    """the records as host batches cut at `cuts`, their optional fields as host descriptors -> (rows, the six counts, the seven counts)"""
    parts = parts_of(records, cuts)
    made = [SAI.batch_of(p) for p in parts]
    rows, stats, sa = ctx.readthrough_original_sa([b for b, _ in made], [n for _, n in made], [(enc, SAI.areas(p, enc)) for p in parts], min_mapq, contigs, raw=True)
    return rows, {k: stats[k] for k in SM.COUNTS}, sa


def model(records, enc, min_mapq=1, contigs=SAI.CONTIGS):
    b, names = SAI.batch_of(records)
    return SAM.find_pairs([b], [names], [(enc, SAI.areas(records, enc))], min_mapq, contigs)


def combined_records(enc, last=None):
    """all sets that have this encoding in one input, every name prefixed by its set's; last: the name of the bam_walk record that ends the input"""
    out = []
    for s in SETS:
        if enc in s.get("encodings", (SAI.BAM, SAI.SAM)) and s["name"] != "bam_walk":
            out += [dict(r, qname=s["name"] + "." + r["qname"]) for r in s["records"]]
    if enc == SAI.BAM:                                                           # the walk set last, and of it the record whose fields run into the record's end
        recs = [dict(r, qname="bam_walk." + r["qname"]) for r in SAI.bam_walk()["records"]]
        out += [r for r in recs if r["qname"] != "bam_walk." + last] + [r for r in recs if r["qname"] == "bam_walk." + last]
    return out


@pytest.fixture(scope="module")
def combined():
    """(records, the model's answer) per (encoding, last record): computed once"""
    out = {}
    for key in ((SAI.BAM, "truncated_Z"), (SAI.BAM, "overlong_B"), (SAI.SAM, None)):
        records = combined_records(*key)
        out[key] = (records, model(records, key[0]))
    return out


@pytest.mark.parametrize("s,enc", CASES, ids=CASE_IDS)
def test_set_as_one_host_batch(ctx, s, enc):
    rows, counts, sa = session(ctx, s["records"], enc)
    assert rows == s["rows"]
    assert counts == s["counts"] and sa == s["sa_counts"]


@pytest.mark.parametrize("s,enc", CASES, ids=CASE_IDS)
def test_set_cut_at_every_record(ctx, s, enc):
    """... the supplementary record one batch later than its primary among the cuts (real_partner's `late`)"""
    for cut in range(1, len(s["records"])):
        rows, counts, sa = session(ctx, s["records"], enc, [cut])
        assert rows == s["rows"], cut
        assert counts == s["counts"] and sa == s["sa_counts"], cut


def test_all_sets_in_one_input_and_in_pieces(ctx, combined):
    for key in ((SAI.BAM, "truncated_Z"), (SAI.SAM, None)):
        records, want = combined[key]
        n = len(records)
        for cuts in ([], [1], [n // 3, n // 3, 2 * n // 3], list(range(7, n, 7))):       # (an empty batch among them)
            assert session(ctx, records, key[0], cuts) == want, cuts


def test_mapq_floor(ctx):
    """-w 30: the grammar set's entries say 60 (stay), 0 and 12 ... against the model"""
    records = SAI.grammar()["records"] + [SAI.tagged(SAI.rec("q29", 0, 999, "60M40S", SAI.S), "chrB,5000,+,60S40M,29,0;"),
                                          SAI.tagged(SAI.rec("q30", 0, 999, "60M40S", SAI.S), "chrB,5000,+,60S40M,30,0;")]
    want = model(records, SAI.SAM, min_mapq=30)
    assert want[2]["sa_refused"] == SAI.grammar()["sa_counts"]["sa_refused"] + 1 and want[2]["pairs_from_sa"] == 6
    for enc in (SAI.BAM, SAI.SAM):
        assert session(ctx, records, enc, min_mapq=30) == want


def test_hashes_cut_to_a_few_bits(ctx, combined):
    """read names that share a hash run, and contig names that share a hash in the table: compared in full"""
    with environment(SSV_RT_HASH_BITS="4", SSV_SA_CONTIG_HASH_BITS="1"):
        for key in ((SAI.BAM, "truncated_Z"), (SAI.SAM, None)):
            records, want = combined[key]
            for cuts in ([], [len(records) // 2]):
                assert session(ctx, records, key[0], cuts) == want


def _fnv(name, bits):
    h = 1469598103934665603
    for ch in name.encode():
        h = ((h ^ ch) * 1099511628211) & (2 ** 64 - 1)
    return h & (2 ** bits - 1)


def test_seventy_thousand_contigs(ctx):
    """names only; a partner on tid 69,999 (above 65,535), and two partners whose names share a hash in the table (16 bits of it: found here, not assumed)"""
    contigs = [f"c{t}" for t in range(70000)]
    seen, pair = {}, None
    for t, name in enumerate(contigs):
        h = _fnv(name, 16)
        if h in seen:
            pair = (seen[h], t)
            break
        seen[h] = t
    assert pair and pair[0] != pair[1]
    records = [SAI.tagged(SAI.rec(f"big{k}", 0, 999, "60M40S", SAI.S), f"c{t},5000,+,60S40M,60,0;") for k, t in enumerate((69999, pair[0], pair[1], 65536))]
    records.append(SAI.tagged(SAI.rec("miss", 0, 999, "60M40S", SAI.S), "c70000,5000,+,60S40M,60,0;"))
    want = model(records, SAI.BAM, contigs=contigs)
    assert [r["key"][3] for r in want[0]] == ["c69999", f"c{pair[0]}", f"c{pair[1]}", "c65536"] and want[2]["sa_refused"] == 1
    with environment(SSV_SA_CONTIG_HASH_BITS="16"):
        assert session(ctx, records, SAI.BAM, contigs=contigs) == want
    assert session(ctx, records, SAI.SAM, [2], contigs=contigs) == want


# ---- through the device decoders and their descriptors ----
def decoded(ctx, records, decoder, n_batches, tmp_path, **text_form):
    """generator over (Batch, Names, Aux) of the records in n_batches pieces, through a device decoder in the form `seeksv run` decodes its input"""
    n = len(records)
    parts = [records[n * k // n_batches:n * (k + 1) // n_batches] for k in range(n_batches)]
    if decoder == "sam":
        whole = ST.text(records, SAI.CONTIGS, SAI.LENS, with_header=False, **text_form).encode("latin-1")
        lines = whole.splitlines(keepends=True)
        at = [0]
        for p in parts:
            at.append(at[-1] + len(p))
        texts = [b"".join(lines[a:b]) for a, b in zip(at, at[1:])]
        ctx.samdec_begin(SAI.CONTIGS)
        ctx.samdec_any_order(True)
        ctx.samdec_sorted(False)
        for k, t in enumerate(texts):
            yield ctx.samdec_decode(t, last=k == len(texts) - 1), ctx.samdec_names(), ctx.samdec_aux()
        return
    for k, part in enumerate(parts):
        path = str(tmp_path / f"part{k}.bam")
        bamio.write_bam(path, SAI.CONTIGS, SAI.LENS, part)
        with host.BamReader(path) as rd:
            for b, _ in ctx.bam_batches(rd, keep_all_seq=False, any_order=True):
                yield b, ctx.bamdec_names(), ctx.bamdec_aux()


def through(ctx, records, decoder, n_batches, tmp_path, **text_form):
    ctx.rt_begin_original_sa(1, SAI.CONTIGS)
    for b, nm, ax in decoded(ctx, records, decoder, n_batches, tmp_path, **text_form):
        assert ax.n == b.n
        ctx.rt_scan_aux(b, nm, ax)
    rows = ctx.rt_decode(ctx.rt_finish(), SAI.CONTIGS)
    stats = ctx.rt_original_stats()
    return rows, {k: stats[k] for k in SM.COUNTS}, ctx.rt_original_sa_stats()


@pytest.mark.parametrize("last", ["truncated_Z", "overlong_B"])
@pytest.mark.parametrize("n_batches", [1, 4])
def test_through_the_bam_decoder(ctx, combined, tmp_path, last, n_batches):
    """the LAST record of the last batch has a Z without its NUL / a B array that runs over the record's end: the inflated stream ends there"""
    records, want = combined[(SAI.BAM, last)]
    assert records[-1]["qname"] == "bam_walk." + last
    assert through(ctx, records, "bam", n_batches, tmp_path) == want


@pytest.mark.parametrize("text_form", [dict(), dict(crlf=True), dict(final_newline=False), dict(crlf=True, final_newline=False)], ids=["lf", "crlf", "no_final_newline", "crlf_no_final"])
@pytest.mark.parametrize("n_batches", [1, 4])
def test_through_the_sam_decoder(ctx, combined, tmp_path, text_form, n_batches):
    records, want = combined[(SAI.SAM, None)]
    assert through(ctx, records, "sam", n_batches, tmp_path, **text_form) == want


def test_both_decoders_give_the_same(ctx, tmp_path):
    """the same records as a BAM and as SAM text (the sets that have both encodings)"""
    records = [r for s in SETS if "encodings" not in s for r in (dict(r, qname=s["name"] + "." + r["qname"]) for r in s["records"])]
    a, b = through(ctx, records, "bam", 2, tmp_path), through(ctx, records, "sam", 3, tmp_path)
    assert a == b == model(records, SAI.BAM) and a[2]["pairs_from_sa"] > 10


# ---- sessions ----
def test_error_sequence(ctx):
    lib, h = ctx._lib, ctx._h
    s = SAI.other_contig()
    b, names = SAI.batch_of(s["records"])
    aux = (SAI.BAM, SAI.areas(s["records"], SAI.BAM))
    with Context(0) as fresh, pytest.raises(SeeksvError, match=r"\(-4\)"):
        fresh.rt_original_sa_stats()                                         # no session at all
    assert lib.ssv_rt_begin_original_sa(h, None, None) == -3
    p = _abi.RtParams(1, 2, None)
    assert lib.ssv_rt_begin_original_sa(h, C.byref(p), None) == -3            # contigs without their ranks
    ctx.rt_begin_original(1, SAI.CONTIGS)                                     # the plain -A mode: no descriptor calls, no SA counts
    with pytest.raises(SeeksvError, match=r"\(-4\)"):
        ctx.rt_scan_aux(b, names, aux)
    ctx.rt_scan(b, names)
    ctx.rt_finish()
    with pytest.raises(SeeksvError, match=r"\(-4\)"):
        ctx.rt_original_sa_stats()
    ctx.rt_begin_original_sa(1, SAI.CONTIGS)
    with pytest.raises(SeeksvError, match=r"\(-4\)"):
        ctx.rt_original_sa_stats()                                           # not finished yet
    with pytest.raises(SeeksvError, match=r"\(-4\)"):
        ctx.rt_scan(b, names)                                                # this mode's batches come with their descriptor
    for bad in ((SAI.BAM, aux[1][:-1]), (2, aux[1])):                        # a descriptor of another batch; no encoding
        with pytest.raises(SeeksvError, match=r"\(-3\)"):
            ctx.rt_scan_aux(b, names, bad)
    a, keep = ctx._as_aux(aux)
    a.bytes -= 1                                                             # the last record's span ends outside
    with pytest.raises(SeeksvError, match=r"\(-3\)"):
        ctx.rt_scan_aux(b, names, a)
    ctx.rt_scan_aux(b, names, aux)                                           # the refused calls left the session as it was
    r = ctx.rt_finish()
    assert r.n_pairs == 3 and r.n_candidates == 4 and ctx.rt_original_sa_stats() == s["sa_counts"] == ctx.rt_original_sa_stats()
    assert lib.ssv_rt_original_sa_stats(h, None) == -3
    with pytest.raises(SeeksvError, match=r"\(-4\)"):
        ctx.rt_scan_aux(b, names, aux)                                       # the session is over
    ctx.rt_begin_original_sa(1, SAI.CONTIGS)                                  # a new session takes the counts away
    with pytest.raises(SeeksvError, match=r"\(-4\)"):
        ctx.rt_original_sa_stats()
    r = ctx.rt_finish()                                                      # an empty session
    assert r.n_pairs == 0 and r.n_candidates == 0 and ctx.rt_original_sa_stats() == dict.fromkeys(SAM.SA_COUNTS, 0)


def test_other_modes_afterwards_give_their_old_results(ctx):
    """the -F mode and the plain -A mode on the same context, behind a session of this mode"""
    s = SAI.real_partner()
    session(ctx, s["records"], SAI.BAM)
    b, names = SAI.batch_of(s["records"])
    rows, stats = ctx.readthrough_original([b], [names], 1, SAI.CONTIGS, raw=True)
    assert (rows, {k: stats[k] for k in SM.COUNTS}) == SM.find_pairs([b], [names], 1, SAI.CONTIGS) and len(rows) == 2
    import readthrough_model as RM
    want, n_cand = RM.find_junction([b], [names], 1, SAI.CONTIGS)
    assert ctx.readthrough([b], [names], 1, SAI.CONTIGS, raw=True) == (want, n_cand)


def test_each_mode_runs_its_own_groups(ctx, tmp_path):
    s = SAI.kinds_slice()
    b, names = SAI.batch_of(s["records"])
    new, old = ("splitread_sa_aux", "splitread_sa_scan", "splitread_sa_finish"), ("splitread_scan", "splitread_finish", "rt_scan", "rt_finish")
    ctx.prof_enable(1)
    ctx.prof_reset()
    ctx.readthrough_original([b], [names], 1, SAI.CONTIGS)
    ctx.readthrough([b], [names], 1, SAI.CONTIGS)
    assert [ctx.prof_get(g)["launches"] for g in old] == [1, 1, 1, 1] and [ctx.prof_get(g)["launches"] for g in new] == [0, 0, 0]
    ctx.prof_reset()
    session(ctx, s["records"], SAI.BAM, [3])
    assert [ctx.prof_get(g)["launches"] for g in new] == [0, 2, 1] and [ctx.prof_get(g)["launches"] for g in old] == [0, 0, 0, 0]
    ctx.prof_reset()
    through(ctx, s["records"], "sam", 2, tmp_path)
    assert [ctx.prof_get(g)["launches"] for g in new] == [2, 2, 1] and [ctx.prof_get(g)["launches"] for g in old] == [0, 0, 0, 0]
    ctx.prof_enable(0)
