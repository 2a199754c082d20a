"""CPU: the Python model of `getsv -F` (tests/readthrough_model.py) against what the REAL reference printed, and the generator of
tests/test_readthrough_differential_gpu.py against the conditions that keep those GPU tests from passing on empty work.

Anchors: tests/golden/readthrough/small.json (the hand-made file of tests/readthrough_inputs.py) and model_anchor.json (generated safe samples),
both written by tests/golden/make_readthrough_reference.py.  After FindJunction the reference runs MergeJunction and then prints EVERY junction
that is left - to the .sv file or, with the filter that stopped it, to stdout (OutputBreakpoint, getsv.cpp:838-987).  So each printed row must be a
junction of model + fold, equal in the columns the -F pass decides, and a model junction without a row can only have gone in MergeJunction."""
import json
import os
from collections import Counter

import pytest

import readthrough_inputs as RT
import readthrough_model as M

GOLDEN = os.path.join(RT.GOLDEN, "readthrough")
FLANK = 50   # getsv -l, MergeJunction's search_length (seeksv.cpp:161)


def golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def printed_rows(entry):
    """every junction the reference printed: .sv rows and the rows stdout names with the filter they did not pass, as the columns of M.row_columns"""
    out = []
    for line in entry["sv"].splitlines():
        if line.startswith("@"):
            continue
        f = line.split("\t")
        assert len(f) == 23, line
        out.append(dict(key=(f[0], int(f[1]), f[2], f[4], int(f[5]), f[6]), left_support=int(f[3]), right_support=int(f[7]), microhomology=int(f[8]),
                        left_cigar=f[19], right_cigar=f[20], left_seq=f[21], right_seq=f[22], where="sv"))
    for line in entry["stdout"].splitlines():
        f = line.split("\t")   # OutputFilteredBreakpoint: reason, the .sv row's first eleven columns, two depths, two rates, CIGARs, seqs
        assert len(f) == 20, line
        f = f[1:]
        out.append(dict(key=(f[0], int(f[1]), f[2], f[4], int(f[5]), f[6]), left_support=int(f[3]), right_support=int(f[7]), microhomology=int(f[8]),
                        left_cigar=f[15], right_cigar=f[16], left_seq=f[17], right_seq=f[18], where="stdout"))
    return out


def merge_neighbours(key, keys):
    """the junctions MergeJunction can fold `key` into or fold into it (getsv.cpp:1355-1357): same contigs and strands, both positions within -l"""
    return [k for k in keys if k != key and (k[0], k[2], k[3], k[5]) == (key[0], key[2], key[3], key[5]) and abs(k[1] - key[1]) <= FLANK and abs(k[4] - key[4]) <= FLANK]


def hold_against_rows(jmap, entry, seeded=()):
    """every printed row is a model junction with equal columns; -> the model junctions without a row"""
    rows = printed_rows(entry)
    assert len(set(r["key"] for r in rows)) == len(rows)
    seen = set()
    for r in rows:
        assert r["key"] in jmap, f"the reference printed a junction the model does not have: {r}"
        c = M.row_columns(r["key"], jmap[r["key"]])
        for col in ("microhomology", "left_cigar", "right_cigar", "left_seq", "right_seq"):
            assert r[col] == c[col], (r["key"], col, r[col], c[col])
        if r["key"] not in seeded and not merge_neighbours(r["key"], jmap):
            # the two clip-read counts: the fold's insert-or-count rule (nothing merged into this row, no -B row under its key)
            assert (r["left_support"], r["right_support"]) == (c["left_support"], c["right_support"]), r["key"]
        seen.add(r["key"])
    return [k for k in jmap if k not in seen]


# ---- anchor 1: the committed hand-made file ----------------------------------------------------------------------------------------------------
SMALL_TAGS = (("default", 1, False), ("loose", 1, False), ("loose_w0", 0, False), ("loose_w20", 20, False), ("loose_B", 1, True), ("loose_B_w0", 0, True))


@pytest.mark.parametrize("tag,min_mapq,seeded", SMALL_TAGS, ids=[t[0] for t in SMALL_TAGS])
def test_small_file_equals_reference_rows(tag, min_mapq, seeded):
    batch, qnames = M.batch_from_records(RT.small_records())
    pairs, n_cand = M.find_junction([batch], [qnames], min_mapq, RT.NAMES)
    jmap = M.apply(pairs, M.seed_rows(RT.b_rows()) if seeded else None)
    seeds = set(M.seed_rows(RT.b_rows())) if seeded else set()
    left = hold_against_rows(jmap, golden("small")[tag], seeds)
    # near1 / near2 lie three bases apart on both sides, yet MergeJunction keeps both (their seqs are unrelated random bases: its similarity test,
    # >= 0.85, does not hold), and every other junction of this file is alone in its neighbourhood: the reference prints a row for each - no model
    # junction may be without one
    assert left == [], left
    assert len(pairs) >= 24 and n_cand > 2 * len(pairs)
    assert set(p["kind"] for p in pairs) == set(range(6))


def test_small_file_counting_rule():
    """multi1..4 (process_bwasw.cpp:198-216): four pairs on one junction, two of them with other seq lengths than the first"""
    batch, qnames = M.batch_from_records(RT.small_records())
    pairs, _ = M.find_junction([batch], [qnames], 1, RT.NAMES)
    key = ("chrB", 6050, "+", "chrA", 20001, "+")
    assert sum(1 for p in pairs if p["key"] == key) == 4
    e = M.apply(pairs)[key]
    assert (e["up"]["support"], e["down"]["support"]) == (0, 2)
    row = [r for r in printed_rows(golden("small")["loose"]) if r["key"] == key][0]
    assert (row["left_support"], row["right_support"]) == (0, 2)


def test_cigar_edits():
    """MinusCigarRight / AddCigarLeft (clip_reads.cpp:507-558)"""
    c = M.parse_cigar_text("40M3I7M2D")
    assert M.cigar_text(M.minus_cigar_right(c, 0)) == "40M3I7M"       # length 0 still drops what follows the last M / I
    assert M.cigar_text(M.minus_cigar_right(c, 7)) == "40M3I"         # >= : the operation that ends exactly there is kept whole
    assert M.cigar_text(M.minus_cigar_right(c, 8)) == "40M2I"
    assert M.cigar_text(M.minus_cigar_right(c, 50)) == "40M3I7M2D"    # nothing left: untouched (returns 0)
    assert M.cigar_text(M.minus_cigar_right(M.parse_cigar_text("5D10M4N6="), 3)) == "5D7M"   # = and X are not counted
    assert M.cigar_text(M.add_cigar_left(M.parse_cigar_text("10M2D"), 5)) == "15M2D"
    assert M.cigar_text(M.add_cigar_left(M.parse_cigar_text("10I2D"), 5)) == "5M10I2D"
    assert M.cigar_text(M.parse_cigar_text("10M"), 3, 4) == "3S10M4S"
    assert M.reverse_complement("ACGTNRY=acgt") == "tgca=YRNACGT"     # only upper-case A C G T change (GetSeq upper-cases the bases before)


# ---- anchor 2: generated safe samples through the real reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", M.ANCHOR_SEEDS)
def test_generated_samples_equal_reference_rows(seed):
    s = M.anchor_sample(seed)
    n = len(s["qnames"])
    for i in range(n):
        assert M.reference_undefined(s["batch"], i, len(s["contigs"]), s["qnames"][i]) is None, i
    w = golden("model_anchor")[str(seed)]
    assert w["records"] == n
    for tag, min_mapq in M.ANCHOR_RUNS:
        pairs, _ = M.find_junction([s["batch"]], [s["qnames"]], min_mapq, s["contigs"])
        jmap = M.apply(pairs)
        assert len(pairs) > 20
        for k in hold_against_rows(jmap, w[tag]):
            # no row: MergeJunction folded it into a neighbour (the only step between FindJunction and the printing that removes a junction)
            assert merge_neighbours(k, jmap), f"seed {seed} {tag}: {k} has no row and no junction near it to be merged into"


def test_safe_samples_reach_every_kind_of_input():
    kinds, n_ops, name_lens, times = Counter(), Counter(), Counter(), Counter()
    mh = {k: set() for k in range(6)}
    for seed in M.ANCHOR_SEEDS:
        s = M.anchor_sample(seed)
        pairs, _ = M.find_junction([s["batch"]], [s["qnames"]], 0, s["contigs"])
        cand = {r for p in pairs for r in p["records"]}
        for p in pairs:
            kinds[p["kind"]] += 1
            mh[p["kind"]].add(min(p["microhomology"], 2))
        for r in cand:
            n_ops[int(s["batch"]["n_cigar"][r])] += 1
            name_lens[len(s["qnames"][r])] += 1
        times.update(Counter(s["qnames"]).values())
    assert all(kinds[k] >= 10 for k in range(6)), kinds
    assert all(mh[k] == {0, 1, 2} for k in (0, 2, 4)), mh
    assert any(n > 64 for n in n_ops) and any(5 < n <= 64 for n in n_ops) and any(n > 100 for n in n_ops) and n_ops[1] and n_ops[2], n_ops
    assert name_lens[1] and name_lens[254], name_lens
    assert max(times) >= 20 and any(4 <= t <= 12 for t in times), times


# ---- the generator of the GPU tests ------------------------------------------------------------------------------------------------------------
GPU_SEEDS = tuple(range(48))


def sample_facts(seed):
    s = M.random_rt_sample(seed)
    n = len(s["qnames"])
    batches, names = M.split(s, s["cuts"])
    pairs, n_cand = M.find_junction(batches, names, 1, s["contigs"])
    return s, n, pairs, n_cand


@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_generator_caps_per_seed(seed):
    """conditions, not measurements: the GPU tests compare against this model's output, so the output must not be empty or one-sided"""
    s, n, pairs, n_cand = sample_facts(seed)
    assert 2700 <= n <= 3400
    assert n_cand >= 0.30 * n, (n_cand, n)
    assert 2 * len(pairs) >= 0.20 * n_cand, (len(pairs), n_cand)
    in_pair = Counter(s["qnames"][r] for p in pairs for r in p["records"])
    kept = Counter(s["qnames"][i] for i in range(n) if M.selected(s["batch"], i, 1, len(s["contigs"])))
    assert any(kept[q] > in_pair[q] for q in kept), "no record is dropped or left held"
    assert any(kept[q] == 4 and in_pair[q] == 4 for q in kept), "no name with four records and two pairs"
    bounds = [0] + s["cuts"] + [n]
    piece = lambda r: max(k for k in range(len(bounds) - 1) if bounds[k] <= r)  # noqa: E731
    assert any(piece(p["records"][0]) != piece(p["records"][1]) for p in pairs), "no pair across a batch cut"
    # cutting changes nothing in the model itself
    assert seed >= 8 or M.find_junction([s["batch"]], [s["qnames"]], 1, s["contigs"]) == (pairs, n_cand)


def test_generator_caps_over_the_seed_set():
    kinds = Counter()
    flags, mapqs, n_ops, lqs, last_ops, tids, name_lens = set(), set(), set(), set(), set(), set(), set()
    odd_even, base_codes, ties, big = set(), set(), 0, 0
    empty_reads, dropped_without_bases = set(), 0
    for seed in GPU_SEEDS[:12]:
        s, n, pairs, n_cand = sample_facts(seed)
        b = s["batch"]
        nt = len(s["contigs"])
        for p in pairs:
            kinds[(p["kind"], p["microhomology"] > 0)] += 1
            if p["kind"] >= 2 and p["key"][0] == p["key"][3] and p["key"][1] == p["key"][4] and p["microhomology"] == 0:
                ties += 1
            if p["kind"] in (2, 4):   # the reverse-complemented slices: where they start in the packed bases
                odd_even.add((p["kind"], len(p["down_seq"]) % 2))
            base_codes.update(p["up_seq"]); base_codes.update(p["down_seq"])
        for i in range(n):
            ops = M.record_ops(b, i)
            flags.add(int(b["flag"][i]) & (4 | 16 | 256 | 1024 | 2048)); mapqs.add(int(b["mapq"][i])); n_ops.add(len(ops)); lqs.add(int(b["l_qseq"][i]))
            t = int(b["tid"][i])
            tids.add("in" if 0 <= t < nt else ("-1" if t == -1 else ("nt" if t == nt else "beyond")))
            name_lens.add(len(s["qnames"][i]))
            if ops and ops[0][1] != M.S and M.selected(b, i, 0, nt):
                last_ops.add(ops[-1][1])
            no_seq = int(b["seq_off"][i]) == M.NO_SEQ
            if M.selected(b, i, 0, nt):
                assert not no_seq or int(b["l_qseq"][i]) <= 0, "a record that can be kept comes without bases"
                if int(b["l_qseq"][i]) == 0:
                    empty_reads.add(no_seq)
            elif no_seq:
                dropped_without_bases += 1
        big = max(big, max(Counter(s["qnames"]).values()))
    # kinds 1, 3, 5 are the branches with microhomology_length = 0 by construction (process_bwasw.cpp:125,164,189): only (kind, False) exists for them
    for k in range(6):
        assert kinds[(k, False)] >= 50, kinds
    for k in (0, 2, 4):
        assert kinds[(k, True)] >= 50, kinds
    assert ties >= 20
    assert odd_even == {(2, 0), (2, 1), (4, 0), (4, 1)}
    assert base_codes == set(M.NT16)
    assert {0, 1, 19, 20, 254, 255} <= mapqs
    assert {0, 1, 2, 5, 6, 64, 65, 130} <= n_ops
    assert {0, 1} <= lqs and any(l % 2 for l in lqs) and max(lqs) >= 1000
    assert empty_reads == {False, True} and dropped_without_bases >= 100   # l_qseq 0 with and without SSV_NO_SEQ among the kept; dropped records without bases
    assert last_ops == {M.M, M.I, M.D, M.N, M.S, M.P, M.EQ, M.X}
    assert tids == {"in", "-1", "nt", "beyond"}
    assert {1, 254} <= name_lens and big >= 300
    for f in (4, 16, 256, 1024, 2048, 16 | 256, 16 | 2048):
        assert f in flags, f
