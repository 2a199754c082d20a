"""The sample of tests/test_markdup_cli_gpu.py is what tests/markdup_cli_inputs.py says it is."""
import markdup_cli_inputs as CI
import markdup_model as mm


def clipped_at(recs, junction):
    (_, ja), _ = junction
    return [r for r in recs if "S" in r["cigar"] and r["tid"] == 0 and r["pos"] + int(r["cigar"].split("M")[0]) == ja + 1]


def test_sample():
    contigs, recs = CI.sample()
    recs = list(recs)
    assert 30000 < len(recs) < 60000 and mm.sorted_ok(recs) and not any(r["flag"] & 0x400 for r in recs)
    a, b = clipped_at(recs, CI.JUNCTION_A), clipped_at(recs, CI.JUNCTION_B)
    assert len(a) == 2 * (1 + CI.COPIES) and len(b) == 4
    assert len({(r["pos"], r["mpos"]) for r in a}) == 2 and len({(r["pos"], r["mpos"]) for r in b}) == 4
    # a clipped read is its contig up to the breakpoint and the other contig behind it
    for r, ((_, ja), (_, jb)) in [(a[0], CI.JUNCTION_A), (b[0], CI.JUNCTION_B)]:
        m = int(r["cigar"].split("M")[0])
        assert r["seq"] == contigs[0][ja + 1 - m:ja + 1] + contigs[1][jb:jb + 100 - m]
    flags = mm.mark(recs)
    marked = [r for r, f in zip(recs, flags) if f & 0x400]
    # the copies and their mates, nothing else: junction A keeps two clipped reads, junction B its four, the background everything
    assert len(marked) == 4 * CI.COPIES and all("copy" in r["qname"] for r in marked)
    assert sum(1 for r in marked if "S" in r["cigar"]) == 2 * CI.COPIES
    assert [r["flag"] for r in CI.flagged(tuple(recs))] == flags


def test_names_both_ends():
    assert CI.names_both_ends("tA\t20001\t+\ttB\t901\t+\n", CI.JUNCTION_A) and not CI.names_both_ends("tA\t20001\t+\ttB\t901\t+\n", CI.JUNCTION_B)


def test_where_the_seams_of_1_MB_chunks_fall():
    _, recs = CI.sample()
    ends = CI.record_ends(recs)
    batch = CI.batch_of(ends)
    assert batch[-1] >= 6                                                     # the file is seven chunks or more
    # inside junction A's first run: two of its four heads come out in the first batch, two in the second
    run_a = [i for i, r in enumerate(recs) if r["qname"].startswith("A0") and r["tid"] == 0]
    assert len(run_a) == 4 and run_a == list(range(run_a[0], run_a[0] + 4)) and len({recs[i]["pos"] for i in run_a}) == 1
    assert [batch[i] for i in run_a] == [0, 0, 1, 1]
    # the first record of tB is the last record of its batch: a run of one record, held back, and the contig change with it
    first_b = next(i for i, r in enumerate(recs) if r["tid"] == 1)
    assert batch[first_b] + 1 == batch[first_b + 1] and recs[first_b + 1]["pos"] != recs[first_b]["pos"] and batch[first_b - 1] == batch[first_b]
    # the pile: one place, no part in the marking, and one batch that holds nothing else
    pile = [i for i, r in enumerate(recs) if r["qname"].startswith("pile")]
    assert len(pile) == CI.PILE and pile == list(range(pile[0], pile[0] + CI.PILE)) and not any(mm.takes_part(recs[i]) for i in pile)
    assert len({(recs[i]["tid"], recs[i]["pos"]) for i in pile}) == 1 and not any(r["pos"] == CI.PILE_POS and r["tid"] == 1 for r in recs if not r["qname"].startswith("pile"))
    inside = [k for k in range(batch[-1] + 1) if k in batch and all(recs[i]["qname"].startswith("pile") for i in range(len(recs)) if batch[i] == k)]
    assert inside
