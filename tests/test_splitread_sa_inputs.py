"""CPU: the hand-made sets of tests/splitread_sa_inputs.py held to their claims by the plain model (tests/splitread_sa_model.py), and the model held to
tests/splitread_model.py where the two must agree: on a complete file the tag mode changes nothing, and with the supplementary records removed the
junctions are the complete file's."""
import pytest

import splitread_inputs as SI
import splitread_model as SM
import splitread_sa_inputs as SAI
import splitread_sa_model as SAM

SETS = SAI.all_sets()
IDS = [s["name"] for s in SETS]
CASES = [(s, enc) for s in SETS for enc in s.get("encodings", (SAI.BAM, SAI.SAM))]
CASE_IDS = [f"{s['name']}-{'sam' if enc else 'bam'}" for s, enc in CASES]


def model(records, enc, cuts=(), min_mapq=1):
    bounds = [0] + list(cuts) + [len(records)]
    parts = [records[a:b] for a, b in zip(bounds, bounds[1:])]
    made = [SAI.batch_of(p) for p in parts]
    return SAM.find_pairs([b for b, _ in made], [n for _, n in made], [(enc, SAI.areas(p, enc)) for p in parts], min_mapq, SAI.CONTIGS)


def junctions(rows):
    return [{k: v for k, v in r.items() if k != "records"} for r in rows]


@pytest.mark.parametrize("s,enc", CASES, ids=CASE_IDS)
def test_set_gives_what_is_written_out(s, enc):
    rows, counts, sa = model(s["records"], enc)
    assert rows == s["rows"]
    assert counts == s["counts"] and sa == s["sa_counts"]
    assert sa["sa_tags"] == sa["sa_multi"] + sa["sa_refused"] + sa["virtuals"]
    assert sa["virtuals"] >= sa["sa_redundant"] + sa["pairs_from_sa"] + sa["sa_dropped_length"]


@pytest.mark.parametrize("s,enc", CASES, ids=CASE_IDS)
def test_model_does_not_depend_on_the_cut(s, enc):
    want = model(s["records"], enc)
    for cut in range(1, len(s["records"])):
        assert model(s["records"], enc, [cut]) == want, cut


@pytest.mark.parametrize("enc", [SAI.BAM, SAI.SAM])
def test_complete_file_is_what_the_plain_rule_gives(enc):
    """every primary has its supplementary: the pairs are splitread_model.find_pairs' exactly, every virtual candidate is redundant"""
    for s in (SAI.kinds_complete(), dict(records=SI.combined(file_form=True)[0])):
        b, names = SAI.batch_of(s["records"])
        rows, counts, sa = model(s["records"], enc)
        assert (rows, counts) == SM.find_pairs([b], [names], 1, SAI.CONTIGS)
        assert sa["virtuals"] == sa["sa_redundant"] == sa["sa_tags"] and sa["pairs_from_sa"] == 0
    assert sa["sa_tags"] == 0 and SAI.kinds_complete()["sa_counts"]["virtuals"] == 6        # (splitread_inputs' records carry no tags)


@pytest.mark.parametrize("enc", [SAI.BAM, SAI.SAM])
def test_supplementary_records_removed_gives_the_complete_files_junctions(enc):
    full, cut = SAI.kinds_complete(), SAI.kinds_slice()
    assert cut["records"] == [r for r in full["records"] if not r["flag"] & SI.SUPP]
    got, want = model(cut["records"], enc)[0], model(full["records"], enc)[0]
    assert len(got) == 6 and junctions(got) == junctions(want)
    for g, r in zip(got, cut["records"]):                                                     # source and virtual candidate share the record index
        assert g["records"][0] == g["records"][1] == cut["records"].index(r)


def test_equal_position_is_stated_apart():
    """the documented order-dependent case: the completing record is up - the virtual candidate always completes, a supplementary record in front of its
    primary does not"""
    s = SAI.equal_position()
    primary = s["records"][0]
    supp = SAI.rec("eq", SI.SUPP | SI.REV, 1019, "40M60H", SAI.RC[:40])
    assert SAI.entry_of(supp) == "chrB,1020,-,40M60S,60,0;"
    virtual = model([primary], SAI.BAM)[0]
    after = model([primary, supp], SAI.BAM)[0]
    before = model([supp, primary], SAI.BAM)[0]
    assert junctions(virtual) == junctions(s["rows"]) == junctions(after) != junctions(before)


def test_walkers_find_what_the_sets_say():
    for name, aux, found in SAI.BAM_WALK:
        assert (SAM.find_bam(aux) is not None) == found, name
    for name, tags, found in SAI.SAM_WALK:
        area = "\t".join(tags).encode()
        for tail in (b"", b"\n", b"\r\n", b"\nnext\tSA:Z:chrA,1,+,60S40M,60,0;"):
            assert (SAM.find_sam(area + tail) is not None) == found, (name, tail)
            if found:
                assert SAM.find_sam(area + tail) == b"chrB,5000,+,60S40M,60,0;", (name, tail)


def test_grammar_cases_one_by_one():
    src = dict(rec=0, key=(b"q", 0))
    for name, value, want in SAI.GRAMMAR:
        status, v = SAM.virtual_of(src, value.encode(), 1, SAI.CONTIGS)
        if want in ("multi", "refused"):
            assert status == want and v is None, name
        else:
            assert status == "ok" and v["R"] == (90 if want == "length" else 100) and v["side"] == "5" and v["pos"] == 5000 and not v["carries"], name
            assert v["tid"] == (0 if want == "length" else want), name
    assert SAM.virtual_of(src, b"chrB,5000,+,60S40M,29,0;", 30, SAI.CONTIGS)[0] == "refused"   # the -w floor
    assert SAM.virtual_of(src, b"chrB,5000,+,60S40M,30,0;", 30, SAI.CONTIGS)[0] == "ok"
