"""-m "not gpu": every property tests/test_samdec_sorted_gpu.py claims of its input sets (tests/original_sam_inputs.py), and of the text tests/original_sam.py
makes of a BAM - without a GPU."""
import os

import bamio
import golden_util as G
import original_sam
import original_sam_inputs as I
import sam_text as ST


def fields(r):
    return ST.line(r, I.NAMES).split("\t")


def test_shipping_records():
    recs = I.shipping_records()
    by = {r["qname"]: r for r in recs}
    assert len(by) == len(recs)
    assert {q: I.ships(r) for q, r in by.items()} == dict(s_first=True, s_last=True, s_both=True, h_s_m=False, s_h_last=False, only_s=True, plain=False, plain_odd=False,
                                                         s_odd=True, s_even=True, star=False, seq_star=False, mid_s_only=False, eq_x=True, s1=True)
    ops = {q: "".join(op for _, op in I.cigar_ops(r)) for q, r in by.items()}
    assert ops["s_first"] == "SM" and ops["s_last"] == "MS" and ops["s_both"] == "SMS" and ops["h_s_m"] == "HSM" and ops["s_h_last"] == "MSH" and ops["only_s"] == "S"
    assert fields(by["only_s"])[5] == "50S" and fields(by["star"])[5] == "*" and fields(by["seq_star"])[9:11] == ["*", "*"] and fields(by["seq_star"])[5] == "3S7M"
    assert len(by["s_odd"]["seq"]) % 2 == 1 and len(by["s_even"]["seq"]) % 2 == 0 and by["s_odd"]["qual"] is None and fields(by["s_odd"])[10] == "*"
    assert len(by["plain_odd"]["seq"]) % 2 == 1 and len(by["s1"]["seq"]) == 2
    # XC on lines that ship (zero and non-zero) and on lines that do not: only s_last and s_even keep it
    assert {q: r["xc"] for q, r in by.items() if "xc" in r} == dict(s_last=1, s_both=0, h_s_m=3, plain=5, s_even=100)
    assert all(any(f.startswith("XC:i:") for f in fields(r)) == ("xc" in r) for r in recs)
    assert by["star"]["flag"] == 0 and I.side_channel(by["star"])   # the flag as decoded has UNMAP
    for r in recs:   # text can say every record: CIGAR and SEQ agree where both are given
        if I.cigar_ops(r) and r["seq"]:
            assert sum(l for l, op in I.cigar_ops(r) if op in "MIS=X") == len(r["seq"])


def test_long_read_records():
    recs = I.long_read_records()
    long_ = [r for r in recs if len(r["seq"]) >= 19999]
    assert [len(r["seq"]) for r in long_] == [20000, 19999] and all(I.ships(r) for r in long_) and long_[1]["qual"] is None
    assert all(len(r["seq"]) == 50 for r in recs if r not in long_) and len(recs) == 22 and any(I.ships(r) for r in recs if r not in long_)


def test_list_size_records():
    assert I.LIST_SIZES == (0, 1, 63, 64, 65, 257)   # none, one, a wavefront's lanes less one / exactly / plus one, more than a workgroup's threads
    for k in I.LIST_SIZES:
        recs = I.list_size_records(k)
        assert len(recs) == 300 and sum(I.ships(r) for r in recs) == k and not any(I.side_channel(r) for r in recs)
        if k > 1:
            assert I.ships(recs[0]) and I.ships(recs[-1])


def test_side_channel_sets():
    none, one = I.side_channel_one()
    assert sum(map(I.side_channel, none)) == 0 and sum(map(I.side_channel, one)) == 1 and not any(map(I.ships, none))
    recs = I.side_channel_forms()
    sc = [I.side_channel(r) for r in recs]
    assert sc[0] and sc[-1] and sum(sc) == 10 and any(a and b for a, b in zip(sc, sc[1:]))
    names = sorted(len(r["qname"]) for r in recs if I.side_channel(r))
    assert names[0] == 1 and names[-1] == 254
    lens = sorted(len(r["seq"]) for r in recs if I.side_channel(r))
    assert lens[:2] == [0, 1]
    assert any(I.side_channel(r) and r["seq"] and r["qual"] is None for r in recs)
    multi = [r for r in recs if I.side_channel(r) and len(I.cigar_ops(r)) > 1]
    assert len(multi) == 1 and I.ships(multi[0]) and len(I.cigar_ops(multi[0])) == 6 and multi[0]["flag"] & 8 and not multi[0]["flag"] & 4
    assert any(I.side_channel(r) and not r["flag"] & 12 for r in recs)           # '*' alone puts the line there
    assert any(I.side_channel(r) and I.cigar_ops(r) and not I.ships(r) for r in recs)   # MUNMAP, mapped, not clipped
    seventy = I.side_channel_seventy()
    assert len(seventy) == 400 and sum(map(I.side_channel, seventy)) == 70 and I.side_channel(seventy[-1]) and any(map(I.ships, seventy))
    lens = sorted(len(r["seq"]) for r in seventy if I.side_channel(r))
    assert lens[0] <= 1 and lens[-1] >= 65   # (from next to nothing to more than a wavefront's lanes)


def test_low_quality_sets():
    quiet, refused = I.low_quality_sets()
    assert " " in fields(quiet[1])[10] and not I.ships(quiet[1]) and not I.side_channel(quiet[1])
    assert len(refused) == 3
    kinds = []
    for recs in refused:
        assert " " in fields(recs[1])[10] and all(" " not in fields(r)[10] for r in (recs[0], recs[2]))
        kinds.append((I.ships(recs[1]), I.side_channel(recs[1])))
    assert kinds == [(True, False), (False, True), (False, True)]
    assert refused[1][1]["flag"] & 4 and refused[2][1]["flag"] & 12 == 8


def test_change_sets():
    none, recs = I.change_records()
    assert I.changes_model(none) == [] and all(r["tid"] == 0 for r in none)
    ch = I.changes_model(recs)
    assert ch == [(0, 1), (5, 2), (6, 0), (8, 2)]
    assert ch[0][0] == 0 and ch[-1][0] == len(recs) - 1 and ch[2][0] == ch[1][0] + 1   # the first record, the last, two in a row
    between = [i for i, r in enumerate(recs) if I.side_channel(r)]
    assert between == [2, 3] and recs[1]["tid"] == recs[4]["tid"] == 1 and all(recs[i]["tid"] == 2 for i in between)
    assert recs[2]["flag"] & 4 and recs[3]["flag"] & 12 == 8
    across = I.across_chunks_records()
    ch = I.changes_model(across)
    assert [t for _, t in ch] == [1, 2, 0] and I.side_channel(across[5]) and across[5]["tid"] == 2 and across[4]["tid"] == 1
    # cutting behind every line puts a change on the first record of a chunk (cut in front of records 2 and 8) and lets other chunks go on where the last one stopped
    assert {i for i, _ in ch} == {2, 6, 8}


def test_alternating():
    recs = I.alternating(65537)
    assert len(I.changes_model(recs)) == 65537 and len(I.changes_model(recs[:65536])) == 65536
    assert max(r["pos"] for r in recs) < min(I.ALTERNATING_LENS[:2])   # (the BAM decoder wants positions inside their contigs)
    assert len(I.body(recs)) < 1 << 22


def test_twelve():
    recs = I.twelve()
    assert len(recs) == 12 and sum(map(I.side_channel, recs)) == 6 and I.side_channel(recs[0]) and I.side_channel(recs[-1])
    assert sum(map(I.ships, recs)) == 4 and any(I.ships(r) and I.side_channel(r) for r in recs)
    assert len(I.changes_model(recs)) == 3
    assert any(r["seq"] == "" for r in recs) and any(r["qual"] is None and r["seq"] for r in recs) and any("xc" in r and I.ships(r) for r in recs) and any("xc" in r and not I.ships(r) for r in recs)
    assert any(I.cigar_ops(r)[:1] == [(2, "H")] for r in recs) and any(not I.cigar_ops(r) and not r["flag"] & 12 for r in recs)
    assert len(I.body(recs)) < 1200   # (the seam tests decode the file twice per byte offset)


def test_text_of_a_bam_says_its_records():
    """original_sam.sam_of_bam: the header lists the contigs, every record line gives back the record (through the decoder's own expectations, sam_text.expected)"""
    path = os.path.join(G.GOLDEN, "getclip", "filters.bam")
    data, n_head, names = original_sam.sam_of_bam(path)
    names2, recs = ST.read_bam_full(path)
    _, hnames, hlens = original_sam.bam_header(path)
    lines = data.decode("latin-1").split("\n")
    assert lines[-1] == "" and names == names2 == hnames and all(l.startswith("@") for l in lines[:n_head]) and not lines[n_head].startswith("@")
    assert [l.split("\t")[1:3] for l in lines[:n_head] if l.startswith("@SQ")] == [[f"SN:{n}", f"LN:{l}"] for n, l in zip(hnames, hlens)]
    assert len(lines) - 1 - n_head == len(recs) and sum("XC:i:1" in l for l in lines) == sum(r["xc"] for r in recs) > 0
    for l, r in zip(lines[n_head:], recs):
        f = l.split("\t")
        ops = bamio.parse_cigar(f[5]) if f[5] != "*" else []
        assert f[0] == r["qname"] and int(f[1]) == r["flag"] and int(f[3]) == r["pos"] + 1 and [[a, b] for a, b in ops] == r["cigar"] and (len(f[9]) if f[9] != "*" else 0) == r["l_qseq"]
        back = ST.expected(dict(qname=f[0], flag=int(f[1]), tid=names.index(f[2]) if f[2] != "*" else -1, pos=int(f[3]) - 1, mapq=int(f[4]), cigar=f[5],
                                mtid=(r["tid"] if f[6] == "=" else names.index(f[6])) if f[6] != "*" else -1, mpos=int(f[7]) - 1, isize=int(f[8]),
                                seq="" if f[9] == "*" else f[9], qual=None if f[10] == "*" else f[10], **({"xc": 1} if "XC:i:1" in f else {})))
        assert back == r, r["qname"]
    crlf, _, _ = original_sam.sam_of_bam(path, crlf=True, final_newline=False)
    assert crlf == data.replace(b"\n", b"\r\n")[:-2]
