"""The original alignments as SAM text: a BAM read with sam_text.read_bam_full, written as the text `samtools view -h` would give for it, keeping XC:i:
(clip_sam.py, for the clipped-sequence alignments, drops the optional fields).  Test tooling only."""
import gzip
import struct

import bamio
import sam_text as ST


def bam_header(path):
    """-> (header text, contig names, contig lengths) of a BAM"""
    data = gzip.open(path, "rb").read(1 << 24)
    assert data[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", data, 4)
    text = data[8:8 + l_text].split(b"\0")[0].decode("latin-1")
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, p)
    p += 4
    names, lens = [], []
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", data, p)
        names.append(data[p + 4:p + 4 + l - 1].decode())
        lens.append(struct.unpack_from("<i", data, p + 4 + l)[0])
        p += 4 + l + 4
    return text, names, lens


def header_text(path):
    """the BAM's own header text when it lists the contigs, one made from its reference list otherwise"""
    text, names, lens = bam_header(path)
    if sum(1 for l in text.split("\n") if l.startswith("@SQ")) != len(names):
        text = "".join(l + "\n" for l in text.split("\n") if l and not l.startswith("@SQ")) + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(names, lens))
    return text if not text or text.endswith("\n") else text + "\n"


def record_line(r, names):
    """one record of read_bam_full as a line of text (no line end); a non-zero XC stays as XC:i:1"""
    lq = r["l_qseq"]
    packed, qual = bytes.fromhex(r["seq"]), bytes.fromhex(r["qual"])
    seq = "".join(bamio.NT16[(packed[k >> 1] >> (4 if k % 2 == 0 else 0)) & 15] for k in range(lq)) or "*"
    q = "*" if lq == 0 or all(b == 0xff for b in qual) else "".join(chr(b + 33) for b in qual)
    tid, mtid = r["tid"], r["mtid"]
    f = [r["qname"], str(r["flag"]), names[tid] if tid >= 0 else "*", str(r["pos"] + 1), str(r["mapq"]), ST.cigar_text([tuple(c) for c in r["cigar"]]),
         "*" if mtid < 0 else "=" if mtid == tid else names[mtid], str(r["mpos"] + 1), str(r["isize"]), seq, q]
    if r["xc"]:
        f.append("XC:i:1")
    return "\t".join(f)


def sam_of_bam(path, crlf=False, final_newline=True):
    """-> (the whole file as bytes, number of header lines, contig names)"""
    names, recs = ST.read_bam_full(path)
    head = header_text(path)
    eol = "\r\n" if crlf else "\n"
    body = eol.join(record_line(r, names) for r in recs)
    if recs and final_newline:
        body += eol
    return (head.replace("\n", eol) + body).encode("latin-1"), head.count("\n"), names
