"""The clipped-sequence re-alignments (clip.bam) as SAM text, for the tests of `seeksv getsv <clip.sam>`: a BAM read back with every field
(sam_text.read_bam_full) and written as the text `bwa mem` would have printed for the fields getsv looks at - header with the BAM header's @SQ lengths, SEQ
decoded from the packed nibbles, '*' for missing qualities and for an empty CIGAR (aux fields are dropped: getsv reads none of them) - and a plain-Python
model of the join's name hash (text_hash, junction_stage.cpp:42-50).  Test tooling only."""
import gzip
import struct

import sam_text as ST

M64 = (1 << 64) - 1


def text_hash(name):
    """clip_text_hash of the bytes (str: latin-1) with 64-bit wraparound: h = 0x9E3779B97F4A7C15 ^ n; per little-endian 8-byte word w, the tail zero padded:
    h = (h ^ w) * 0xFF51AFD7ED558CCD, h ^= h >> 29; result h * 0xC4CEB9FE1A85EC53"""
    b = name.encode("latin-1") if isinstance(name, str) else bytes(name)
    h = 0x9E3779B97F4A7C15 ^ len(b)
    for i in range(0, len(b), 8):
        w = int.from_bytes(b[i:i + 8], "little")  # (a short last slice is the zero-padded tail word)
        h = ((h ^ w) * 0xFF51AFD7ED558CCD) & M64
        h ^= h >> 29
    return (h * 0xC4CEB9FE1A85EC53) & M64


def bam_header(path):
    """-> (target names, target lengths) of a BAM"""
    data = gzip.open(path, "rb").read()
    assert data[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, p)
    p += 4
    names, lens = [], []
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", data, p)
        names.append(data[p + 4:p + 4 + l - 1].decode())
        lens.append(struct.unpack_from("<i", data, p + 4 + l)[0])
        p += 4 + l + 4
    return names, lens


def records(path):
    """the BAM's records as the dicts sam_text.line writes: seq as characters, qual None (-> '*') when the BAM holds none"""
    _, recs = ST.read_bam_full(path)
    out = []
    for r in recs:
        n = r["l_qseq"]
        packed, qual = bytes.fromhex(r["seq"]), bytes.fromhex(r["qual"])
        seq = "".join(ST.NT16[(packed[i >> 1] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(n))
        out.append(dict(qname=r["qname"], flag=r["flag"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar=[(l, op) for l, op in r["cigar"]],
                        mtid=r["mtid"], mpos=r["mpos"], isize=r["isize"], seq=seq, qual=None if n == 0 or qual == b"\xff" * n else qual))
    return out


def text(path, **kw):
    """the whole SAM file (str) for the BAM at `path`; kw: sam_text.text's (crlf, final_newline, with_header, ...)"""
    names, lens = bam_header(path)
    return ST.text(records(path), names, lens, **kw)


def write(sam_path, bam_path, **kw):
    """the BAM as SAM text at sam_path (gzip when it ends in .gz); -> the bytes"""
    data = text(bam_path, **kw).encode("latin-1")
    with (gzip.open(sam_path, "wb") if sam_path.endswith(".gz") else open(sam_path, "wb")) as f:
        f.write(data)
    return data
