"""SAM text for the `getsv -F` tests: writes the record dicts of tests/readthrough_inputs.py / tests/bamio.py (qname, flag, tid, pos 0-based, mapq, cigar,
mtid, mpos, isize, seq, qual None | bytes | str, and optionally xc: the value of an XC:i: tag, tags: further optional fields) as SAM text, in variants
that encode to the same records, and reads a BAM back with every field (what tests/bamio.read_bam_records leaves out).  Plain Python, test tooling only."""
import copy
import ctypes as C
import gzip
import struct

import numpy as np

import bamio

NT16 = bamio.NT16


def header(names, lens):
    return "@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(names, lens))


def cigar_text(cig):
    if isinstance(cig, str):
        return cig if cig else "*"
    return "".join(f"{l}{bamio.CIGAR_OPS[op] if isinstance(op, int) else op}" for l, op in cig) or "*"


def qual_text(q):
    if q is None:
        return "*"
    if isinstance(q, str):
        return q
    return "".join(chr(b + 33) for b in q)


def line(r, names, k=0, lower=False, dot_n=False, hex_flags=False, tags=False):
    """one record line without its line end.  The variants change the text, not the record: lower-case bases, '.' for N, flags in hex, optional fields
    behind QUAL (tags: a few that the decoder must ignore; an `xc` of the record becomes an XC:i: tag in every variant)"""
    tid, mtid = r.get("tid", -1), r.get("mtid", -1)
    seq = r.get("seq", "") or "*"
    if lower:
        seq = seq.lower()
    if dot_n:
        seq = seq.replace("N", ".").replace("n", ".")
    flag = r.get("flag", 0)
    f = [r["qname"], hex(flag) if hex_flags else str(flag), names[tid] if tid >= 0 else "*", str(r.get("pos", -1) + 1), str(r.get("mapq", 0)),
         cigar_text(r.get("cigar", "")), "*" if mtid < 0 else "=" if mtid == tid else names[mtid], str(r.get("mpos", -1) + 1), str(r.get("isize", 0)),
         seq, qual_text(r.get("qual")) if r.get("seq", "") else "*"]
    opt = []
    if tags:
        opt += [f"NM:i:{k % 7}", "XS:Z:XC:i:9", f"AS:i:{50 + k % 50}"][:1 + k % 3]
    if "xc" in r:
        opt.insert(len(opt) // 2, f"XC:i:{r['xc']}")
    opt += list(r.get("tags", []))
    return "\t".join(f + opt)


def text(recs, names, lens, crlf=False, final_newline=True, with_header=True, **variant):
    """the whole file as str"""
    eol = "\r\n" if crlf else "\n"
    body = eol.join(line(r, names, k, **variant) for k, r in enumerate(recs))
    if recs and final_newline:
        body += eol
    return (header(names, lens).replace("\n", eol) if with_header else "") + body


def write(path, recs, names, lens, **kw):
    data = text(recs, names, lens, **kw).encode("latin-1")
    with (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")) as f:
        f.write(data)
    return data


def clip_positions(recs, lens):
    """what readthrough_inputs.write_f_bam does to the positions before it writes the BAM"""
    for r in recs:
        r["pos"] = max(0, min(int(r["pos"]), lens[r["tid"]] - 1))
    return recs


def has_eq_x(r):
    c = r.get("cigar", "")
    return any(ch in cigar_text(c) for ch in "=X")


def without_eq_x(recs):
    """the records whose NAME owns no '=' / 'X' CIGAR (libbam 0.1.16's text reader aborts on those characters)"""
    bad = {r["qname"] for r in recs if has_eq_x(r)}
    return [r for r in recs if r["qname"] not in bad]


def with_extras(recs, seed, n_targets=3):
    """copies of the records with qualities, mate fields and XC tags (the -F path reads none of them: the decoder must still get them right)"""
    rng = np.random.RandomState(seed)
    out = copy.deepcopy(recs)
    for r in out:
        n = len(r.get("seq", ""))
        if rng.rand() < 0.8:
            r["qual"] = bytes(rng.randint(0, 94, n).astype(np.uint8).tolist())
        m = rng.rand()
        if m < 0.4:
            r["mtid"], r["mpos"], r["isize"] = r["tid"], int(rng.randint(0, 3000)), int(rng.randint(-2000, 2000))
        elif m < 0.6:
            r["mtid"], r["mpos"] = int(rng.randint(0, n_targets)), int(rng.randint(0, 3000))
        if rng.rand() < 0.3:
            r["xc"] = int(rng.choice([0, 0, 1, 7, 100]))
    return out


def bam_aux(r):
    """the record's `xc` as BAM aux bytes (for bamio.write_bam)"""
    return b"XCi" + struct.pack("<i", r["xc"]) if "xc" in r else b""


def read_bam_full(path):
    """-> (target_names, [dict(qname, flag, tid, pos, mapq, cigar=[[len, code]], mtid, mpos, isize, l_qseq, seq (hex of the packed nibbles), qual (hex), xc)])"""
    data = gzip.open(path, "rb").read()
    assert data[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, p)
    p += 4
    names = []
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", data, p)
        names.append(data[p + 4:p + 4 + l - 1].decode())
        p += 4 + l + 4
    recs = []
    while p < len(data):
        bs, tid, pos, l_rn, mapq, _bin, n_cig, flag, l_seq, mtid, mpos, isize = struct.unpack_from("<iiiBBHHHiiii", data, p)
        end = p + 4 + bs
        q = p + 36
        qname = data[q:q + l_rn - 1].decode("latin-1")
        q += l_rn
        cig = [[c >> 4, c & 15] for c in struct.unpack_from("<%dI" % n_cig, data, q)]
        q += 4 * n_cig
        seq = data[q:q + (l_seq + 1) // 2]
        q += (l_seq + 1) // 2
        qual = data[q:q + l_seq]
        q += l_seq
        xc = 0
        while q < end:  # aux: tag, type, value
            tag, ty = data[q:q + 2], chr(data[q + 2])
            q += 3
            if ty in "cCsSiI":
                size = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4}[ty]
                v = int.from_bytes(data[q:q + size], "little", signed=ty.islower())
                q += size
                if tag == b"XC":
                    xc = int(v != 0)
            elif ty == "A":
                q += 1
            elif ty in "fF":
                q += 4
            elif ty in "ZH":
                q = data.index(b"\0", q) + 1
            else:
                raise ValueError("aux type " + ty)
        recs.append(dict(qname=qname, flag=flag, tid=tid, pos=pos, mapq=mapq, cigar=cig, mtid=mtid, mpos=mpos, isize=isize, l_qseq=l_seq,
                         seq=seq.hex(), qual=qual.hex(), xc=xc))
        p = end
    return names, recs


def expected(r):
    """a record dict as read_bam_full gives it back from a BAM (or from the decoder) of that record"""
    cig = r.get("cigar", "")
    cig = bamio.parse_cigar(cig) if isinstance(cig, str) and cig not in ("", "*") else ([] if isinstance(cig, str) else cig)
    seq = r.get("seq", "")
    packed = bytearray((len(seq) + 1) // 2)
    for i, ch in enumerate(seq):
        packed[i >> 1] |= NT16.index(ch.upper()) << (4 if i % 2 == 0 else 0)
    q = r.get("qual")
    qual = b"\xff" * len(seq) if q is None else bytes(ord(c) - 33 for c in q) if isinstance(q, str) else bytes(q)
    return dict(qname=r["qname"], flag=r.get("flag", 0), tid=r.get("tid", -1), pos=r.get("pos", -1), mapq=r.get("mapq", 0), cigar=[[l, op] for l, op in cig],
                mtid=r.get("mtid", -1), mpos=r.get("mpos", -1), isize=r.get("isize", 0), l_qseq=len(seq), seq=bytes(packed).hex(), qual=qual.hex(),
                xc=int(r.get("xc", 0) != 0))


def batch_records(b, names):
    """a host batch (dict of arrays: Context.batch_to_host, host.BamReader.read_batch) + read names -> records as read_bam_full gives them"""
    out = []
    for i in range(len(b["tid"])):
        co, nc, lq, so = int(b["cigar_off"][i]), int(b["n_cigar"][i]), int(b["l_qseq"][i]), int(b["seq_off"][i])
        nb = (lq + 1) // 2
        out.append(dict(qname=names[i], flag=int(b["flag"][i]), tid=int(b["tid"][i]), pos=int(b["pos"][i]), mapq=int(b["mapq"][i]),
                        cigar=[[int(c) >> 4, int(c) & 15] for c in b["cigar"][co:co + nc]], mtid=int(b["mtid"][i]), mpos=int(b["mpos"][i]), isize=int(b["isize"][i]),
                        l_qseq=lq, seq=bytes(b["seqqual"][so:so + nb]).hex(), qual=bytes(b["seqqual"][so + nb:so + nb + lq]).hex(), xc=int(b["xc"][i])))
    return out


def ends_of(r):
    """the cigar_ends byte of a record as read_bam_full gives it"""
    return 0xff if not r["cigar"] else r["cigar"][0][1] | r["cigar"][-1][1] << 4


_hip = None


def hip_runtime():
    """the HIP runtime the library is linked against (loaded already), for the few raw calls the GPU tests make themselves"""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


def device_to_host(ctx, ptr, nbytes):
    """nbytes of the context's GPU memory at ptr -> bytes (the read names and record lines of a device batch)"""
    ctx.sync()
    buf = C.create_string_buffer(max(1, int(nbytes)))
    assert not nbytes or hip_runtime().hipMemcpy(buf, ptr, int(nbytes), 2) == 0
    return buf.raw[:int(nbytes)]


def names_to_host(ctx, names, n):
    """the n read names an _abi.Names in HBM points at (Context.samdec_names: its `bytes` says how much text there is) -> list of str"""
    if n == 0:
        return []
    off = np.frombuffer(device_to_host(ctx, names.off, n * 8), dtype=np.uint64)
    raw = device_to_host(ctx, names.base, int(names.bytes)) + b"\0"
    return [raw[int(o) + names.bias:raw.index(b"\0", int(o) + names.bias)].decode("latin-1") for o in off]
