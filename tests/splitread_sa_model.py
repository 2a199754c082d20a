"""`seeksv run -A -S` in plain Python: the split-read rule of tests/splitread_model.py (imported, not edited) plus virtual candidates from SA tags.  The rule
as include/seeksv_hip.h states it at ssv_rt_begin_original_sa:

1. Who gets a virtual candidate.  A SOURCE is a record that takes part under ssv_rt_begin_original's rule and carries the read (no H, bases present,
   l_qseq == R).  Only a source has its optional fields looked at.  A hard-clipped record never gets a virtual candidate.
2. Finding the value.
   BAM: the typed fields are walked as libbam does: A c C s S i I f d Z H B; an unknown type ends the walk.  The first field with tag SA and type Z is
   taken; SA with another type is passed over.  Nothing is read beyond the record's block_size: a Z or H value with no NUL before the record's end, or a
   B array that runs over it, ends the walk with no value.
   SAM text: optional fields start at field 12.  A field matches only when it begins with "SA:Z:" directly behind a tab.  The value ends at the tab, at a
   '\\r' before the newline, at the newline, or at the end of the last line.
3. The value's grammar: rname,pos,strand,CIGAR,mapQ,NM; - one entry, parsed as written: rname up to the first ','; pos decimal 1 to 2^31-1; strand '+' or
   '-'; CIGAR one or more operations of MIDNSHP=X, each length below 2^28, at most 65535; mapQ decimal 0 to 255; NM a run of digits (at least one),
   ignored; the entry ends with ';', a missing final ';' at the value's end is accepted.  Anything else is sa_refused.  Bytes behind the first entry's ';'
   make it sa_multi.  rname must be a contig of the header, by exact name: else sa_refused.
4. The virtual candidate is what a record with that tid, pos0, strand and CIGAR would give (S stands for the record's H; both are clips): exactly one
   end clipped and mapQ >= min_mapq, else sa_refused; same formulas; its source's name, key, mate bits and record index; no bases, never carries the read.
5. Pairing.  Phase 1: hold / pair / drop over the real candidates alone - exactly splitread_model.find_pairs.  Phase 2: every real candidate that left
   phase 1 with no partner and is nobody's partner, if it owns a virtual candidate, pairs with it (source = A, held; virtual = B, completing) when the
   strand / side test passes and R_source == R_virtual (unequal: sa_dropped_length).  A virtual candidate whose source found a real partner is
   sa_redundant.  The row stands where a record right behind the source would have completed it.
6. Everything behind the pairing is splitread_model.pair_of.

Slow and obvious on purpose; it shares nothing with the kernels (seeksv_amd/csrc/splitread_sa_parse.h, splitread_sa_kernels.h)."""
import re
import struct

import splitread_model as SM

SA_COUNTS = ("sa_tags", "sa_multi", "sa_refused", "virtuals", "sa_redundant", "pairs_from_sa", "sa_dropped_length")
BAM, SAM = 0, 1
_FIXED = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4, b"d": 8}
_ENTRY = re.compile(rb"([^,]*),([0-9]+),([+-]),((?:[0-9]+[MIDNSHP=X])+),([0-9]+),([0-9]+)", re.S)
_OP = re.compile(rb"([0-9]+)([MIDNSHP=X])")


def find_bam(aux):
    """the value of the first SA:Z field among BAM's typed fields (bytes: the record's optional-field area), or None"""
    p, end = 0, len(aux)
    while end - p >= 3:
        tag, ty = aux[p:p + 2], aux[p + 2:p + 3]
        p += 3
        if ty in _FIXED:
            size = _FIXED[ty]
        elif ty in (b"Z", b"H"):
            nul = aux.find(b"\0", p)
            if nul < 0:
                return None
            if ty == b"Z" and tag == b"SA":
                return aux[p:nul]
            size = nul - p + 1
        elif ty == b"B":
            if end - p < 5:
                return None
            size = 5 + struct.unpack_from("<I", aux, p + 1)[0] * {b"c": 1, b"C": 1, b"s": 2, b"S": 2}.get(aux[p:p + 1], 4)
        else:
            return None
        if end - p < size:
            return None
        p += size
    return None


def find_sam(area):
    """the value of the first field that begins with SA:Z: in a line's text from field 12 on (bytes; it may still hold the line's end), or None"""
    line = area.split(b"\n")[0]
    if area[len(line):len(line) + 1] == b"\n" and line.endswith(b"\r"):
        line = line[:-1]
    for field in line.split(b"\t"):
        if field.startswith(b"SA:Z:"):
            return field[5:]
    return None


def parse_entry(value):
    """-> ("ok", dict(rname, pos0, strand, ops [(len, op code)], mapq)) | ("refused", None) | ("multi", None)"""
    m = _ENTRY.match(value)
    if not m:
        return "refused", None
    rest = value[m.end():]
    if rest not in (b"", b";") and not rest.startswith(b";"):
        return "refused", None
    pos, mapq = int(m.group(2)), int(m.group(5))
    ops = [(int(l), b"MIDNSHP=X".index(c)) for l, c in _OP.findall(m.group(4))]
    if not 1 <= pos <= 2 ** 31 - 1 or mapq > 255 or len(ops) > 65535 or any(l >= 2 ** 28 for l, _ in ops):
        return "refused", None
    if len(rest) > 1:
        return "multi", None
    return "ok", dict(rname=m.group(1), pos0=pos - 1, strand=m.group(3).decode(), ops=ops, mapq=mapq)


def virtual_of(source, value, min_mapq, contigs):
    """a source candidate's SA value -> ("ok", the virtual candidate) | ("refused", None) | ("multi", None)"""
    status, e = parse_entry(value)
    if status != "ok":
        return status, None
    names = [c.encode() if isinstance(c, str) else c for c in contigs]
    if e["rname"] not in names or e["mapq"] < min_mapq or SM.clipped(e["ops"][0][1]) == SM.clipped(e["ops"][-1][1]):
        return "refused", None
    R, side, left, right, ref_len = SM.lengths(e["ops"])
    return "ok", dict(tid=names.index(e["rname"]), pos=e["pos0"] + (1 if side == "5" else ref_len), side=side, left=left, right=right, R=R, strand=e["strand"],
                      cigar=[(l, op) for l, op in e["ops"] if not SM.clipped(op)], carries=False, hard=False, bases=None, rec=source["rec"], key=source["key"])


def _geometry_passes(a, b):
    same_strand, same_side = a["strand"] == b["strand"], a["side"] == b["side"]
    return (same_strand and not same_side) or (not same_strand and same_side)


def find_pairs(batches, names, auxes, min_mapq, contigs):
    """the rule over batches in input order.  auxes[k] = (encoding BAM | SAM, [the optional-field bytes of every record of batch k]).
    -> (rows in the order of the completing record, a virtual row right behind its source; counts: splitread_model.COUNTS; sa_counts: SA_COUNTS)"""
    counts, sa = dict.fromkeys(SM.COUNTS, 0), dict.fromkeys(SA_COUNTS, 0)
    held, real, virtual_of_rec, partnered, rows, rec_index = {}, [], {}, set(), [], 0
    # ---- phase 1: splitread_model.find_pairs' loop, which also notes who found a partner and which sources own a virtual candidate ----
    for b, nm, (enc, areas) in zip(batches, names, auxes):
        for i in range(len(b["tid"])):
            this = rec_index
            rec_index += 1
            if not SM.takes_part(b, i, min_mapq, len(contigs)):
                continue
            c = SM.candidate_of(b, i, nm[i].encode()[:255], this)
            real.append(c)
            counts["candidates"] += 1
            counts["hard_clipped"] += c["hard"]
            if c["carries"]:
                value = (find_sam if enc == SAM else find_bam)(bytes(areas[i]))
                if value is not None:
                    sa["sa_tags"] += 1
                    status, v = virtual_of(c, value, min_mapq, contigs)
                    sa[{"ok": "virtuals", "refused": "sa_refused", "multi": "sa_multi"}[status]] += 1
                    if v:
                        virtual_of_rec[this] = v
            a = held.get(c["key"])
            if a is None:
                held[c["key"]] = c
                continue
            if not _geometry_passes(a, c):
                continue
            if a["R"] != c["R"]:
                counts["dropped_length"] += 1
                continue
            if not (a["carries"] or c["carries"]):
                counts["dropped_no_carrier"] += 1
                continue
            row, borrowed = SM.pair_of(a, c, contigs)
            rows.append(((this, 0), row))
            counts["pairs"] += 1
            counts["pairs_borrowed"] += borrowed
            partnered.update((a["rec"], c["rec"]))
            del held[c["key"]]
    # ---- phase 2: the sources left alone against their virtual candidates ----
    for c in real:
        v = virtual_of_rec.get(c["rec"])
        if v is None:
            continue
        if c["rec"] in partnered:
            sa["sa_redundant"] += 1
            continue
        if not _geometry_passes(c, v):
            continue
        if c["R"] != v["R"]:
            sa["sa_dropped_length"] += 1
            continue
        row, borrowed = SM.pair_of(c, v, contigs)
        rows.append(((c["rec"], 1), row))
        sa["pairs_from_sa"] += 1
        counts["pairs"] += 1
        counts["pairs_borrowed"] += borrowed
    rows.sort(key=lambda r: r[0])
    return [r for _, r in rows], counts, sa
