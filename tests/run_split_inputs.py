"""Inputs of tests/test_realign_split_batch_gpu.py and tests/test_run_split_gpu.py: query sets for the device row builder
(ssv_realign_split_batch) on the reference of tests/realign_split_inputs.py - the shapes at which packing bases and qualities goes wrong - and a
variant of that module's end-to-end sample in which both unmapped-pair FASTQ files hold junction reads.  tests/test_run_split_inputs.py holds every
set to its property with the models alone; a set that misses its property is changed here, not excused there.

A set is a tuple of (name, sequence, quality text); names are unique within a set (the -F pass pairs records by name)."""
import functools

import numpy as np

import readthrough_model as RM
import realign_model as M
import realign_split_inputs as SI
import realign_split_model as SM
from realign_inputs import dna, revcomp

# every length at which the row kernel takes another path: nothing, one base, around the shortest aligned read, around 64 / 128 bases (8 / 16 whole
# dwords of nibbles), around 512 (one round of the wavefront's nibble dwords), the longest aligned read, one more, and far more
LENGTHS = (0, 1, 19, 20, 21, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1024, 1025, 1500)
NAME_1 = "abcdefghijklmnopqrstuvwxyz"   # the names of one byte
LONG_NAME = 254


def _qual(rng, n):
    return "".join(chr(33 + int(x)) for x in rng.randint(0, 42, n))


def _plain_contigs():
    return [c for i, c in enumerate(SI.reference()) if i != 7]   # (not the contig with the five copies of 30 bases)


def _stretch(rng, n):
    """n bases of one contig (long enough for it), either strand"""
    fits = [c for c in _plain_contigs() if len(c) > n + 40]
    c = fits[int(rng.randint(len(fits)))]
    p = int(rng.randint(20, len(c) - n - 20))
    s = c[p:p + n]
    return revcomp(s) if rng.randint(2) else s


class _Names:
    """unique names: one byte while they last, then lengths 2.. in turn, a 254-byte one every `long_every` reads"""
    def __init__(self, tag, long_every=7):
        self.tag, self.k, self.long_every = tag, 0, long_every

    def next(self):
        k = self.k
        self.k += 1
        if k < 3:
            return NAME_1[(ord(self.tag[0]) + k) % 26]
        if k % self.long_every == 3:
            head = f"{self.tag}{k}_"
            return head + "x" * (LONG_NAME - len(head))
        return f"{self.tag}{k}" + "/1"[: k % 3] + "y" * (k % 8)


def _set(tag, seqs, seed):
    rng = np.random.RandomState(seed)
    nm = _Names(tag)
    out = tuple((nm.next(), s, _qual(rng, len(s))) for s in seqs)
    assert len({e[0] for e in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def length_set():
    """every length of LENGTHS three times: a stretch of the reference on either strand where the length aligns (1,024: 400 bases | 324 of nothing | 300
    bases of another place - 167 seeds, fewer than candidate slots -, as a whole reverse-complemented once), random or reference text where it does not"""
    rng = np.random.RandomState(2501)
    text = "".join(SI.reference())
    seqs = []
    for n in LENGTHS:
        for k in range(3):
            if n < M.K:
                seqs.append(dna(rng, n))
            elif n > M.MAX_Q:
                seqs.append(text[100 + k:100 + k + n])
            elif n == 1024:
                s = _stretch(rng, 400) + dna(rng, 324) + _stretch(rng, 300)
                seqs.append(revcomp(s) if k == 1 else s)
            else:
                seqs.append(_stretch(rng, n))
    return _set("L", seqs, 2502)


@functools.lru_cache(maxsize=None)
def alphabet_set():
    """N, other letters and lower case in split reads of every strand combination: an N is a mismatch, lower case is not; both records of a read carry the
    same codes, mirrored on the reverse strand"""
    seqs = []
    for name in ("ff", "fr", "rf", "rr"):
        r = SI.read(name)
        c = revcomp(r)[:-2]
        seqs += [r[1:].lower(), r[:7] + "N" + r[8:91] + "n" + r[92:], c[:50].lower() + c[50:], r[:30] + "R" + r[31:65] + "." + r[66:], "N" * 37 + r[40:]]   # 99, 100, 98, 100, 97 bases
    seqs += ["N" * 33, "n" * 64, "acgtn" * 13]
    return _set("A", seqs, 2503)


@functools.lru_cache(maxsize=None)
def strand_set():
    """each strand combination of primary and mate, the read as drawn and reverse-complemented; overlap, gap, deletion"""
    return _set("S", SI.geometry_set()[0], 2504)


@functools.lru_cache(maxsize=None)
def no_mate_set():
    """no read has a mate: one stretch each, random sequence, too short, too long, a piece inside the other, an own part of 19"""
    rng = np.random.RandomState(2505)
    seqs = [_stretch(rng, int(n)) for n in rng.randint(30, 200, 24)] + [dna(rng, 77), dna(rng, 19), "".join(SI.reference())[7:7 + 1100], SI.read("contained"), SI.read("own19"),
                                                                         revcomp(SI.read("len40"))]
    return _set("N", seqs, 2506)


@functools.lru_cache(maxsize=None)
def all_mate_set():
    """every read has a mate"""
    names = ("ff", "fr", "rf", "rr", "overlap5", "gap10", "del20", "own20", "mapq5050", "len64", "len65", "len250", "len1024")
    seqs = []
    for n in names:
        seqs += [SI.read(n), revcomp(SI.read(n))]
    return _set("M", seqs, 2507)


def one_set():
    return _set("O", [SI.read("fr")], 2508)


def empty_set():
    return ()


SETS = dict(length=length_set, alphabet=alphabet_set, strand=strand_set, no_mate=no_mate_set, all_mate=all_mate_set, one=one_set, empty=empty_set)


def offsets_mod8(entries):
    """-> (where the reads start, where the names start) modulo 8, as ssv_realign_split_batch's caller lays them out: back to back, names with their NULs"""
    so, no, s_at, n_at = set(), set(), 0, 0
    for name, s, _ in entries:
        so.add(s_at % 8); no.add(n_at % 8)
        s_at += len(s); n_at += len(name.encode()) + 1
    return so, no


@functools.lru_cache(maxsize=None)
def model_reference():
    return M.Reference(SI.reference())


def model_results(entries, max_occ=None, ref=None):
    """align_split of every read of a set"""
    ref = ref or model_reference()
    return [SM.align_split(ref, s, max_occ) for _, s, _ in entries]


def model_rows(entries, results):
    """the records `seeksv realign -P` writes for a set, as tests/bamio.py's record dicts (qname, cigar as [(length, code)]): realign_split_model.bam_records
    of every read, one after the other"""
    rows = []
    for (name, s, q), res in zip(entries, results):
        for r in SM.bam_records(name, s, q, res):
            rows.append(dict(qname=r["name"], flag=r["flag"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar=[(l, RM.OPS.index(op)) for l, op in r["cigar"]],
                             seq=r["seq"], qual=r["qual"]))
    return rows


def model_junctions(rows, contigs, min_mapq=1):
    """the rows through the -F model -> (pairs, n_candidates)"""
    batch, names = RM.batch_from_records(rows)
    return RM.find_junction([batch], [names], min_mapq, list(contigs))


# ---- end to end: `seeksv run -P` ----
def unmapped_fastq(recs):
    """getclip's unmapped-pair side channel over bamio record dicts in file order -> (entries of prefix.unmapped_1.fq, entries of _2.fq): a pair is
    written when its second record comes by, READ1's data to file 1 and READ2's to file 2, names with /1 and /2; bases as stored"""
    held, f1, f2 = {}, [], []
    for r in recs:
        if not r["flag"] & 12:
            continue
        end = 1 if r["flag"] & 64 else 2
        if r["qname"] not in held:
            held[r["qname"]] = (end, r)
            continue
        e0, r0 = held[r["qname"]]
        if e0 == end:
            continue
        a, b = (r0, r) if e0 == 1 else (r, r0)
        f1.append((r["qname"] + "/1", a["seq"], a["qual"]))
        f2.append((r["qname"] + "/2", b["seq"], b["qual"]))
        del held[r["qname"]]
    return f1, f2


@functools.lru_cache(maxsize=None)
def e2e_variant():
    """realign_split_inputs.e2e_sample() with READ1 as the unmapped end of every odd junction pair: prefix.unmapped_1.fq.gz and prefix.unmapped_2.fq.gz
    both hold junction reads (and both hold mapped mates, which come back 100M and seed nothing) -> (contigs, records)"""
    contigs, recs = SI.e2e_sample()
    out = []
    for r in recs:
        r = dict(r)
        if r["qname"].startswith("jn") and int(r["qname"][2:]) % 2:
            r["flag"] = {73: 137, 133: 69}[r["flag"]]   # the mapped end becomes READ2 (1 + 8 + 128), the unmapped one READ1 (1 + 4 + 64)
        out.append(r)
    return contigs, tuple(out)


E2E_KEY = ("tA", SI.E2E_A + 1, "+", "tB", SI.E2E_B + 1, "+")
