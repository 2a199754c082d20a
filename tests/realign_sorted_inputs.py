"""Inputs of tests/test_realign_sorted_model.py and tests/test_realign_sorted_gpu.py: one reference with the kinds of repeat the sorted index exists
for, a few tens of kilobases, and queries built for one rule of its seed admission each.  Seeded; the model runs over them in a second or two.

repeat_reference() -> (names, contigs):
  r0, r1, r2   random, about 3 kb
  E            300 exact copies of a 120-base element, each followed by a 40-base random spacer.  The stride (160) is a multiple of the sampling
               step, so every sampled 20-mer inside the element occurs exactly 300 times: more than the hash index's probe limit (256), more than
               the candidate array holds (192), fewer than bwa mem's default cap (500)
  F            12 copies of a 100-base element with 0-3 substitutions each, 37 random bases apart (stride 137: the copies are sampled in
               different phases); a query's seeds stay below 192
  polyA        6000 A: one 20-mer, ~1500 occurrences
  c35, c19     a contig that holds four sampled 20-mers, and one that holds none"""
import functools

import numpy as np

from realign_inputs import JUNK_BYTES, dna, revcomp, sub

E_LEN, E_GAP, E_COPIES = 120, 40, 300
E_STRIDE = E_LEN + E_GAP
F_LEN, F_GAP, F_COPIES = 100, 37, 12
F_STRIDE = F_LEN + F_GAP
POLY_A = 6000
NAMES = ("r0", "E", "r1", "F", "polyA", "c35", "r2", "c19")
CAPS = (1, 299, 300, 500, 65535)
E_COPY = 250   # the copy the part-repeat queries are cut from: beyond the 192 that admission in offset order would ever reach


@functools.lru_cache(maxsize=None)
def repeat_reference():
    rng = np.random.RandomState(1701)
    e = dna(rng, E_LEN)
    f = dna(rng, F_LEN)
    ctg_e = "".join(e + dna(rng, E_GAP) for _ in range(E_COPIES))
    ctg_f = dna(rng, 211)
    for k in range(F_COPIES):
        ctg_f += sub(f, sorted(set(int(x) for x in rng.randint(0, F_LEN, k % 4))), rng) + dna(rng, F_GAP)
    contigs = (dna(rng, 3001), ctg_e, dna(rng, 2999), ctg_f, "A" * POLY_A, dna(rng, 35), dna(rng, 3203), dna(rng, 19))
    return NAMES, contigs


def _junk(s, k):
    """s with its second byte replaced by one that is no base (the first two 20-mers go)"""
    return s[0] + JUNK_BYTES[k % len(JUNK_BYTES)] + s[2:]


@functools.lru_cache(maxsize=None)
def repeat_queries():
    """-> (queries, labels): every case as is, reverse-complemented, and each of the two with a junk byte (/fwd, /rev, /fwd-junk, /rev-junk)"""
    _, c = repeat_reference()
    rng = np.random.RandomState(1702)
    ctg_e, ctg_f = c[1], c[3]
    base = []
    for a in (0, 30, 60):
        base.append((f"E60@{a}", ctg_e[a:a + 60]))
    k0 = E_COPY * E_STRIDE
    base.append(("E36+spacer24", ctg_e[k0 + E_LEN - 36:k0 + E_LEN + 24]))
    base.append(("spacer24+E36", ctg_e[k0 + E_STRIDE - 24:k0 + E_STRIDE + 36]))
    base.append(("E20+spacer40", ctg_e[k0 + E_LEN - 20:k0 + E_LEN + 40]))
    for k in range(F_COPIES):
        at = 211 + k * F_STRIDE + 20
        base.append((f"F60-copy{k}", ctg_f[at:at + 60]))
    base.append(("polyA60", "A" * 60))
    base.append(("unique40+A20", c[0][1000:1040] + "A" * 20))
    base.append(("A20+unique40", "A" * 20 + c[2][500:540]))
    for i in range(6):
        base.append((f"random{i}", dna(rng, 60)))
    base.append(("c35", c[5]))
    base.append(("c19", c[7]))
    base.append(("c35-and-neighbours", c[4][-10:] + c[5] + c[6][:15]))
    for n in (19, 20, 1024, 1025):
        base.append((f"len{n}", c[6][700:700 + n]))
    q, lab = [], []
    for k, (name, s) in enumerate(base):
        r = revcomp(s)
        q += [s, r, _junk(s, k), _junk(r, k + 1)]
        lab += [name + "/fwd", name + "/rev", name + "/fwd-junk", name + "/rev-junk"]
    return tuple(q), tuple(lab)


def query(label):
    q, lab = repeat_queries()
    return q[lab.index(label)]


def e_copy_start(k):
    """global offset of copy k of the element inside contig E"""
    return k * E_STRIDE


def poly_a_sampled():
    """the indexed positions of the poly-A contig"""
    _, c = repeat_reference()
    lo = sum(len(x) for x in c[:4])
    return sum(1 for p in range(lo, lo + POLY_A - 19) if p % 4 == 0)


@functools.lru_cache(maxsize=None)
def repeat_model():
    import realign_model as M
    return M.Reference(repeat_reference()[1])


@functools.lru_cache(maxsize=None)
def repeat_expected(max_occ):
    """the model's hit of every query of repeat_queries() under this cap, computed once for all tests"""
    import realign_sorted_model as SM
    ref = repeat_model()
    return tuple(SM.align_sorted(ref, s, max_occ) for s in repeat_queries()[0])
