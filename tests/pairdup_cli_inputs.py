"""The sample of tests/test_pairdup_cli_gpu.py: tests/markdup_cli_inputs.py's sample (through tests/coordsort_inputs.py's cli_sample, which adds pairs with one
unmapped end) with the copies at junction A clipped differently.  There the clipped first read of an original is `mM(100-m)S` at p, and its three copies are
the same read at the same place.  Here copy k starts with k + 2 bases soft-clipped - `(k+2)S(m-k-2)M(100-m)S` at p + k + 2, its mate's mpos moved with it - as
an aligner clips a copy whose first bases it could not place: four aligned positions, one unclipped 5' end.  `run -M`'s rule (aligned positions) finds none
of them; `run -D`'s marks all three copies of both originals."""
import functools

import coordsort_inputs as ci
import markdup_cli_inputs as CI
import markdup_model as mm
import pairdup_model as pm

NAMES, LENS = CI.NAMES, CI.LENS


@functools.lru_cache(maxsize=None)
def sample():
    """-> (contigs, records, coordinate sorted, no duplicate flag set)"""
    contigs, recs = ci.cli_sample()
    out = []
    for r in recs:
        name = r["qname"]
        if name.startswith("A") and "copy" in name:
            lead = int(name[-1]) + 2
            if r["tid"] == 0:       # the clipped read
                m = int(r["cigar"].split("M")[0])
                r = dict(r, pos=r["pos"] + lead, cigar=f"{lead}S{m - lead}M{100 - m}S")
            else:                   # its mate
                r = dict(r, mpos=r["mpos"] + lead)
        out.append(r)
    out.sort(key=lambda r: (r["tid"], r["pos"]))
    return contigs, tuple(out)


def flagged(recs):
    """the records, in the order given, with the pair rule's duplicate flags set"""
    return tuple(dict(r, flag=f) for r, f in zip(recs, pm.mark(list(recs))))


def flagged_by_M(recs):
    return tuple(dict(r, flag=f) for r, f in zip(recs, mm.mark(list(recs))))
