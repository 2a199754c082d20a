"""The inputs of tests/rare_inputs.py really have the properties tests/test_rare_paths_gpu.py relies on - checked with the oracle and the host
reader alone (no GPU): an input that stopped forcing its second attempt would leave the GPU test green and empty."""
import numpy as np
import pytest

import bamio
import oracle_lib as O
import rare_inputs as R
from seeksv_amd import host
from test_bam_reader import NAMES, LENS

SAMPLE = 4096   # events the first guess of the compact table's quality alphabet looks at (cluster_sort, clip_api.inc)


def _quals(b, lo, hi):
    """the quality bytes of reads [lo, hi) of a ladder batch"""
    lq = int(b["l_qseq"][0])
    entry = (lq + 1) // 2 + lq
    return b["seqqual"][:len(b["tid"]) * entry].reshape(-1, entry)[lo:hi, (lq + 1) // 2:]


@pytest.mark.parametrize("name,first,late,shape", R.TRANSITIONS, ids=[t[0] for t in R.TRANSITIONS])
def test_ladder_alphabet_arrives_late(name, first, late, shape):
    b = R.ladder_batch(first, late)
    o = O.getclip([b])
    assert o["n_events"] == 6000 > SAMPLE and o["n_clusters"] == 5744 and int((o["support"] == 3).sum()) == 128
    assert (o["side"] == ord("5")).sum() == (o["side"] == ord("3")).sum() == 2872            # both event lists fill
    early, rest = _quals(b, 0, 5000), _quals(b, 5001, 6000)   # (read 5000 is the third of a stack that began before: it carries the stack's qualities)
    assert 5000 > SAMPLE and not np.isin(early, late).any()
    assert set(np.unique(early)) == (set(first) if first else {0xff}) and set(np.unique(rest)) == set(first) | set(late)
    assert set(np.unique(_quals(b, 0, SAMPLE))) == (set(first) if first else {0xff})         # the first guess is `first`, all of it
    chars = set()
    for k in range(o["n_clusters"]):
        sl, ql, sr, qr, _ = host.cluster_strings(o, k)
        if ql != "*":
            chars |= set(ql) | set(qr)
    assert chars == {chr(v + 33) for v in set(first) | set(late)}
    assert bool(o["qual_missing"].any()) == (not first)


def test_ladder_options_reach_every_rung():
    first, late = R.TRANSITION["4to5"][1:3]
    plain = O.getclip([R.ladder_batch(first, late)])
    b = R.ladder_batch(first, late, n_every=7, big_bin=70000, long_skip=True)
    o = O.getclip([b])
    assert o["n_events"] == 76000 and int(o["support"].max()) == 70000 > 65535               # the support column needs 32 bits
    assert int(o["cigar"].max()) >> 4 == 4096 and int(plain["cigar"].max()) >> 4 < 4096        # an operation that needs more than 16 bits
    n_bases = sum(host.cluster_strings(o, k)[0].count("N") + host.cluster_strings(o, k)[2].count("N") for k in range(0, o["n_clusters"], 50))
    assert n_bases > 64                                                                          # (a fiftieth of the table alone overflows SSV_EXC_CAP=64)
    assert not np.isin(_quals(b, 0, 5000), late).any() and np.isin(_quals(b, 6000, 76000), late).any()


def test_clip_overflow_batch_fills_six_tiles():
    b = R.clip_overflow_batch()
    n = len(b["tid"])
    assert n == 12 * 8192
    clipped = b["n_cigar"] == 2
    per_tile = clipped.reshape(12, 8192).sum(axis=1)
    assert set(per_tile[:6]) <= {819, 820} and (per_tile[6:] == 8192).all()
    # a workgroup's share of the initial staging, one tile per workgroup (ssv_clip_scan_range): the dense tiles do not fit, the others do
    share = -(-max(1 << 16, n // 8) // 12)
    assert 820 <= share < 8192
    o = O.getclip([b])
    assert o["n_events"] == o["n_clusters"] == 54068


@pytest.mark.parametrize("tail", [False, True])
def test_getsv_overflow_batch_is_all_candidates(tail):
    b = R.getsv_overflow_batch(tail)
    hdr, plan = R.getsv_overflow_plan()
    n0 = 20 * 4096
    assert len(b["tid"]) == n0 + (100 if tail else 0) and (np.diff(b["pos"][:n0]) >= 0).all()
    assert [tuple(w) for w in plan.windows] == [(0, 5001, 16399)]
    # every record of the first contig starts in a 512-base tile that the one depth window touches
    assert (b["pos"][:n0] >> 9 >= 5001 >> 9).all() and (b["pos"][:n0] >> 9 <= 16399 >> 9).all()
    ntiles = -(-len(b["tid"]) // 4096)
    assert -(-max(1 << 16, len(b["tid"]) // 8) // ntiles) < 4096                                 # a workgroup's share of the initial staging: less than a tile
    mean, sd = R.GETSV_OVERFLOW_STATS
    c = O.discordant([b], plan.junctions, mean, sd, 4, 20)
    assert len(c) == 21 and int(c.min()) == 520 and int(c.max()) == 707
    rs, pd, mx = O.depth([b], plan.windows, plan.ranges, plan.points, 20)
    assert mx == 500 and int(pd.max()) == 500                                                    # far below the pileup's read cap
    plan.close()
    hdr.close()


def test_decoy_records_fool_the_record_start_rule(tmp_path):
    """(first_guess restates k_find_records' rule as it stands today: this proves that the fixture still fools the rule, nothing about the decoder)"""
    recs = R.decoy_records()
    path = str(tmp_path / "decoy.bam")
    bamio.write_bam(path, NAMES, LENS, recs)
    names, lens, batches = host.read_bam(path)
    assert sum(len(b["tid"]) for b in batches) == len(recs) == 604
    assert [int(p) for b in batches for p in b["pos"]] == [r["pos"] for r in recs]
    stream, starts = R.bgzf_blocks(path)
    true = set(R.true_record_starts(stream))
    assert len(true) == 604
    bounds = starts + [len(stream)]
    kinds = set()
    for k in range(1, len(starts)):
        lo, hi = bounds[k], bounds[k + 1]
        if lo == hi:
            continue
        g = R.first_guess(stream, lo, hi, len(NAMES), LENS)
        if g is not None and g not in true:
            kinds.add("holds a true start" if any(lo <= s < hi for s in true) else "holds none")
    assert kinds == {"holds a true start", "holds none"}
