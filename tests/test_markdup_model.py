"""The plain model of the duplicate-marking rule (tests/markdup_model.py) against the answers written by hand beside every input set (tests/markdup_inputs.py)."""
import pytest

import markdup_inputs as mi
import markdup_model as mm


@pytest.mark.parametrize("s", mi.SETS, ids=[s["name"] for s in mi.SETS])
def test_model_gives_the_written_answers(s):
    flags = mm.mark(s["records"])
    marked = [i for i, (f, r) in enumerate(zip(flags, s["records"])) if f != r["flag"]]
    assert marked == s["dup"]
    assert all(flags[i] == s["records"][i]["flag"] | 0x400 for i in marked)      # nothing but the one bit, and a preset bit stays as it is
    assert all(f & 0x400 for f, r in zip(flags, s["records"]) if r["flag"] & 0x400)


def test_digest_is_fnv1a_over_name_and_positions():
    # FNV-1a's step with the constants the read-through stage hashes names with (its offset basis is the project's 19-digit one, not the published 20-digit one)
    assert mm.fnv1a(b"") == 1469598103934665603 and mm.fnv1a(b"a") == ((1469598103934665603 ^ 97) * 1099511628211) % (1 << 64)
    assert mm.fnv1a(b"ab") == ((mm.fnv1a(b"a") ^ 98) * 1099511628211) % (1 << 64)
    h, t = mi.pair("n", 0, 100, 1, 300)
    assert mm.is_head(h) and not mm.is_head(t)
    assert mm.digest(h) == mm.digest(t) == mm.fnv1a(b"n" + (0).to_bytes(4, "little") + (100).to_bytes(4, "little") + (1).to_bytes(4, "little") + (300).to_bytes(4, "little"))
    assert mm.digest(h, 4) == mm.digest(h) & 15


def test_stats_of_a_set():
    st = {}
    mm.mark(mi.BY_NAME["mixed"]["records"], stats=st)
    # 12 paired records take part; groups looked at: two at c0:100, one at c0:400 (the heads' runs have two records or more)
    assert st == dict(records=15, taking_part=12, groups=3, heads_marked=3, tails_marked=3, set_entries=3)


def test_narrow_digest_marks_more_never_fewer():
    for s in mi.SETS:
        wide, narrow = mm.mark(s["records"]), mm.mark(s["records"], digest_bits=1)
        assert all(n & 0x400 for w, n in zip(wide, narrow) if w & 0x400)
