"""CPU: the plain models of tests/primitives_model.py against slower restatements of themselves, and every input builder against the
property it states - what tests/test_primitives_gpu.py relies on when it compares the kernels with these models bit for bit."""
import numpy as np
import pytest

import primitives_model as M

W, TILE = M.WS_W, M.WS_TILE
WS_SIZES = [1, 2, W, W + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + W // 2]


def _rng(*seed):
    return np.random.default_rng([0x5ca9] + [int(s) for s in seed])


# ---- scan ----

@pytest.mark.parametrize("name", sorted(M.SCAN_PAIRS))
def test_scan_model_equals_python_integers(name):
    tin, tout = M.SCAN_PAIRS[name]
    for n, carry in ((0, 0), (0, 2 ** 40 + 7), (1, 0), (300, 0), (300, 0xfffffff0), (300, 2 ** 40 + 7)):
        if np.dtype(tout).itemsize == 4 and carry >= 2 ** 32:
            continue
        x = M.scan_values(name, n, _rng(1, n))
        out, total = M.scan_model(x, tout, carry)
        ref, ref_total = M.scan_model_python(x, tout, carry)
        assert out.dtype == np.dtype(tout) and np.array_equal(out, ref) and total == ref_total, (name, n, carry)


def test_scan_values_cover_what_the_gpu_tests_claim():
    """u32 sums wrap, u64 partial sums pass 2^32 (they go through the wave shuffles as two halves), i32 inputs have both signs"""
    x = M.scan_values("u32_u32", 4096, _rng(2))
    assert int(x.astype(np.uint64).sum()) > 100 * 2 ** 32
    y = M.scan_values("u64_u64", 64, _rng(3))
    assert int(y.max()) > 2 ** 32 and int(y.sum()) < 2 ** 64
    z = M.scan_values("i32_i64", 4096, _rng(4))
    assert z.min() < 0 < z.max()
    assert M.one_hot_positions(3 * 2048 + 5, 2048) == [0, 7, 8, 63, 64, 255, 256, 511, 512, 2047, 2048, 2049, 4095, 4096, 6148]


# ---- radix sort ----

@pytest.mark.parametrize("key_bits,passes", [(1, 1), (8, 1), (9, 2), (33, 5), (41, 6), (64, 8)])
def test_radix_model_is_a_stable_sort_of_whole_bytes(key_bits, passes):
    assert M.radix_passes(key_bits) == passes
    rng = _rng(5, key_bits)
    for kind in M.RADIX_KEY_KINDS:
        keys, vals = M.radix_keys(kind, 1500, rng), M.radix_vals("iota", 1500, rng)
        k, v, idx = M.radix_model(keys, vals, key_bits)
        assert idx == passes & 1
        low = [int(x) & ((1 << (8 * passes)) - 1) for x in keys]
        ref = sorted(range(1500), key=lambda i: low[i])      # Python's sort is stable
        assert np.array_equal(v, np.array(ref, np.uint32)) and np.array_equal(k, keys[ref]), kind
    assert M.radix_model(np.zeros(0, np.uint64), np.zeros(0, np.uint32), key_bits)[2] == 0


def test_radix_inputs_have_their_properties():
    rng = _rng(6)
    n = 5000
    assert len(np.unique(M.radix_keys("equal", n, rng))) == 1
    alt = M.radix_keys("alternating", n, rng)
    assert all(((int(alt[0]) >> s) & 255) != ((int(alt[1]) >> s) & 255) for s in range(0, 64, 8)) and np.array_equal(alt[2:], alt[:-2])
    assert len(np.unique(M.radix_keys("eight", n, rng))) == 8
    top = M.radix_keys("top_byte", n, rng)
    assert len(np.unique(top & np.uint64(2 ** 56 - 1))) == 1 and len(np.unique(top >> np.uint64(56))) > 200
    hn = M.radix_keys("high_noise", n, rng)
    assert set((hn & np.uint64(255)).tolist()) == {0, 1, 128, 255} and len(np.unique(hn >> np.uint64(8))) == n
    rv = M.radix_vals("random", n, rng)
    assert (rv == 0xffffffff).sum() >= n // 7 and np.array_equal(M.radix_vals("iota", n, rng), np.arange(n))


# ---- window sort ----

def _shifts_one_by_one(keys, vals, w):
    """k_window_rank_sort read literally, in Python integers"""
    e = list(zip(keys.tolist(), vals.tolist()))
    n = len(e)
    return [sum(e[j] < e[g] for j in range(g + 1, min(n, g + w + 1))) - sum(e[j] > e[g] for j in range(max(0, g - w), g)) for g in range(n)]


def test_window_shifts_equal_the_loop_over_every_element():
    rng = _rng(7)
    for n in (1, 2, 5, 70, 300):
        for swaps in (0, 3, 40):
            k, v = M.ws_random_swaps(n, swaps, rng)
            assert M.window_shifts(k, v, 32).tolist() == _shifts_one_by_one(k, v, 32)
            assert M.window_shifts(k, v, 4).tolist() == _shifts_one_by_one(k, v, 4)


def test_max_inversion_distance_equals_brute_force():
    rng = _rng(8)
    for n in (1, 2, 40, 150):
        for swaps in (0, 2, 30):
            k, v = M.ws_random_swaps(n, swaps, rng)
            e = list(zip(k.tolist(), v.tolist()))
            brute = max([j - i for i in range(n) for j in range(i + 1, n) if e[i] > e[j]], default=0)
            assert M.max_inversion_distance(k, v) == brute


@pytest.mark.parametrize("n", WS_SIZES)
@pytest.mark.parametrize("name", sorted(M.WS_GUARANTEED))
def test_guaranteed_inputs_have_every_inverted_pair_inside_the_window(name, n):
    """... and for them the model gives flag 0 and exactly the sorted list"""
    for seed in range(4):
        k, v = M.WS_GUARANTEED[name](n, _rng(9, n, seed), W, TILE)
        assert len(k) == n == len(v) and not (v == M.UNWRITTEN).any()
        assert len(set(zip(k.tolist(), v.tolist()))) == n
        assert M.max_inversion_distance(k, v) <= W
        flag, ko, vo = M.window_sort_model(k, v, W)
        order = np.lexsort((v, k))
        assert flag == 0 and np.array_equal(ko, k[order]) and np.array_equal(vo, v[order])
    if name == "block_reversed" and n > W:
        assert M.max_inversion_distance(k, v) == W      # the last window slot on either side is needed
    if name != "sorted" and n > 2:
        assert M.max_inversion_distance(k, v) > 0
    if name == "equal_runs" and n > 2:
        assert (np.diff(k.astype(np.int64)) >= 0).all() and (np.diff(v.astype(np.int64)) < 0).any()


def test_blocks_straddle_every_multiple_of_the_tile():
    for n in WS_SIZES + [5 * TILE, 33 * TILE + 7]:
        cuts = M._block_bounds(n, W, TILE)
        assert cuts[0] == 0 and cuts[-1] == n
        for m in range(TILE, n, TILE):
            assert m not in cuts
    k, v = M.ws_block_reversed(3 * TILE + W // 2, _rng(10), W, TILE)
    for m in (TILE, 2 * TILE, 3 * TILE):    # an inverted pair across every tile edge
        assert (k[m - 1], v[m - 1]) > (k[m], v[m])


def test_displacement_counter_example_raises_the_flag():
    """tile_sort.h used to promise exact ranks "if no element is WS_W or more places from its sorted position": this list has a maximum
    displacement of 31 and the window sort gets it wrong - the guarantee is about inverted PAIRS (here one is 50 places apart)"""
    k, v = M.ws_displacement_counter_example()
    assert M.max_displacement(k, v) == 31 < W
    assert M.max_inversion_distance(k, v) == 50
    flag, ko, vo = M.window_sort_model(k, v, W)
    assert flag == 1
    dst = np.arange(len(k)) + M.window_shifts(k, v, W)
    assert len(np.unique(dst)) < len(k)       # wrong ranks: two elements on one slot


def test_must_flag_inputs_raise_the_flag():
    for n, at in ((W + 2, 0), (200, 77), (TILE + 100, TILE - W - 1), (TILE + 100, TILE - 1)):
        k, v = M.ws_far_swap(n, at, W)
        assert M.max_inversion_distance(k, v) == W + 1 and M.window_sort_model(k, v, W)[0] == 1
    for n, start in ((2 * W, 0), (TILE + 100, TILE - W), (TILE + 100, TILE - 5)):
        k, v = M.ws_reversed_run(n, start, W)
        assert M.max_inversion_distance(k, v) == 2 * W - 1 and M.window_sort_model(k, v, W)[0] == 1


def test_flag_zero_always_means_the_sorted_list():
    """what makes the check sufficient: n stores into n slots with none left unwritten is a permutation, and a strictly increasing
    permutation of the input is the sorted list.  Held here on lists with a few long-range swaps: never a silent wrong result."""
    clean = flagged = 0
    for seed in range(300):
        rng = _rng(11, seed)
        n = int(rng.integers(2, 400))
        k, v = M.ws_random_swaps(n, int(rng.integers(0, 4)), rng)
        flag, ko, vo = M.window_sort_model(k, v, W)
        if flag == 0:
            sk, sv = M.sorted_pairs(k, v)
            assert np.array_equal(ko, sk) and np.array_equal(vo, sv), seed
            clean += 1
        else:
            assert M.max_inversion_distance(k, v) > W, seed    # a list the window covers is never flagged
            flagged += 1
    assert clean > 30 and flagged > 30
