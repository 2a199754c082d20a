"""Plain numpy models of the three device primitives (seeksv_amd/csrc/scan.h, radix_sort.h, tile_sort.h) and the inputs their tests use
(tests only; importable without a GPU).  Everything here is integers and orders, so the models are exact: tests/test_primitives_gpu.py
compares the kernels with them bit for bit, and tests/test_primitives_model.py holds every input to the property its builder states.

The sizes are parameters (the window W, the tile): the GPU tests pass the constants the test library reports, the CPU tests the same
values as literals of their own (WS_W, WS_TILE below mirror tile_sort.h and are checked against the library on the GPU)."""
import numpy as np

WS_W, WS_TILE = 32, 1024          # tile_sort.h (held against the library's constants by test_primitives_gpu.py::test_constants)
U64_MAX = np.uint64(2 ** 64 - 1)
UNWRITTEN = np.uint32(0xffffffff)  # sort_nearly_sorted fills val_out with this before the ranks are stored

# ---- exclusive_scan -------------------------------------------------------------------------------------------------

SCAN_PAIRS = {  # name -> (input dtype, output dtype)
    "u16_u32": (np.uint16, np.uint32), "u32_u32": (np.uint32, np.uint32), "u32_u64": (np.uint32, np.uint64),
    "u64_u64": (np.uint64, np.uint64), "i32_i64": (np.int32, np.int64),
}


def scan_model(x, out_dtype, carry_in=0):
    """-> (out, total): out[i] = carry_in + x[0] + ... + x[i - 1] and total = carry_in + sum(x), both reduced modulo the width of out_dtype.
    The sums are formed modulo 2^64 (np.uint64 wraps; a negative input is its two's complement) and then cut to the output width, which is
    the same residue."""
    out_dtype = np.dtype(out_dtype)
    x = np.asarray(x)
    wide = x.astype(np.int64).view(np.uint64) if x.dtype.kind == "i" else x.astype(np.uint64)
    carry = np.uint64(int(carry_in) % 2 ** 64)
    with np.errstate(over="ignore"):
        inc = np.cumsum(wide, dtype=np.uint64) + carry
    ex = np.empty(len(wide), np.uint64)
    if len(wide):
        ex[0] = carry
        ex[1:] = inc[:-1]
    total = int(inc[-1]) if len(wide) else int(carry)
    bits = 8 * out_dtype.itemsize
    total %= 2 ** bits
    if out_dtype.kind == "i":
        out = ex.view(np.int64).astype(out_dtype)
        total = total - 2 ** bits if total >= 2 ** (bits - 1) else total
    else:
        out = ex.astype(out_dtype)   # keeps the low bits
    return out, total


def scan_model_python(x, out_dtype, carry_in=0):
    """the same with Python integers, element by element: what scan_model is held against on small inputs"""
    out_dtype = np.dtype(out_dtype)
    bits = 8 * out_dtype.itemsize

    def cut(v):
        v %= 2 ** bits
        return v - 2 ** bits if out_dtype.kind == "i" and v >= 2 ** (bits - 1) else v
    s, out = int(carry_in), []
    for v in np.asarray(x).tolist():
        out.append(cut(s))
        s += int(v)
    return np.array(out, out_dtype), cut(s)


def scan_values(name, n, rng):
    """random inputs over the WHOLE input range of the pair (u32 sums wrap several times), u64 inputs below 2^40 (sums pass 2^32 at once
    and stay below 2^64 for any n the tests use), i32 inputs of both signs"""
    tin, _ = SCAN_PAIRS[name]
    if name == "u64_u64":
        return rng.integers(0, 2 ** 40, n, dtype=np.uint64, endpoint=True)
    info = np.iinfo(tin)
    return rng.integers(info.min, info.max, n, dtype=tin, endpoint=True)


def one_hot_positions(n, scan_tile, thread_run=8, wave=64, block=256):
    """the places where a single 1 crosses an edge of the scan kernels: a thread's run of 8, a lane / a wavefront of the strided reduce
    (64, 256), a wavefront of the blocked downsweep (64 * 8), a tile, the last element"""
    want = [0, thread_run - 1, thread_run, wave - 1, wave, block - 1, block, wave * thread_run - 1, wave * thread_run,
            scan_tile - 1, scan_tile, scan_tile + 1, 2 * scan_tile - 1, 2 * scan_tile, n - 1]
    return sorted({p for p in want if 0 <= p < n})


# ---- radix_sort_pairs -----------------------------------------------------------------------------------------------

def radix_passes(key_bits):
    return (key_bits + 7) // 8 if key_bits > 0 else 0


def radix_model(keys, vals, key_bits):
    """-> (keys, vals, buffer index): a stable sort by the low 8 * ceil(key_bits / 8) bits (the sort runs whole 8-bit passes); the bits
    above travel with the key; the result lies in buffer (number of passes) & 1"""
    keys, vals = np.asarray(keys, np.uint64), np.asarray(vals, np.uint32)
    passes = radix_passes(key_bits)
    mask = U64_MAX if passes >= 8 else np.uint64((1 << (8 * passes)) - 1)
    order = np.argsort(keys & mask, kind="stable")
    return keys[order], vals[order], (passes & 1 if len(keys) else 0)


RADIX_KEY_KINDS = ("uniform", "equal", "alternating", "eight", "top_byte", "high_noise")


def radix_keys(kind, n, rng):
    """uniform: 64 random bits.  equal: one key (every pass: one digit holds whole tiles).  alternating: two keys that differ in every
    byte, lane by lane (a wavefront's match masks are two interleaved halves in every pass).  eight: eight distinct random keys (long runs of equal
    keys: stability shows in the values).  top_byte: keys that differ only in bits 56-63.  high_noise: four values in the low byte under
    56 random bits (with key_bits <= 8 the random bits lie above the sorted range and must come through untouched and unused)."""
    if kind == "uniform":
        return rng.integers(0, 2 ** 64 - 1, n, dtype=np.uint64, endpoint=True)
    if kind == "equal":
        return np.full(n, 0x0123456789abcdef, np.uint64)
    if kind == "alternating":
        return np.where(np.arange(n) & 1, np.uint64(0x3c3c3c3c3c3c3c3c), np.uint64(0xc3c3c3c3c3c3c3c3))
    if kind == "eight":
        return rng.integers(0, 2 ** 64 - 1, 8, dtype=np.uint64, endpoint=True)[rng.integers(0, 8, n)]
    if kind == "top_byte":
        return (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x00a5a5a5a5a5a5a5)
    if kind == "high_noise":
        return (rng.integers(0, 2 ** 56, n, dtype=np.uint64) << np.uint64(8)) | np.array([0, 1, 128, 255], np.uint64)[rng.integers(0, 4, n)]
    raise ValueError(kind)


def radix_vals(kind, n, rng):
    """iota (the callers' ordinals), or random u32 with 0xffffffff among them"""
    if kind == "iota":
        return np.arange(n, dtype=np.uint32)
    v = rng.integers(0, 2 ** 32 - 1, n, dtype=np.uint32, endpoint=True)
    v[::7] = 0xffffffff
    return v


# ---- sort_nearly_sorted ---------------------------------------------------------------------------------------------

def _greater(ka, va, kb, vb):
    """ts_greater: (ka, va) > (kb, vb)"""
    return (ka > kb) | ((ka == kb) & (va > vb))


def window_shifts(keys, vals, w=WS_W):
    """k_window_rank_sort, element by element: element g moves down by the number of elements at g - w .. g - 1 that are greater and up by
    the number at g + 1 .. g + w that are smaller (places outside the list do not exist)"""
    keys, vals = np.asarray(keys, np.uint64), np.asarray(vals, np.uint32)
    n = len(keys)
    shift = np.zeros(n, np.int64)
    for d in range(1, min(w, n - 1) + 1):
        inv = _greater(keys[:-d], vals[:-d], keys[d:], vals[d:])   # inv[g]: the pair (g, g + d) is inverted
        shift[d:] -= inv                                           # the later one of the pair: an earlier element is greater
        shift[:-d] += inv                                          # the earlier one: a later element is smaller
    return shift


def window_sort_model(keys, vals, w=WS_W):
    """sort_nearly_sorted -> (flag, keys_out, vals_out).  Slots that no element lands on keep val 0xffffffff (and an undefined key); the flag
    (k_check_sorted_pairs) is raised when a slot holds 0xffffffff or the list is not strictly increasing by (key, value).  Two elements on one
    slot leave another slot empty, so the flag does not depend on which of the two stores wins; the arrays are meaningful where flag == 0."""
    keys, vals = np.asarray(keys, np.uint64), np.asarray(vals, np.uint32)
    n = len(keys)
    dst = np.arange(n) + window_shifts(keys, vals, w)
    assert n == 0 or (dst.min() >= 0 and dst.max() < n)   # a shift never leaves the list: at most g greater before, n - 1 - g smaller behind
    ko, vo = np.zeros(n, np.uint64), np.full(n, UNWRITTEN, np.uint32)
    ko[dst], vo[dst] = keys, vals
    flag = len(np.unique(dst)) != n or bool((vo == UNWRITTEN).any()) or bool((~_greater(ko[1:], vo[1:], ko[:-1], vo[:-1])).any())
    return int(flag), ko, vo


def sorted_pairs(keys, vals):
    """the list in (key, value) order"""
    order = np.lexsort((vals, keys))
    return np.asarray(keys, np.uint64)[order], np.asarray(vals, np.uint32)[order]


def max_inversion_distance(keys, vals):
    """the largest j - i over pairs i < j with element i > element j (0 for a sorted list): for every j the FIRST earlier element that is
    greater, which is where the running maximum first exceeds element j"""
    keys, vals = np.asarray(keys, np.uint64), np.asarray(vals, np.uint32)
    n = len(keys)
    if n < 2:
        return 0
    rank = np.empty(n, np.int64)                       # dense ranks: equal pairs get equal ranks
    order = np.lexsort((vals, keys))
    ks, vs = keys[order], vals[order]
    rank[order] = np.cumsum(np.concatenate(([0], (ks[1:] != ks[:-1]) | (vs[1:] != vs[:-1]))))
    run = np.maximum.accumulate(rank)
    first = np.searchsorted(run, rank, side="right")   # first i with run[i] > rank[j]
    d = np.arange(n) - first
    return int(max(d.max(), 0))


def max_displacement(keys, vals):
    """the largest distance of an element from its place in the sorted list (elements are distinct in the lists this is used on)"""
    order = np.lexsort((vals, keys))
    return int(np.abs(order - np.arange(len(order))).max()) if len(order) else 0


def _base_list(n, rng, dup=True):
    """a sorted list of n distinct (key, value) pairs: keys non-decreasing (with runs of equal keys when dup), values the ordinals"""
    step = rng.integers(0 if dup else 1, 4, n, dtype=np.uint64)
    return np.cumsum(step, dtype=np.uint64) + np.uint64(1000), np.arange(n, dtype=np.uint32)


def _block_bounds(n, w, tile):
    """cuts of [0, n) into blocks of at most w + 1 elements such that no cut falls on a multiple of `tile`: every multiple of the tile
    inside the list lies strictly inside a block"""
    cuts, p = [0], 0
    while p < n:
        s = w + 1
        if (p + s) % tile == 0:
            s -= 1
        p = min(p + s, n)
        cuts.append(p)
    assert all(c % tile or c in (0, n) for c in cuts) and max(np.diff(cuts), default=0) <= w + 1
    return cuts


def _shuffle_blocks(keys, vals, cuts, rng, reverse=False):
    keys, vals = keys.copy(), vals.copy()
    for a, b in zip(cuts[:-1], cuts[1:]):
        p = np.arange(a, b)[::-1] if reverse else a + rng.permutation(b - a)
        keys[a:b], vals[a:b] = keys[p], vals[p]
    return keys, vals


def ws_sorted(n, rng, w=WS_W, tile=WS_TILE):
    """PROPERTY: strictly increasing by (key, value) - no inverted pair at all"""
    return _base_list(n, rng)


def ws_block_shuffled(n, rng, w=WS_W, tile=WS_TILE):
    """PROPERTY: a sorted list permuted inside blocks of at most w + 1 elements, so every inverted pair lies inside a block: at most w places
    apart.  A block straddles every multiple of the tile."""
    k, v = _base_list(n, rng)
    return _shuffle_blocks(k, v, _block_bounds(n, w, tile), rng)


def ws_block_reversed(n, rng, w=WS_W, tile=WS_TILE):
    """PROPERTY: as ws_block_shuffled with every block reversed: each block's first and last element are inverted exactly w places apart
    (the last window slot on either side decides)"""
    k, v = _base_list(n, rng, dup=False)
    return _shuffle_blocks(k, v, _block_bounds(n, w, tile), rng, reverse=True)


def ws_extreme_keys(n, rng, w=WS_W, tile=WS_TILE, kind="zeros_max"):
    """PROPERTY: as ws_block_shuffled, with the keys 0 and 2^64 - 1 only: all 0 (`zeros`), all 2^64 - 1 (`max`), or 0 in the first half and
    2^64 - 1 in the second (`zeros_max`).  Values start at 1: a zero-filled place outside the list is the pair (0, 0), smaller than every
    element - counted behind the list's end it would move the last elements up."""
    k = {"zeros": np.zeros(n, np.uint64), "max": np.full(n, U64_MAX), "zeros_max": np.where(np.arange(n) < n // 2, np.uint64(0), U64_MAX)}[kind]
    v = np.arange(1, n + 1, dtype=np.uint32)
    return _shuffle_blocks(k, v, _block_bounds(n, w, tile), rng)


def ws_equal_runs(n, rng, w=WS_W, tile=WS_TILE):
    """PROPERTY: keys non-decreasing, constant over each block of at most w + 1 elements and different from block to block; the values of
    a block distinct and in random order.  Every inverted pair is a pair of equal keys inside one block: the value decides."""
    cuts = _block_bounds(n, w, tile)
    k = np.repeat(np.arange(len(cuts) - 1, dtype=np.uint64) * np.uint64(3) + np.uint64(5), np.diff(cuts))
    return _shuffle_blocks(k, np.arange(n, dtype=np.uint32), cuts, rng)


WS_GUARANTEED = {  # name -> builder(n, rng, w, tile): every inverted pair at most w places apart, all (key, value) pairs distinct
    "sorted": ws_sorted, "block_shuffled": ws_block_shuffled, "block_reversed": ws_block_reversed, "equal_runs": ws_equal_runs,
    "zeros": lambda n, rng, w=WS_W, tile=WS_TILE: ws_extreme_keys(n, rng, w, tile, "zeros"),
    "max": lambda n, rng, w=WS_W, tile=WS_TILE: ws_extreme_keys(n, rng, w, tile, "max"),
    "zeros_max": lambda n, rng, w=WS_W, tile=WS_TILE: ws_extreme_keys(n, rng, w, tile, "zeros_max"),
}


def ws_far_swap(n, at, w=WS_W):
    """PROPERTY: strictly increasing but for ONE swap of the elements at `at` and `at + w + 1`: that pair is inverted w + 1 places apart"""
    k, v = np.arange(n, dtype=np.uint64) * np.uint64(2) + np.uint64(10), np.arange(n, dtype=np.uint32)
    a, b = at, at + w + 1
    assert 0 <= a and b < n
    k[[a, b]], v[[a, b]] = k[[b, a]], v[[b, a]]
    return k, v


def ws_displacement_counter_example(n=200, w=WS_W):
    """PROPERTY: no element is w or more places from its sorted position, and yet one pair is inverted 50 places apart.
    The list [31.5, 0..24, 26..30, 32..50, 25.5, 51..n) (keys doubled to make them integers): 31.5 stands 31 places early, 25.5
    stands 24 places late, everything between them moved by one place at most - and 31.5 > 25.5 are 50 places apart, outside each other's
    window.  (Written for w = 32.)"""
    assert w == 32 and n > 60
    k = [63] + [2 * x for x in range(0, 25)] + [2 * x for x in range(26, 31)] + [2 * x for x in range(32, 51)] + [51] + [2 * x for x in range(51, n)]
    return np.array(k, np.uint64), np.arange(len(k), dtype=np.uint32)


def ws_reversed_run(n, start, w=WS_W):
    """PROPERTY: strictly increasing but for a run of 2 w elements from `start` that is reversed: its ends are inverted 2 w - 1 places apart"""
    k, v = np.arange(n, dtype=np.uint64) * np.uint64(2) + np.uint64(10), np.arange(n, dtype=np.uint32)
    assert 0 <= start and start + 2 * w <= n
    k[start:start + 2 * w], v[start:start + 2 * w] = k[start:start + 2 * w][::-1].copy(), v[start:start + 2 * w][::-1].copy()
    return k, v


def ws_random_swaps(n, swaps, rng):
    """a strictly increasing list after `swaps` swaps of random pairs of places, however far apart (no property promised: flag or sorted)"""
    k, v = _base_list(n, rng, dup=False)
    for _ in range(swaps):
        a, b = rng.integers(0, n, 2)
        k[[a, b]], v[[a, b]] = k[[b, a]], v[[b, a]]
    return k, v
