"""-m gpu: exclusive_scan (scan.h), radix_sort_pairs (radix_sort.h) and sort_nearly_sorted (tile_sort.h) called DIRECTLY, through the
test-only library of tests/native/prim_check.hip (`make primcheck`), and compared bit for bit with the plain models of
tests/primitives_model.py (integers and orders: no tolerance anywhere).  The whole passes reach these primitives only with the sizes and
values their fixtures happen to produce; here every size at which the code takes another path is called by name, derived from the
constants the library reports: the direct and the three-kernel form of the scan, one, two and three chunks of the scan of the sums, a
second trip over the raw sums, partial tiles and wavefronts of the sorts.

Every output and scratch array is followed by 64 guard elements that must come back untouched; scratch arrays have exactly the size the
headers ask for (scan_scratch_elems(n), 256 * rs_tiles(n)), as several callers allocate them.

The scan's three-kernel path UNDER the radix sort (a histogram of more than SCAN_DIRECT_TILES * SCAN_TILE counters) needs more than 67 M
keys and is not reachable in seconds: the scan tests below cover that path on its own, at D*T + 1 and 2*C*T + 1 elements."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import primitives_model as M
from seeksv_amd import _abi

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_BYTE = 0xA5
_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(_abi.LIBDIR, "libseeksv_primcheck.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make primcheck`")
        L = C.CDLL(path)
        V, I64, U64 = C.c_void_p, C.c_int64, C.c_uint64
        L.ssvp_const.argtypes, L.ssvp_const.restype = [C.c_int], I64
        L.ssvp_scan_scratch_elems.argtypes, L.ssvp_scan_scratch_elems.restype = [I64], I64
        L.ssvp_rs_tiles.argtypes, L.ssvp_rs_tiles.restype = [I64], I64
        for name in M.SCAN_PAIRS:
            getattr(L, "ssvp_scan_" + name).argtypes = [V, V, I64, U64, V, V]
        L.ssvp_scan_sums_u32.argtypes = L.ssvp_scan_sums_u64.argtypes = [V, I64, U64, V]
        L.ssvp_scan_sums_lists_u64.argtypes = [V, C.c_int, I64, I64]
        L.ssvp_radix_sort_pairs.argtypes = [V, V, V, V, I64, C.c_int, V, V]
        L.ssvp_sort_nearly_sorted.argtypes = [V, V, V, V, I64, V]
        _lib = L
    return _lib


class K:
    """the constants of the three headers, as the library was compiled with them"""
    def __init__(self):
        self.T, self.D, self.C, self.RS_TILE, self.W, self.WS_TILE = (int(lib().ssvp_const(i)) for i in range(6))


@pytest.fixture(scope="module")
def k():
    return K()


def _rng(*seed):
    return np.random.default_rng([0x9f1d] + [int(s) for s in seed])


class Dev:
    """`n` elements of `dtype` on the device (from `data`, or the guard pattern) followed by GUARD guard elements; extra: further elements
    in front of the guards that belong to the array (the `total` of an in-place scan)"""
    def __init__(self, dtype, n, data=None, extra=0):
        self.dtype, self.n, self.size = np.dtype(dtype), n, n + extra
        host = np.full((self.size + GUARD) * self.dtype.itemsize, GUARD_BYTE, np.uint8)
        if data is not None:
            assert len(data) == n and np.asarray(data).dtype == self.dtype
            host[:n * self.dtype.itemsize] = np.ascontiguousarray(data).view(np.uint8)
        self.t = torch.from_numpy(host).cuda()
        self._host = None

    @property
    def ptr(self):
        return self.t.data_ptr()

    def at(self, i):
        return self.ptr + i * self.dtype.itemsize

    def host(self):
        if self._host is None:
            self._host = self.t.cpu().numpy().view(self.dtype)
        return self._host

    def get(self, n=None):
        return self.host()[:self.size if n is None else n]

    def guards_intact(self):
        return bool((self.host()[self.size:].view(np.uint8) == GUARD_BYTE).all())

    def untouched(self):
        """the guard pattern everywhere: nothing was written at all"""
        return bool((self.host().view(np.uint8) == GUARD_BYTE).all())


def _pattern(dtype):
    return int(np.full(1, GUARD_BYTE, np.uint8).repeat(np.dtype(dtype).itemsize).view(dtype)[0])


def test_constants(k):
    """the sizes below are derived from these; the model's own copies of the window and its tile are the library's"""
    assert (k.W, k.WS_TILE) == (M.WS_W, M.WS_TILE)
    assert k.T > 0 and k.D > 0 and k.C > 0 and k.RS_TILE > 0 and lib().ssvp_const(6) == -1
    for n in (0, 1, k.T, k.T + 1):
        assert lib().ssvp_scan_scratch_elems(n) == -(-n // k.T) + 1
        assert lib().ssvp_rs_tiles(n) == -(-n // k.RS_TILE)


# ---- exclusive_scan -------------------------------------------------------------------------------------------------

def _carry_for(tout):
    return 0xfffffff0 if np.dtype(tout).itemsize == 4 else 2 ** 40 + 7


def _run_scan(name, x, carry, total_form, in_place=False):
    """one exclusive_scan call -> nothing; asserts out, total and every guard.  total_form: "null" | "separate" | "behind" (out + n)"""
    tin, tout = M.SCAN_PAIRS[name]
    n = len(x)
    want, want_total = M.scan_model(x, tout, carry)
    behind = total_form == "behind"
    if in_place:
        assert np.dtype(tin) == np.dtype(tout)
        out = Dev(tout, n, x, extra=1 if behind else 0)
        src = out
    else:
        src = Dev(tin, n, x)
        out = Dev(tout, n, extra=1 if behind else 0)
    scratch = Dev(tout, int(lib().ssvp_scan_scratch_elems(n)))
    total = Dev(tout, 1) if total_form == "separate" else None
    tp = {"null": None, "separate": total and total.ptr, "behind": out.at(n)}[total_form]
    rc = getattr(lib(), "ssvp_scan_" + name)(src.ptr, out.ptr, n, carry, scratch.ptr, tp)
    assert rc == 0, rc
    what = (name, n, carry, total_form, in_place)
    got = out.get(n)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {n} wrong, first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}")
    assert out.guards_intact() and scratch.guards_intact() and (in_place or src.guards_intact()), what
    if total_form == "separate":
        assert int(total.get()[0]) == want_total and total.guards_intact(), what
    elif behind:
        assert int(out.get()[n]) == want_total, what
    if not in_place and n:
        assert np.array_equal(src.get(n), x), what
    return out, scratch


def _small_sizes(k):
    return [0, 1, 255, 256, 257, k.T - 1, k.T, k.T + 1, 257 * k.T + 3]


@pytest.mark.parametrize("size", range(9), ids=["0", "1", "255", "256", "257", "T-1", "T", "T+1", "257T+3"])
@pytest.mark.parametrize("name", sorted(M.SCAN_PAIRS))
def test_exclusive_scan_sizes_and_forms(k, name, size):
    """random values over the whole input range: carry 0 with a separate total, a carry with no total, a carry with the total behind the
    output, and (same type in and out) in place with the total behind the array.  257 T + 3 gives the last workgroups a second trip over the
    raw sums of the tiles before them."""
    n = _small_sizes(k)[size]
    tin, tout = M.SCAN_PAIRS[name]
    x = M.scan_values(name, n, _rng(1, n))
    carry = _carry_for(tout)
    _run_scan(name, x, 0, "separate")
    _run_scan(name, x, carry, "null")
    _run_scan(name, x, carry, "behind")
    if np.dtype(tin) == np.dtype(tout):
        _run_scan(name, x, carry, "behind", in_place=True)
        _run_scan(name, x, 0, "null", in_place=True)


@pytest.mark.parametrize("name", sorted(M.SCAN_PAIRS))
def test_exclusive_scan_of_nothing_writes_the_carry_alone(k, name):
    tin, tout = M.SCAN_PAIRS[name]
    carry = _carry_for(tout)
    for form in ("null", "separate", "behind"):
        out, scratch = _run_scan(name, np.zeros(0, tin), carry, form)
        assert scratch.untouched()                       # (its one element too)
        assert form == "behind" or out.untouched()


@pytest.mark.parametrize("name", sorted(M.SCAN_PAIRS))
def test_exclusive_scan_one_hot(k, name):
    """a single 1 (-1 for the signed pair) at every edge: out is 0 up to it and the 1 behind it"""
    tin, tout = M.SCAN_PAIRS[name]
    n = 3 * k.T + 5
    for p in M.one_hot_positions(n, k.T):
        x = np.zeros(n, tin)
        x[p] = -1 if np.dtype(tin).kind == "i" else 1
        _run_scan(name, x, 0, "separate")
    x = np.zeros(n, tin)
    x[k.T] = 1
    _run_scan(name, x, _carry_for(tout), "behind", in_place=np.dtype(tin) == np.dtype(tout))


@pytest.mark.parametrize("name,in_place", [("u32_u32", True), ("u32_u64", False)])
@pytest.mark.parametrize("over", [0, 1], ids=["last-direct", "first-three-kernel"])
def test_exclusive_scan_around_the_direct_limit(k, name, in_place, over):
    """D * T elements: the last size k_scan_down_direct serves (D raw sums per workgroup); D * T + 1: the first that goes through
    k_scan_sums and k_scan_down - D + 1 sums, so the second chunk of the scan of the sums holds exactly one"""
    n = k.D * k.T + over
    assert (-(-n // k.T) > k.D) == bool(over) and -(-n // k.T) - k.C * (k.D // k.C) == over
    x = M.scan_values(name, n, _rng(2, over))
    _run_scan(name, x, _carry_for(M.SCAN_PAIRS[name][1]), "behind", in_place=in_place)


def test_exclusive_scan_three_chunks_of_sums(k):
    """u16 -> u32 over 2 C T + 1 elements: 2 C + 1 tile sums, three chunks in k_scan_sums (the next chunk prefetched while this one is scanned)"""
    n = 2 * k.C * k.T + 1
    assert -(-n // k.T) == 2 * k.C + 1 > k.D
    x = M.scan_values("u16_u32", n, _rng(3))
    _run_scan("u16_u32", x, 0xfffffff0, "separate")


# ---- k_scan_sums, k_scan_sums_lists ---------------------------------------------------------------------------------

def _sums_sizes(k):
    c = k.C
    return [0, 1, 15, 16, 17, 255, 256, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 25000]


SUMS_IDS = ["0", "1", "15", "16", "17", "255", "256", "C-1", "C", "C+1", "2C-1", "2C", "2C+1", "25000"]


def _sums_values(dtype, m, rng):
    return M.scan_values("u32_u32" if np.dtype(dtype).itemsize == 4 else "u64_u64", m, rng)


@pytest.mark.parametrize("size", range(14), ids=SUMS_IDS)
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["u32", "u64"])
def test_scan_sums(k, dtype, size):
    """one workgroup, in place, chunk by chunk: with and without carry, with and without a total"""
    m = _sums_sizes(k)[size]
    x = _sums_values(dtype, m, _rng(4, m))
    fn = lib().ssvp_scan_sums_u32 if np.dtype(dtype).itemsize == 4 else lib().ssvp_scan_sums_u64
    for carry in (0, _carry_for(dtype)):
        want, want_total = M.scan_model(x, dtype, carry)
        for with_total in (False, True):
            sums, total = Dev(dtype, m, x), Dev(dtype, 1)
            assert fn(sums.ptr, m, carry, total.ptr if with_total else None) == 0
            assert np.array_equal(sums.get(), want) and sums.guards_intact(), (m, carry, with_total)
            assert (int(total.get()[0]) == want_total and total.guards_intact()) if with_total else total.untouched(), (m, carry, with_total)


@pytest.mark.parametrize("size", range(1, 14), ids=SUMS_IDS[1:])
def test_scan_sums_lists(k, size):
    """three lists, one workgroup each, carry 0 and no total: `stride` elements apart, the gap between two lists untouched"""
    m = _sums_sizes(k)[size]
    for stride in (m, m + 5):
        rng = _rng(5, m, stride)
        lists = [_sums_values(np.uint64, m, rng) for _ in range(3)]
        flat = np.full(2 * stride + m, _pattern(np.uint64), np.uint64)
        want = flat.copy()
        for i, x in enumerate(lists):
            flat[i * stride:i * stride + m] = x
            want[i * stride:i * stride + m] = M.scan_model(x, np.uint64, 0)[0]
        buf = Dev(np.uint64, len(flat), flat)
        assert lib().ssvp_scan_sums_lists_u64(buf.ptr, 3, m, stride) == 0
        assert np.array_equal(buf.get(), want) and buf.guards_intact(), (m, stride)


# ---- radix_sort_pairs -----------------------------------------------------------------------------------------------

def _radix_sizes(k):
    r = k.RS_TILE
    return [0, 1, 63, 64, 65, 255, 256, 257, r - 1, r, r + 1, 5 * r + 77, 40 * r + 1]


RADIX_IDS = ["0", "1", "63", "64", "65", "255", "256", "257", "R-1", "R", "R+1", "5R+77", "40R+1"]


@pytest.mark.parametrize("key_bits", [1, 8, 9, 33, 41, 64])
@pytest.mark.parametrize("size", range(13), ids=RADIX_IDS)
def test_radix_sort_pairs(k, size, key_bits):
    """every key distribution x (iota | random values): the returned buffers hold the stable sort by the low whole bytes of key_bits, with
    the full keys; the buffer index is the parity of the passes.  40 R + 1 keys: a histogram of several scan tiles."""
    n = _radix_sizes(k)[size]
    nt = int(lib().ssvp_rs_tiles(n))
    for kind in M.RADIX_KEY_KINDS:
        for vkind in ("iota", "random"):
            rng = _rng(6, n, key_bits, M.RADIX_KEY_KINDS.index(kind), vkind == "iota")
            keys, vals = M.radix_keys(kind, n, rng), M.radix_vals(vkind, n, rng)
            wk, wv, widx = M.radix_model(keys, vals, key_bits)
            kb = [Dev(np.uint64, n, keys), Dev(np.uint64, n)]
            vb = [Dev(np.uint32, n, vals), Dev(np.uint32, n)]
            ghist = Dev(np.uint32, 256 * nt)
            scratch = Dev(np.uint32, int(lib().ssvp_scan_scratch_elems(256 * nt)))
            r = lib().ssvp_radix_sort_pairs(kb[0].ptr, kb[1].ptr, vb[0].ptr, vb[1].ptr, n, key_bits, ghist.ptr, scratch.ptr)
            what = (n, key_bits, kind, vkind)
            assert r == widx, what
            gk, gv = kb[r].get(), vb[r].get()
            if not (np.array_equal(gk, wk) and np.array_equal(gv, wv)):
                bad = np.flatnonzero((gk != wk) | (gv != wv))
                raise AssertionError(f"{what}: {len(bad)} of {n} pairs wrong, first at {bad[0]}: got ({int(gk[bad[0]]):#x}, {int(gv[bad[0]])}) want ({int(wk[bad[0]]):#x}, {int(wv[bad[0]])})")
            assert all(b.guards_intact() for b in kb + vb + [ghist, scratch]), what
            if n == 0:
                assert kb[1].untouched() and vb[1].untouched() and ghist.untouched() and scratch.untouched()


# ---- sort_nearly_sorted ---------------------------------------------------------------------------------------------

def _window_sort(keys, vals):
    """-> (flag, keys_out, vals_out) of the device, guards checked"""
    n = len(keys)
    ki, vi, ko, vo = Dev(np.uint64, n, keys), Dev(np.uint32, n, vals), Dev(np.uint64, n), Dev(np.uint32, n)
    flag = Dev(np.int32, 1, np.zeros(1, np.int32))
    assert lib().ssvp_sort_nearly_sorted(ki.ptr, vi.ptr, ko.ptr, vo.ptr, n, flag.ptr) == 0
    assert ko.guards_intact() and vo.guards_intact() and flag.guards_intact()
    assert np.array_equal(ki.get(), keys) and np.array_equal(vi.get(), vals)
    return int(flag.get()[0]), ko.get(), vo.get()


def _ws_sizes(k):
    return [1, 2, k.W, k.W + 1, k.WS_TILE - 1, k.WS_TILE, k.WS_TILE + 1, 3 * k.WS_TILE + k.W // 2]


@pytest.mark.parametrize("size", range(8), ids=["1", "2", "W", "W+1", "TILE-1", "TILE", "TILE+1", "3TILE+W/2"])
@pytest.mark.parametrize("name", sorted(M.WS_GUARANTEED))
def test_window_sort_of_lists_it_guarantees(k, name, size):
    """every inverted pair at most W places apart (tests/test_primitives_model.py holds the builders to that): no flag, and the sorted list
    - these lists never take the radix sort behind the window sort"""
    n = _ws_sizes(k)[size]
    for seed in range(3):
        keys, vals = M.WS_GUARANTEED[name](n, _rng(7, n, seed), k.W, k.WS_TILE)
        mflag, mk, mv = M.window_sort_model(keys, vals, k.W)
        sk, sv = M.sorted_pairs(keys, vals)
        assert mflag == 0 and np.array_equal(mk, sk) and np.array_equal(mv, sv)
        flag, gk, gv = _window_sort(keys, vals)
        assert flag == 0, (name, n, seed)
        assert np.array_equal(gk, mk) and np.array_equal(gv, mv), (name, n, seed)


def _must_flag(k):
    t, w = k.WS_TILE, k.W
    return {
        "swap_at_start": M.ws_far_swap(w + 2, 0, w), "swap_inside": M.ws_far_swap(200, 77, w),
        "swap_across_tile_edge": M.ws_far_swap(t + 100, t - 1, w), "swap_up_to_tile_edge": M.ws_far_swap(t + 100, t - w - 1, w),
        "swap_at_end": M.ws_far_swap(2 * t + 7, 2 * t + 7 - w - 2, w),
        "displacement_31": M.ws_displacement_counter_example(200, w),
        "displacement_31_at_tile_edge": _shifted(M.ws_displacement_counter_example(200, w), t - 20),
        "reversed_run_across_tile_edge": M.ws_reversed_run(t + 100, t - w, w), "reversed_run_is_the_list": M.ws_reversed_run(2 * w, 0, w),
    }


def _shifted(pair, lead):
    """`lead` smaller elements in front of the list"""
    keys, vals = pair
    return (np.concatenate([np.zeros(lead, np.uint64), keys + np.uint64(1)]),
            np.concatenate([np.arange(lead, dtype=np.uint32), vals + np.uint32(lead)]))


@pytest.mark.parametrize("name", ["swap_at_start", "swap_inside", "swap_across_tile_edge", "swap_up_to_tile_edge", "swap_at_end", "displacement_31",
                                  "displacement_31_at_tile_edge", "reversed_run_across_tile_edge", "reversed_run_is_the_list"])
def test_window_sort_flags_what_it_cannot_sort(k, name):
    """an inverted pair more than W places apart: the model raises the flag, and so must the device (the output is not compared: two
    elements store to one slot).  `displacement_31`: no element 32 or more places from its sorted position, and still not sortable."""
    keys, vals = _must_flag(k)[name]
    assert M.max_inversion_distance(keys, vals) > k.W
    assert M.window_sort_model(keys, vals, k.W)[0] == 1
    assert _window_sort(keys, vals)[0] == 1


def test_window_sort_flag_is_the_models_on_random_swaps(k):
    """lists with a few swaps at any distance: the same flag as the model for every one, and the sorted list wherever the flag is 0"""
    clean = flagged = 0
    for seed in range(60):
        rng = _rng(8, seed)
        n = int(rng.integers(2, 3 * k.WS_TILE))
        keys, vals = M.ws_random_swaps(n, int(rng.integers(0, 4)), rng)
        if seed % 3 == 0:       # swaps that stay inside the window
            keys, vals = M.ws_block_shuffled(n, rng, k.W, k.WS_TILE)
            a = int(rng.integers(0, n))
            b = min(n - 1, a + int(rng.integers(0, 2 * k.W)))
            keys[[a, b]], vals[[a, b]] = keys[[b, a]], vals[[b, a]]
        mflag, mk, mv = M.window_sort_model(keys, vals, k.W)
        flag, gk, gv = _window_sort(keys, vals)
        assert flag == mflag, seed
        if flag == 0:
            sk, sv = M.sorted_pairs(keys, vals)
            assert np.array_equal(gk, sk) and np.array_equal(gv, sv) and np.array_equal(gk, mk) and np.array_equal(gv, mv), seed
            clean += 1
        else:
            flagged += 1
    assert clean >= 10 and flagged >= 10
