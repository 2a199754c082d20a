// prim_check.hip - TESTS ONLY: the three device primitives every stage rests on (scan.h, radix_sort.h, tile_sort.h) behind C entry points of
// their own, so that tests/test_primitives_gpu.py can call them at sizes and in forms of its choice.  Nothing here is part of libseeksv_hip.so
// or of its ABI.  Every entry point takes raw device pointers, launches on the null stream, waits, and returns the HIP error code (0 = fine).
#include "scan.h"
#include "radix_sort.h"
#include "tile_sort.h"

using namespace ssv;

static hipError_t finish()
{
	hipError_t e = hipGetLastError();
	hipError_t s = hipStreamSynchronize(nullptr);
	return e != hipSuccess ? e : s;
}

extern "C" {

// which: 0 SCAN_TILE, 1 SCAN_DIRECT_TILES, 2 SCAN_SUMS_CHUNK, 3 RS_TILE, 4 WS_W, 5 WS_TILE; anything else -1
int64_t ssvp_const(int which)
{
	switch (which) {
	case 0: return SCAN_TILE;
	case 1: return SCAN_DIRECT_TILES;
	case 2: return SCAN_SUMS_CHUNK;
	case 3: return RS_TILE;
	case 4: return WS_W;
	case 5: return WS_TILE;
	}
	return -1;
}

int64_t ssvp_scan_scratch_elems(int64_t n) { return scan_scratch_elems(n); }
int64_t ssvp_rs_tiles(int64_t n) { return rs_tiles(n); }

#define SSVP_SCAN(NAME, TIN, TOUT)                                                                                         \
	int ssvp_scan_##NAME(const void *in, void *out, int64_t n, uint64_t carry_in, void *scratch, void *total)             \
	{                                                                                                                      \
		exclusive_scan<TIN, TOUT>(nullptr, (const TIN *)in, (TOUT *)out, n, (TOUT)carry_in, (TOUT *)scratch, (TOUT *)total); \
		return (int)finish();                                                                                              \
	}
SSVP_SCAN(u16_u32, uint16_t, uint32_t)
SSVP_SCAN(u32_u32, uint32_t, uint32_t)
SSVP_SCAN(u32_u64, uint32_t, uint64_t)
SSVP_SCAN(u64_u64, uint64_t, uint64_t)
SSVP_SCAN(i32_i64, int32_t, int64_t)
#undef SSVP_SCAN

int ssvp_scan_sums_u32(void *sums, int64_t m, uint64_t carry_in, void *total)
{
	k_scan_sums<uint32_t><<<1, BLOCK, 0, nullptr>>>((uint32_t *)sums, m, (uint32_t)carry_in, (uint32_t *)total);
	return (int)finish();
}

int ssvp_scan_sums_u64(void *sums, int64_t m, uint64_t carry_in, void *total)
{
	k_scan_sums<uint64_t><<<1, BLOCK, 0, nullptr>>>((uint64_t *)sums, m, carry_in, (uint64_t *)total);
	return (int)finish();
}

// `lists` lists of m sums, `stride` elements apart (lists >= 1)
int ssvp_scan_sums_lists_u64(void *sums, int lists, int64_t m, int64_t stride)
{
	if (lists < 1) return (int)hipErrorInvalidValue;
	k_scan_sums_lists<uint64_t><<<(unsigned)lists, BLOCK, 0, nullptr>>>((uint64_t *)sums, m, stride);
	return (int)finish();
}

// -> the index (0 / 1) of the buffers that hold the result, or -(HIP error code)
int ssvp_radix_sort_pairs(void *keys0, void *keys1, void *vals0, void *vals1, int64_t n, int key_bits, void *ghist, void *scan_scratch)
{
	uint64_t *keys[2] = {(uint64_t *)keys0, (uint64_t *)keys1};
	uint32_t *vals[2] = {(uint32_t *)vals0, (uint32_t *)vals1};
	const int r = radix_sort_pairs(nullptr, keys, vals, n, key_bits, (uint32_t *)ghist, (uint32_t *)scan_scratch);
	const hipError_t e = finish();
	return e != hipSuccess ? -(int)e : r;
}

// n >= 1 (a grid of 0 workgroups is not a launch; the clip pass calls it with events only); *flag is raised, never cleared
int ssvp_sort_nearly_sorted(const void *key_in, const void *val_in, void *key_out, void *val_out, int64_t n, void *flag)
{
	if (n < 1) return (int)hipErrorInvalidValue;
	const hipError_t e = sort_nearly_sorted(nullptr, (const uint64_t *)key_in, (const uint32_t *)val_in, (uint64_t *)key_out, (uint32_t *)val_out, n, (int *)flag);
	const hipError_t s = finish();
	return (int)(e != hipSuccess ? e : s);
}

} // extern "C"
