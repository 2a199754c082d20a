// batch_columns.h - the array members of ssv_batch_t (include/seeksv_hip.h), stated once.  Derived from this table: the staging of host batches
// (upload_host_batch, staged_view), check_batch, k_build_rec's source (SoaCols, soa_cols), ssv_batch_to_host, and the columns the two device decoders
// write, reserve and hand out (DecodedCols here, DecodedColumns in seeksv_hip.hip).
#pragma once

#include <stddef.h>
#include <string.h>
#include <type_traits>

#include "seeksv_hip.h"

namespace ssv {

enum ColLen { LEN_N, LEN_CIGAR, LEN_SEQQUAL }; // what counts a column's elements: n, n_cigar_total, seqqual_bytes

// X(member, length, in_rec, nullable, never_empty), in the order a batch's copies are issued
//   in_rec       `rec` stands in for the column: a batch with record lines need not have it, and it is not staged
//   nullable     may be NULL whatever else the batch has
//   never_empty  its staging buffer is there (16 bytes at least) even for a batch without such bytes
#define SSV_BATCH_COLUMNS(X)                  \
	X(tid, LEN_N, false, false, false)          \
	X(pos, LEN_N, false, false, false)          \
	X(flag, LEN_N, true, false, false)          \
	X(mapq, LEN_N, true, false, false)          \
	X(n_cigar, LEN_N, false, false, false)      \
	X(l_qseq, LEN_N, true, false, false)        \
	X(mtid, LEN_N, true, false, false)          \
	X(mpos, LEN_N, true, false, false)          \
	X(isize, LEN_N, true, false, false)         \
	X(cigar_off, LEN_N, true, false, false)     \
	X(cigar, LEN_CIGAR, false, false, true)     \
	X(xc, LEN_N, true, true, false)             \
	X(seq_off, LEN_N, true, false, false)       \
	X(seqqual, LEN_SEQQUAL, false, false, true) \
	X(cigar_ends, LEN_N, false, true, false)

#define X(member, ...) COL_##member,
enum BatchCol { SSV_BATCH_COLUMNS(X) COL_COUNT };
#undef X

struct BatchColDesc { size_t at, elem; ColLen len; bool in_rec, nullable, never_empty; }; // at: offsetof(ssv_batch_t, member); elem: bytes per element
#define X(member, ...) {offsetof(ssv_batch_t, member), sizeof(*ssv_batch_t::member), __VA_ARGS__},
constexpr BatchColDesc kBatchCols[COL_COUNT] = {SSV_BATCH_COLUMNS(X)};
#undef X

inline const void *col_get(const ssv_batch_t &b, int k) { const void *p; memcpy(&p, reinterpret_cast<const char *>(&b) + kBatchCols[k].at, sizeof(p)); return p; }
inline void col_set(ssv_batch_t &b, int k, const void *p) { memcpy(reinterpret_cast<char *>(&b) + kBatchCols[k].at, &p, sizeof(p)); }
inline size_t col_bytes(const ssv_batch_t &b, int k)
{
	const ColLen len = kBatchCols[k].len;
	return (size_t)(len == LEN_N ? b.n : len == LEN_CIGAR ? b.n_cigar_total : b.seqqual_bytes) * kBatchCols[k].elem;
}

// structure-of-arrays source of k_build_rec (batches that come without `rec`): every column, read-only
struct SoaCols {
#define X(member, ...) decltype(ssv_batch_t::member) member;
	SSV_BATCH_COLUMNS(X)
#undef X
};

// the columns as a device decoder writes them (ssv_bamdec_decode, ssv_samdec_decode); what only one of the two writes is a struct beside this one
struct DecodedCols {
#define X(member, ...) std::remove_const_t<std::remove_pointer_t<decltype(ssv_batch_t::member)>> *member;
	SSV_BATCH_COLUMNS(X)
#undef X
	uint32_t *seq_bytes; // bytes of packed bases + qualities the record ships (0 when not shipped): scanned into seq_off
};

} // namespace ssv
