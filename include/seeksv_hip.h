/*
 * seeksv_hip.h - C ABI of libseeksv_hip.so: the MI355X (gfx950) implementation of seeksv's
 * per-BAM-record hot path (getclip -> cluster -> getsv BAM passes).
 *
 * The reference (qiukunlong/seeksv v1.2.3) has no FFI/plugin API: the path sits behind four C++
 * call sites.  Each entry point below names the reference interface it replaces.
 * Conventions: plain C structs of pointers + counts over CALLER-OWNED buffers (structure of
 * arrays); every call returns int (0 = ok, <0 = ssv_status); nothing throws, nothing exits;
 * work is queued on the context's HIP stream and calls that return results synchronise that
 * stream before returning.  One context per GPU, not shared between threads.
 *
 * There is NO CPU fallback in this library: without a usable HIP device ssv_ctx_create fails
 * with SSV_E_NODEVICE and nothing else can be called.
 */
#ifndef SEEKSV_HIP_H_
#define SEEKSV_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSV_ABI_VERSION 9 /* v9 (additive, same version): ssv_rt_begin_original / ssv_rt_original_stats, ssv_rt_original_counts (`seeksv run -A`: junctions from the input's own supplementary alignments).
                             v9 (additive, same version): ssv_regions_set / ssv_regions_clear / ssv_region_retain / ssv_batch_select / ssv_region_lds_capacity, ssv_region, ssv_region_info (`seeksv run -L`, `-X`: the retained records restricted to BED regions).
                             v9 (additive, same version): ssv_pairdup_retain / ssv_pairdup_rows / ssv_pairdup_mark, ssv_pairdup_stats (`seeksv run -D`: duplicate pairs by unclipped 5' ends, any record order).
                             v9 (additive, same version): ssv_batch_sort, ssv_sorted, ssv_samdec_any_order (`seeksv run -u`: an original in any order, coordinate sorted while it is retained).
                             v9 (additive, same version): ssv_dup_begin / ssv_dup_retain / ssv_dup_finish, ssv_dup_stats (`seeksv run -M`: duplicate read pairs marked while the sample is retained).
                             v9 (additive, same version): ssv_samdec_sorted / ssv_samdec_lists (getclip, run: the original alignments as SAM text).
                             v9 (additive, same version): ssv_realign_split_batch (`seeksv run -P`: the split alignments as a device batch for ssv_rt_scan).
                             v9 (additive, same version): ssv_clip_table_wire_bytes, ssv_table_wire (what a cluster table's copy really moved).
                             v9 (additive, same version): ssv_realign_query_alts, SSV_RA_F_ALT_CUT (`seeksv realign -S`).
                             v9 (additive, same version): ssv_realign_query_gapped, ssv_realign_gap (`seeksv realign -g`).
                             v9 (additive, same version): ssv_aln_pack, ssv_aln_cols (getsv: the clipped-sequence re-alignments as SAM text).
                             v9 (additive, same version): ssv_samdec_begin / ssv_samdec_decode / ssv_samdec_names / ssv_samdec_last / ssv_samdec_prefetch (getsv -F on SAM text).
                             v9 (additive, same version): ssv_rt_begin / ssv_rt_scan / ssv_rt_finish (getsv -F), ssv_names_t, ssv_bamdec_names.
                             v9: ssv_table_block_bytes(left_len, right_len) lost the parameters of the removed formats; ssv_bamdec_info.unmapped_raw stays valid for one more decode.
                             v8: table formats 1 and 2 (four-piece blocks with 4-bit bases) removed - 0 ASCII or 3 compact; ssv_group with SSV_GROUP_RCCL_ONE */

typedef enum {
	SSV_OK = 0,
	SSV_E_NODEVICE = -1, /* no HIP device / HIP runtime error at init */
	SSV_E_HIP = -2,      /* a HIP call failed; text in ssv_last_error() */
	SSV_E_ARG = -3,      /* bad argument */
	SSV_E_STATE = -4,    /* call out of sequence (e.g. finish before begin) */
	SSV_E_NOMEM = -5,    /* device allocation failed */
	SSV_E_RANGE = -6     /* an output buffer supplied by the caller is too small */
} ssv_status;

/* Where the arrays of a batch live. */
typedef enum {
	SSV_MEM_HOST = 0,   /* host memory (pinned preferred); the library stages it to the GPU */
	SSV_MEM_DEVICE = 1, /* already resident in this GPU's HBM; used in place, zero copies */
	/* SSV_MEM_DEVICE | SSV_MEM_PERSISTENT: a device batch whose `cigar` and `seqqual` arrays stay valid and unchanged until the
	 * getclip pass that scanned it has delivered its table (ssv_clip_cluster[_async] has returned): clip events then keep
	 * pointing at the batch's own bytes and the cluster table is cut straight out of them - nothing is copied in between.
	 * Without the flag ssv_clip_scan copies the bytes of the batch's clip events into context memory before it returns. */
	SSV_MEM_PERSISTENT = 2
} ssv_mem;

/*
 * The "cold" fields of one record as ONE 64-byte line: everything of BAM's fixed 32-byte record core (sam/bam.h:169-178)
 * plus the first five CIGAR operations and the offsets of the variable parts.  The streaming kernels never touch it (they read the
 * hot columns tid / pos / n_cigar below, 2-8 bytes per record); the per-candidate kernels (1-3 % of the records) fetch exactly this
 * one line instead of one 64-byte sector per structure-of-arrays column.  Arrays of ssv_record must be 64-byte aligned.
 */
typedef struct {
	int32_t tid, pos;         /* as in the hot columns */
	uint16_t flag;
	uint8_t mapq;
	uint8_t xc;               /* 1 if the XC:i aux value != 0 (clip_reads.cpp:126-129) */
	uint16_t n_cigar;
	uint16_t pad;
	int32_t l_qseq, mtid, mpos, isize;
	uint32_t cigar_off;       /* index of the record's first operation in cigar[] (all operations are there too) */
	uint32_t cigar_head[5];   /* operations 0..4 (0 beyond n_cigar): 99.9 % of short-read records need nothing else */
	uint64_t seq_off;         /* as seq_off[] below */
} ssv_record;

/*
 * One batch of decoded BAM records in file order.  Field meaning follows samtools' bam1_core_t (reference: sam/bam.h:169-178) -
 * the reference's samread() loop bodies (clip_reads.h:410, cluster.cpp:48, getsv.cpp:1067, bam2depth.h:29) consume exactly these.
 * Layout: the hot columns tid, pos, n_cigar (structure of arrays: what the streaming passes read) are always required; the other
 * fixed fields come either as the classic structure-of-arrays columns (flag ... seq_off) or as `rec`, one 64-byte line per record
 * (the device decoder and the GPU generator write it natively).  A batch without `rec` is transposed into one on the device first.
 *   seq_off[i] = byte offset into seqqual of record i's ceil(l_qseq/2) packed 4-bit bases followed
 *   by l_qseq quality bytes, or SSV_NO_SEQ when the batcher did not ship them.  The batcher must
 *   ship them for every record whose first or last CIGAR operation is 'S' (only those can become
 *   clip events, clip_reads.cpp:124,150); it may omit all others.
 *   A SSV_MEM_DEVICE batch must leave at least 8 readable bytes after seqqual[seqqual_bytes - 1] (whole aligned dwords are read).
 */
#define SSV_NO_SEQ UINT64_MAX
typedef struct {
	int64_t n;                 /* records in the batch (< 2^31) */
	int32_t mem;               /* ssv_mem */
	int32_t max_ref_span;      /* >= the longest reference span (sum of M,D,N,=,X lengths) of any record in the batch;
	                              0 = unknown (the library then measures it with an extra pass over the CIGARs) */
	const int32_t *tid;        /* [n] reference id, -1 = unplaced */
	const int32_t *pos;        /* [n] 0-based leftmost coordinate */
	const uint16_t *flag;      /* [n] */
	const uint8_t *mapq;       /* [n] */
	const uint16_t *n_cigar;   /* [n] */
	const int32_t *l_qseq;     /* [n] */
	const int32_t *mtid;       /* [n] */
	const int32_t *mpos;       /* [n] */
	const int32_t *isize;      /* [n] */
	const uint32_t *cigar_off; /* [n] index of the record's first op in cigar[] */
	const uint32_t *cigar;     /* [n_cigar_total] BAM encoding: len<<4 | op */
	const uint8_t *xc;         /* [n] 1 if the XC:i aux value != 0 (clip_reads.cpp:126-129); NULL = all 0 */
	const uint64_t *seq_off;   /* [n] see above */
	const uint8_t *seqqual;    /* [seqqual_bytes] */
	int64_t n_cigar_total;
	int64_t seqqual_bytes;
	const ssv_record *rec;     /* [n] or NULL; when given, flag / mapq / l_qseq / mtid / mpos / isize / cigar_off / xc / seq_off may be NULL */
	const uint8_t *cigar_ends; /* [n] or NULL: a hot copy of the two CIGAR operations the getclip pass looks at first - (code of the first
	                              operation) | (code of the last operation) << 4, BAM's operation codes; 0xff for a record without CIGAR.
	                              The streaming pass of getclip reads this byte per record and passes on the records with an `S` at either
	                              end (1 % of a WGS sample).  NULL: the library builds the column from the record lines first (64 B/record
	                              instead of 1: fill it where the records are parsed anyway). */
	const struct ssv_tid_run *tid_runs; /* [n_tid_runs] or NULL, HOST memory whatever `mem` says (it is a handful of entries): the tid column as runs -
	                              run k covers the records [tid_runs[k].first, tid_runs[k + 1].first) (the last one up to n), all on contig
	                              tid_runs[k].tid; tid_runs[0].first == 0, firsts strictly increasing.  A coordinate-sorted BAM has one run per
	                              contig, and the batcher sees the changes while it parses the records anyway.  With it (up to 48 runs) the
	                              streaming pass of getsv does not read the tid column at all - 4 of its 8 bytes per record - except in the
	                              few tiles a run boundary falls into; the column must still be there (other passes read single entries).
	                              The list's shape is always checked (SSV_E_ARG); with SSV_VERIFY_RUNS=1 in the environment ssv_getsv_scan also
	                              holds it against the tid column (one extra streaming pass) and refuses a list that disagrees. */
	int64_t n_tid_runs;
} ssv_batch_t;

typedef struct ssv_tid_run { int64_t first; int32_t tid; int32_t pad; } ssv_tid_run;

typedef struct ssv_ctx ssv_ctx; /* opaque */

/* ---- context ------------------------------------------------------------------------------- */

/* device = HIP device ordinal.  Fails (SSV_E_NODEVICE) when there is no GPU: no CPU path exists. */
int ssv_ctx_create(int device, ssv_ctx **out);
void ssv_ctx_destroy(ssv_ctx *ctx);
/* Block until everything queued on the context's stream has finished. */
int ssv_sync(ssv_ctx *ctx);
/* Text of the last error on this context (or of the last failed ssv_ctx_create when ctx == NULL). */
const char *ssv_last_error(const ssv_ctx *ctx);
int ssv_abi_version(void);
/* GPUs this process can see (0 when there is none or the HIP runtime is not usable). */
int ssv_device_count(void);
/* The hipStream_t the context launches on (for callers that time with HIP events). */
void *ssv_stream(ssv_ctx *ctx);

/* ---- host batches: pinned memory and the copy that runs ahead -------------------------------- */
/*
 * The reference's record loops read one bam1_t at a time through samread() (clip_reads.h:410, cluster.cpp:48, getsv.cpp:1067,
 * bam2depth.h:29); here the batcher decodes whole batches into two alternating sets of arrays and the library copies batch k+1 to HBM
 * while the kernels of batch k run:
 *     ssv_batch_prefetch(ctx, &b[1]);  ssv_clip_scan(ctx, &b[0]);  ssv_batch_prefetch(ctx, &b[2]);  ssv_clip_scan(ctx, &b[1]); ...
 * ssv_host_alloc hands out page-locked host memory (usable from every GPU); only copies out of such memory run asynchronously.
 * ssv_batch_prefetch starts copying a SSV_MEM_HOST batch on the context's upload stream into one of two staging sets and returns at once;
 * at most two batches may be announced and not yet scanned.  The scan calls (ssv_clip_scan, ssv_isize_scan, ssv_getsv_scan,
 * ssv_getsv_prime) must then be given exactly the announced batches, in that order (SSV_E_STATE otherwise).  With or without prefetch:
 * when a scan call returns, the batch's host arrays have been read and may be reused.
 * Announcements belong to the stream of batches, not to a pass: ssv_clip_begin leaves them alone (a driver ends a getclip pass and begins the
 * next in the middle of a stream - and of a batch, ssv_clip_scan_range - while batch k+1 is on its way already).  ssv_isize_begin and
 * ssv_getsv_begin start a new reading of the file and drop what is still announced; ssv_batch_prefetch_drop does so on request (a caller that
 * gives up a stream early) and returns once the copies in flight have read their host arrays.
 */
int ssv_host_alloc(size_t bytes, void **p);
int ssv_host_free(void *p);
/* Page-lock memory the caller already has - e.g. a range of a read-only file mapping (ssvh_bam_map_blocks, seeksv_host.h): the chunks of a BAM then
 * go from the page cache to the GPU by DMA, no staging copy (measured on the round-4 box: locking 0.03 s/GB on one thread, copies out of the locked
 * mapping at PCIe rate, 57 GB/s; allocating page-locked staging memory costs 0.25 s/GB before a byte is read).  p and bytes are rounded outwards to
 * whole pages by the caller.  SSV_E_HIP when the runtime refuses the range (callers fall back to staging buffers). */
int ssv_host_register(void *p, size_t bytes);
int ssv_host_unregister(void *p);
/* Ask for the pages of [p, p + bytes) - anonymous memory that has not been touched yet - on the NUMA node GPU `device` hangs on (mbind, MPOL_PREFERRED): a copy between the GPU
 * and host memory on the OTHER socket of a two-socket box crosses the sockets' link and runs at 60-70 % of the PCIe rate (round 6: the same 0.55 GB table took 9.7 or 13.8 ms
 * depending on where its pages had landed).  ssv_host_alloc does this for what it hands out (the device current at the call).  Best effort: SSV_OK whatever the kernel says. */
int ssv_host_bind_near(void *p, size_t bytes, int device);
int ssv_batch_prefetch(ssv_ctx *ctx, const ssv_batch_t *b);
int ssv_batch_prefetch_drop(ssv_ctx *ctx);

/* ---- batches that stay: one decode of the file for every pass ---------------------------------- */
/*
 * The reference reads the BAM once per command (getclip: clip_reads.h:410; getsv: cluster.cpp:48 for the insert sizes, getsv.cpp:1067 and
 * bam2depth.h:29 through the index) because each command is a process of its own.  What the passes look at is 80 bytes a record - the
 * hot columns, one 64-byte line, the CIGARs, the bases of the soft-clipped reads - so a 30x genome (617 M records) stays resident in 50 GB
 * of HBM: ssv_batch_retain copies a device batch (the decoder's, valid only until the next decode) into device memory of its own -
 * SSV_MEM_DEVICE | SSV_MEM_PERSISTENT, record lines built once - and every later pass scans it in place: the file is inflated once.
 * ssv_batch_release lets go of it: the memory is the context's again and the next ssv_batch_retain takes it from there (kept until the
 * context goes or any of its allocations runs out of device memory - a fresh allocation of GBs behind the release of tens of GB waits
 * for the driver to clear them, up to 1.7 s measured).  (`seeksv run` and bench.py's file leg work this way.)
 */
int ssv_batch_retain(ssv_ctx *ctx, const ssv_batch_t *device_batch, ssv_batch_t *out);
int ssv_batch_release(ssv_ctx *ctx, ssv_batch_t *retained);

/* ---- getclip: replaces InputBamOutputReads<>'s record loop (clip_reads.h:363, 410-446) ------ */

typedef struct {
	double match_rate;      /* -t, default 0.9  (seeksv.cpp:15,131) */
	int32_t min_mapq;       /* -q, default 1    (seeksv.cpp:130) */
	int32_t save_low_quality; /* -s             (seeksv.cpp:141) */
	/* Range-partitioned runs (one GPU per reference interval).  A rank scans its interval plus a halo of
	 * records that start before it, and keeps only the clip events whose breakpoint (tid, 1-based pos) lies in
	 * [own_lo, own_hi): every (contig, side, position) bin then lives on exactly one rank with its reads in BAM order.
	 * initial_last_tid = tid of the last mapped-pair record before the first scanned record (0 at the start of the
	 * file, clip_reads.h:407).  All zero = whole file on one GPU. */
	int32_t use_ownership;
	int32_t initial_last_tid;
	int32_t own_lo_tid, own_lo_pos;
	int32_t own_hi_tid, own_hi_pos;
} ssv_clip_params;

/* Start a getclip pass.  last_tid state starts at initial_last_tid (0 like the reference's, clip_reads.h:407). */
int ssv_clip_begin(ssv_ctx *ctx, const ssv_clip_params *p);
/*
 * Scan one batch (GetSClipReads, clip_reads.cpp:112-192, incl. the contig-switch rule of
 * clip_reads.h:423-438): appends the batch's clip events - key, slice lengths, CIGAR, where the read's packed bases and
 * qualities lie - to context-owned HBM.  A host batch's arrays may be reused when the call returns, a device batch's after ssv_sync(), except
 * the `cigar` and `seqqual` arrays of a SSV_MEM_PERSISTENT batch (see ssv_mem).
 */
int ssv_clip_scan(ssv_ctx *ctx, const ssv_batch_t *b);
/*
 * The same for the records [rec_begin, rec_end) of the batch only.  For input whose contigs come back (an unsorted BAM): the reference
 * flushes and clears its maps at EVERY change of contig among the mapped-pair records (clip_reads.h:423-438), so the reads of two
 * visits of one contig never share a cluster.  A pass of this library bins by (contig, side, position); a driver therefore ends the
 * pass (ssv_clip_cluster) in front of the first record of a visit whose contig is not greater than every contig of the pass so far
 * and starts the next one there (initial_last_tid = the contig before): scan [0, i) - cluster - begin - scan [i, n).  Records before
 * rec_begin still count as "the record before" of the contig-switch rule.  A batch announced with ssv_batch_prefetch stays announced
 * until a call with rec_end == n has consumed it.
 */
int ssv_clip_scan_range(ssv_ctx *ctx, const ssv_batch_t *b, int64_t rec_begin, int64_t rec_end);
/* Events collected so far (synchronises). */
int ssv_clip_event_count(ssv_ctx *ctx, int64_t *n_events);

/*
 * Cluster table = what the two multimaps hold when the reference flushes them
 * (InsertSeq/ChangeSeqAndQual, clip_reads.cpp:57-108,260-283), in the reference's emit order
 * (per contig: all '5' rows by position, then all '3' rows; ties in creation order,
 * clip_reads.h:432-433).  All pointers are HOST buffers owned by the context, valid until the
 * next ssv_clip_begin / ssv_ctx_destroy.
 */
typedef struct {
	int32_t tid;
	uint8_t side;              /* '5' or '3' */
	uint8_t pad[3];
	int64_t first;             /* index of the run's first cluster */
} ssv_table_run;

typedef struct {
	int64_t n_clusters;
	int64_t n_events;
	const int32_t *tid;        /* [n_clusters] */
	const int32_t *pos;        /* [n_clusters] 1-based breakpoint coordinate */
	const uint8_t *side;       /* [n_clusters] '5' or '3' */
	const int32_t *support;    /* [n_clusters] support_read_no */
	const int32_t *left_len;   /* [n_clusters] |seq_left|  */
	const int32_t *right_len;  /* [n_clusters] |seq_right| */
	const uint8_t *qual_missing; /* [n_clusters] 1: reference prints "*" for both qualities */
	const uint64_t *str_off;   /* [n_clusters] offset into str of: seq_left, qual_left, seq_right, qual_right; every block starts
	                              4-byte aligned and is zero padded to a multiple of 4 bytes */
	const uint8_t *str;        /* ASCII, not NUL terminated */
	const uint64_t *cigar_off; /* [n_clusters] offset into cigar */
	const int32_t *n_cigar;    /* [n_clusters] ops of the record whose CIGAR the cluster carries */
	const uint32_t *cigar;     /* BAM-encoded ops INCLUDING S/H (GenerateCigar drops those when printing) */
	int32_t seq_packed;        /* 0: the layout above (format 0).  1: format 3, below. */
	int32_t qual_bits;         /* 8: qualities are characters (phred + 33), one byte each; format 3: bits per quality (or per group of qualities) in the
	                              quality stream, below.  Lossless: base qualities are most of the table's bytes and come from a handful of values
	                              on current sequencers. */
	uint8_t qual_alphabet[64]; /* index -> quality character (v8: 64 places; the entries in use are non-zero and increasing) */
	/* ---- format 3, the compact table: what the host can rebuild does not cross PCIe ----
	 * (The arrays below are what a caller reads.  pos, c_len, c_support, c_ncig and c_cigar cross in a narrower form of the library's own, ~7 instead of
	 * ~17 bytes a cluster, and stand rebuilt at these widths when ssv_clip_table_wait returns: ssv_clip_table_wire_bytes.)
	 * Handed out by ssv_clip_table_wait: pos, c_cigar (cigar too when cigar_bytes is 4), str and the fields below; tid, side, support, left_len, right_len, qual_missing,
	 * n_cigar, str_off and cigar_off are NULL until ssv_clip_table_expand() has rebuilt them on the host.
	 *   c_len      [n_clusters][2] left_len, right_len, len_bytes (2 or 4) wide each
	 *   c_support  [n_clusters] support_bytes (2 or 4) wide;  c_ncig [n_clusters] ncig_bytes (1 or 2) wide;  c_flags bit 0 = qual_missing
	 *   runs       the table is a sequence of (contig, side) runs; run r covers clusters [runs[r].first, runs[r + 1].first)
	 *   a cluster's string block = [base stream | quality stream], each zero padded to whole 32-bit words; blocks follow each other in
	 *   cluster order (str_off = running sum of ssv_table_block_bytes3), CIGARs likewise (cigar_off = running sum of n_cigar):
	 *     base stream     the n = left_len + right_len bases of seq_left then seq_right, base_bits each, base i at stream bits
	 *                     [i * base_bits, +base_bits) (bit b of a stream = bit b % 8 of byte b / 8).  base_bits 2: index into "ACGT", and
	 *                     every base that is something else is listed in base_exc (the stream holds 0 there); base_bits 4 (only when
	 *                     that list would be too long): index into "=ACMGRSVTWYHKDBN"
	 *     quality stream  the n qualities the same way at qual_bits each (8: characters), all zero when qual_missing.  qual_group k > 1 (v7; alphabets
	 *                     whose size R is far from a power of two - five values: k = 3, qual_bits = 7; nine to eleven: k = 2, qual_bits = 7; v8: 17 to 45 values - a
	 *                     HiSeq-style 40-value alphabet -: k = 2, qual_bits = 11, i.e. 5.5 bits a quality instead of 8): the stream is
	 *                     ceil(n / k) groups of qual_bits bits, group g at stream bits [g * qual_bits, +qual_bits), holding qualities
	 *                     g k .. g k + k - 1 as the number i_0 + R i_1 + R^2 i_2 (i_j = index into qual_alphabet; places behind the stream's end: 0),
	 *                     R = the number of qual_alphabet entries in use (they are characters, so non-zero)
	 *   base_exc   sorted; cluster << 28 | base index << 4 | index into "=ACMGRSVTWYHKDBN" */
	int32_t format;            /* the ssv_clip_table_format the table was built with */
	int32_t base_bits;
	int32_t len_bytes, support_bytes, ncig_bytes;
	int32_t qual_group;        /* format 3: qualities per group of qual_bits bits (1: every quality its own field) */
	const void *c_len;
	const void *c_support;
	const void *c_ncig;
	const uint8_t *c_flags;
	const ssv_table_run *runs;
	int64_t n_runs;
	const uint64_t *base_exc;
	int64_t n_base_exc;
	uint64_t str_bytes;        /* bytes of str / operations of cigar (all formats) */
	uint64_t cigar_ops;
	int64_t support_sum;       /* format 3, after ssv_clip_table_expand: sum of the support column (= n_events: every clip event is in one cluster) */
	const void *c_cigar;       /* format 3 (v7): the CIGAR operations, cigar_bytes wide each - 2: length << 4 | code in 16 bits (every
	                              length of the table is below 4096; `cigar` is NULL then: read (const uint16_t *)c_cigar + cigar_off[k]); 4: = cigar */
	int32_t cigar_bytes, pad4;
} ssv_cluster_table;

/* Table format of the following ssv_clip_cluster[_async] calls: 0 ASCII (default), 3 the compact table (see ssv_cluster_table: ~100
 * instead of ~330 bytes per 150-base cluster; the table is the path's output and PCIe bounds the step).  (1 and 2, the four-piece blocks
 * with 4-bit bases of ABI versions below 8, are gone: SSV_E_ARG.) */
int ssv_clip_table_format(ssv_ctx *ctx, int format);
/* Format 3: rebuild the columns that did not cross PCIe (contig and side from the runs, the widened support / lengths / flags, string
 * and CIGAR offsets as running sums) into context-owned host memory, on n_threads host threads (0: as many as the machine has), and
 * set the pointers in *t.  Valid as long as the table. */
int ssv_clip_table_expand(ssv_ctx *ctx, ssv_cluster_table *t, int32_t n_threads);
/* What really crossed PCIe for a table handed out by ssv_clip_table_wait[_prev], in bytes per piece (v9, additive).  The widths in ssv_cluster_table
 * describe the arrays that are handed out; a format-3 table's small columns cross narrower than that (below) and are rebuilt on a host thread of
 * the context while the strings are still crossing.
 *   narrow 1: per cluster one row of 6 bytes - pos as a u16 step from the cluster before (0xffff: pos stands in a list of (cluster, pos) escapes: a run's
 *             first cluster, the first cluster of every 256 sorted slots, steps of 65535 and more), left_len, right_len, support as a byte each, n_cigar
 *             with a 2-bit CIGAR kind (1: exactly left_len M right_len S; 2: exactly left_len S right_len M; 0: the operations cross in the CIGAR stream);
 *          0: the columns as they are handed out (a length of 256 or more, a support of 255 or more, a CIGAR of 64 operations or more;
 *             SSV_TABLE_WIRE=wide, SSV_TABLE_WIDE_COLUMNS, SSV_PACK_COLS=split; format 0)
 *   flags (one byte a cluster), runs, base exceptions and the strings cross as they are handed out. */
typedef struct {
	int32_t narrow, pad;
	uint64_t total;            /* the sum of the pieces below */
	uint64_t rows, flags, cigar, runs, base_exc, pos_esc, str;
} ssv_table_wire;
int ssv_clip_table_wire_bytes(ssv_ctx *ctx, const ssv_cluster_table *t, ssv_table_wire *out);
/* Bytes of one cluster's string block in format 3 (n_bases = left_len + right_len). */
uint64_t ssv_table_block_bytes3(int64_t n_bases, int32_t base_bits, int32_t qual_bits);
/* The same for a table whose qualities go in groups (ssv_cluster_table.qual_group; 1 = the function above). */
uint64_t ssv_table_block_bytes3g(int64_t n_bases, int32_t base_bits, int32_t qual_bits, int32_t qual_group);
/* Bytes of one cluster's string block in format 0: seq_left, qual_left, seq_right, qual_right as characters, padded to a multiple of 4 (v9: two parameters). */
uint64_t ssv_table_block_bytes(int32_t left_len, int32_t right_len);

/* Sort events into (contig, side, position) bins and run the greedy consensus clustering. */
int ssv_clip_cluster(ssv_ctx *ctx, ssv_cluster_table *out);
/*
 * The same in two halves: ssv_clip_cluster_async returns as soon as the clustering kernels are done and the copy of the table
 * to host memory has been queued on a second stream (n_clusters / n_events are known then); ssv_clip_table_wait blocks until
 * that copy has landed and hands the table out.  Two tables are kept, so the caller may start the next getclip pass (or the
 * getsv passes) while the previous table is still crossing PCIe: a table stays valid until the second-next
 * ssv_clip_cluster[_async] call.
 */
int ssv_clip_cluster_async(ssv_ctx *ctx, int64_t *n_clusters, int64_t *n_events);
int ssv_clip_table_wait(ssv_ctx *ctx, ssv_cluster_table *out);
/* The table of the call before the most recent ssv_clip_cluster[_async] (pipelined drivers: cluster k+1, then collect table k). */
int ssv_clip_table_wait_prev(ssv_ctx *ctx, ssv_cluster_table *out);

/* ---- somatic: the tumor rows' look-ups among the normal's clusters, on the table where it lies (v9, additive; `seeksv somatic -K`) ----
 * What ReadTumorFileAndOutputSomaticInfo (somatic.cpp:58-427) asks of the normal sample's clusters is two look-ups per row; a look-up is a probe.  A cluster is
 * (tid, pos, side, seq_left, seq_right, support); its clipped side is seq_left for side '5' and seq_right for side '3'.  A probe sees the clusters of its own
 * tid and side whose clipped side has at least min_clipped_len characters (unsigned compare, somatic.h:54), in the table's order (by position, ties in creation
 * order), and the FIRST that matches gives the hit:
 *   begin(x, y): n = min(|x|, |y|), m = the i < n with x[i] == y[i]; true iff n > 0 and (double)m / n >= match_rate.  end(x, y): the same from the last characters.
 *   mode 0 (exact):    candidates with pos == lo; match iff begin(b, seq_right) && end(a, seq_left)
 *   mode 1 / 2 (anchored): candidates with lo <= pos <= hi; (s1, s2, s3, s4) = (seq_left, seq_right, a, b) in mode 1, (a, b, seq_left, seq_right) in mode 2;
 *                      no match if |s2| < 10; h = the FIRST occurrence of s2[0..10) in s4 (none: no match; a later one is never tried);
 *                      match iff end(s1, s3 + s4[0..h)) && begin(s2, s4[h..))          (Compare, clip_reads.cpp:333-370)
 * Over passes (a BAM is several; a contig may come back in a later one) the order is that of the reference's multimap over the whole file: smaller position
 * first, equal positions in pass order - a later pass's match replaces the stored hit only when its pos is strictly smaller (an exact probe: only when there is none). */
typedef struct {
	int32_t tid;            /* contig id in the scanned batches' header; < 0: not in the header, the probe finds nothing */
	int32_t lo, hi;         /* 1-based breakpoint positions, inclusive; an exact probe has lo == hi; lo may be <= 0 */
	uint8_t side;           /* '3' or '5' */
	uint8_t mode;           /* 0 exact, 1 anchored (cluster first), 2 anchored (probe first) */
	uint8_t pad[2];
	uint32_t a_off, a_len, b_off, b_len;   /* the probe's two strings, in `text` */
} ssv_clip_probe;
typedef struct { int32_t support, pos, pass, pad; int64_t cluster; } ssv_clip_probe_hit;   /* support 0: no cluster matched; pass: 0-based count of clustered passes since the set; cluster: index in that pass's table */

/* Copies probes and text to the device and zeroes the hits.  The probes stay set across ssv_clip_begin calls until a set with n == 0, the next set or
 * ssv_ctx_destroy; while they are set, every ssv_clip_cluster[_async] runs them against that pass's table (timing group `somatic_probe`) - the table must
 * be format 0: a format-3 cluster call returns SSV_E_ARG.  NULL arguments with n > 0, a side other than '3' / '5', a mode above 2, an offset plus length
 * beyond text_bytes: SSV_E_ARG, and nothing is changed. */
int ssv_clip_probe_set(ssv_ctx *ctx, const ssv_clip_probe *probes, int64_t n, const char *text, uint64_t text_bytes,
                       double match_rate, uint32_t min_clipped_len);
/* Synchronises; the hits accumulated over all passes clustered since the set, and how many passes that was. */
int ssv_clip_probe_get(ssv_ctx *ctx, ssv_clip_probe_hit *hits /* [n] */, int64_t *passes);

/* ---- getsv pass 1: replaces CalculateInsertsizeDeviation (cluster.cpp:15-83) ---------------- */

int ssv_isize_begin(ssv_ctx *ctx, int32_t min_mapq, int64_t max_pairs);
/* *done is set to 1 once max_pairs qualifying records have been seen (the reference breaks there).  The reference compares the count
   with max_pairs for EQUALITY after every record it does not skip (cluster.cpp:68): max_pairs < 0 is no limit, and max_pairs == 0 ends the
   pass at the first such record when that one does not qualify and is no limit when it does. */
int ssv_isize_accumulate(ssv_ctx *ctx, const ssv_batch_t *b, int32_t *done);
/* Returns n_pairs==0 exactly when the reference returns 1 and leaves mean/sd untouched. */
int ssv_isize_finish(ssv_ctx *ctx, int64_t *n_pairs, int32_t *mean, int32_t *sd);

/* ---- getsv passes 2+3, fused: FindDiscordantReadPairs (getsv.cpp:990-1120) and
 *      main_depth (bam2depth.cpp:17-142) ------------------------------------------------------- */

/* One junction and its (already clamped) query window, getsv.cpp:1041-1060. */
typedef struct {
	int32_t up_tid;      /* tid of up_chr */
	int32_t down_tid;    /* tid of down_chr, -1 if absent from the header (never matches) */
	int32_t up_pos;      /* 1-based */
	int32_t down_pos;    /* 1-based */
	int32_t beg;         /* 0-based window start after clamping */
	int32_t end;         /* window end after clamping; candidates: ref_end > beg && pos < end */
	uint8_t up_strand;   /* '+' or '-' */
	uint8_t down_strand;
	uint8_t pad[2];
} ssv_junction;

/* 1-based inclusive interval on a contig. */
typedef struct {
	int32_t tid;
	int32_t beg;
	int32_t end;
} ssv_interval;

typedef struct {
	/* discordant tally (may be disabled with n_junctions = 0) */
	const ssv_junction *junctions; /* host */
	int64_t n_junctions;
	int32_t mean, sd, times;       /* from ssv_isize_finish; times = 4 (seeksv.cpp:161) */
	int32_t disc_min_mapq;         /* -q (20) */
	/* depth (may be disabled with n_windows = 0) */
	const ssv_interval *windows;   /* host; merged windows: sorted by (tid,beg), pairwise disjoint */
	int64_t n_windows;
	int32_t depth_min_mapq;        /* -q (20) */
	int32_t n_targets;             /* contigs in the BAM header */
	const int32_t *target_len;     /* host [n_targets] */
} ssv_getsv_params;

int ssv_getsv_begin(ssv_ctx *ctx, const ssv_getsv_params *p);
/* One fused pass over a batch: discordant-pair tally per junction + coverage of the windows. */
int ssv_getsv_scan(ssv_ctx *ctx, const ssv_batch_t *b);
/*
 * Range-partitioned runs (one GPU per run of records): the reference's pileup keeps at most ~8000 reads alive (bam_plp_push), a rule that
 * depends on the records BEFORE a rank's first one.  Right after ssv_getsv_begin a rank replays the last records before its range through
 * the pileup's bookkeeping only (nothing of them is counted: they belong to the rank before).  *sufficient = 0: the replayed batch itself
 * begins inside a > 8000x stack, or is shorter than 16,384 records and so too short to tell (a batch that starts at the file's first record
 * is exact whatever the answer: the caller knows that case): call ssv_getsv_begin again and replay a longer run.  At WGS depths the first 24,576 records before the range always suffice.
 */
int ssv_getsv_prime(ssv_ctx *ctx, const ssv_batch_t *b, int32_t *sufficient);
/*
 * counts[n_junctions]      = abnormal_read_pair_no per junction (getsv.cpp:1116)
 * range_sum[n_ranges]      = sum over the interval of per-column depth (bam2depth.cpp:101-122);
 *                            each range must lie inside one window
 * point_depth[n_points]    = depth at (tid, beg) (bam2depth.cpp:123-124); 0 outside every window
 * max_depth                = largest per-column depth inside the windows.  The depths follow libbam 0.1.16's pileup, which keeps at
 *                            most ~8000 reads alive: a read that is not the first at its start position is dropped when 2 + (accepted
 *                            reads of the contig ending at or after that start, a read without M/D/N operation only while it is the
 *                            first read at the current start) > 8000 (bam_plp_push); batches must arrive in file order
 */
int ssv_getsv_finish(ssv_ctx *ctx, int32_t *counts,
                     const ssv_interval *ranges, int64_t n_ranges, uint64_t *range_sum,
                     const ssv_interval *points, int64_t n_points, int32_t *point_depth,
                     int32_t *max_depth);

/* ---- range-partitioned runs: the one exchange step ------------------------------------------------------------------
 * One context per GPU, one host thread per context.  Each rank scans its own run of records (libseeksv_host's ssvh_bam_partition cuts the
 * file) for ALL junctions and windows; the per-rank result vectors - discordant counts, depth sums, point depths: KBs to a few MB - are
 * all-gathered and added up by every rank.  RCCL (ncclAllGather over xGMI, loaded on first use) when the ranks sit on different GPUs;
 * ranks that share a GPU (tests on a one-GPU box) exchange through host memory.  SSV_GROUP_RCCL_ONE=1 makes a group of ONE rank an RCCL
 * communicator as well (ncclCommInitAll over one device), so that the RCCL branch runs end to end where there is a single GPU. */
typedef struct ssv_group ssv_group;
int ssv_group_create(ssv_ctx **ctxs, int n, ssv_group **out);
void ssv_group_destroy(ssv_group *g);
int ssv_group_uses_rccl(const ssv_group *g);
/* Called by every rank from its own thread: send = this rank's `bytes` bytes (host memory), recv = n * bytes, rank order.
 * No rank is ever left waiting: the ranks agree through the host - before anything is exchanged - that all of them arrived, prepared and
 * bring vectors of one size; a rank whose ncclAllGather fails aborts the group's communicators (ncclCommAbort) so that its peers come back;
 * a rank that does not arrive within SSV_GROUP_TIMEOUT_S (default 600) breaks the group.  In every such case EVERY rank returns an error
 * (SSV_E_HIP / SSV_E_ARG for the rank at fault, SSV_E_STATE for the others) and nothing in `recv` may be used; after an abort or a timeout
 * the group only answers SSV_E_STATE.  (SSV_GROUP_FAIL=<rank>:<1|2|3> injects a failure before the exchange / in the
 * collective's call / behind an issued collective: tests.) */
int ssv_group_allgather(ssv_group *g, int rank, const void *send, size_t bytes, void *recv);

/* ---- device-side BGZF inflate + BAM record decode ---------------------------- */

/*
 * What libbam's samread() does per record on one core (sam/sam.h:73: bgzf inflate + bam_read1) for a whole chunk of the file on
 * the GPU: the caller hands over the COMPRESSED bytes of a run of whole BGZF blocks plus their table, and gets the decoded records
 * as an SSV_MEM_DEVICE batch that ssv_clip_scan / ssv_isize_accumulate / ssv_getsv_scan consume directly - the inflated bytes
 * never cross PCIe.  libseeksv_host's ssvh_bam_read_blocks produces the input.
 *   one chunk = blocks in file order; a record may straddle chunks (its head is carried over inside the context);
 *   c_off/c_len = the block's raw deflate payload inside `comp` (after the 18-byte BGZF header, without the 8-byte trailer),
 *   u_len = its ISIZE.  A chunk must inflate to < 4 GB.
 */
typedef struct {
	uint64_t c_off;
	uint32_t c_len;
	uint32_t u_len;
} ssv_bgzf_block;

typedef struct {
	int64_t n_records;           /* records of the last chunk */
	uint64_t inflated_bytes;     /* bytes the chunk inflated to */
	uint64_t tail_offset;        /* internal: where the unfinished record starts */
	uint32_t repaired_blocks;    /* blocks whose speculated first record start had to be corrected (diagnostic) */
	int32_t last_tid;            /* contig of the last record without UNMAP|MUNMAP so far */
	/* host-side lists of the last chunk (pinned memory owned by the context, valid until the next decode; unmapped_raw: until the decode AFTER
	 * the next one - two buffers in turn, so that a host thread can pair a chunk's reads up while the next chunk is decoded): */
	const uint8_t *unmapped_raw; /* the UNMAP|MUNMAP records as they lie in the BAM stream (block_size prefixed), in order: */
	uint64_t unmapped_bytes;     /*   the unmapped-pair FASTQ side channel of getclip (clip_reads.h:415-419) decodes them on the host */
	uint32_t n_tid_runs;         /* contig changes among the other records, in order (the flush sequence of clip_reads.h:423-438): */
	const uint32_t *tid_run_index; /* record index inside the batch, */
	const int32_t *tid_run_tid;    /* its contig */
} ssv_bamdec_info;

/* Start a file: n_targets of its header (plausibility of speculated record starts), and the offset of the first record inside the
 * inflated stream of the first chunk (= the length of the BAM header: magic, text, reference list). */
int ssv_bamdec_begin(ssv_ctx *ctx, int32_t n_targets, uint64_t first_record_offset);
/* Optional, after ssv_bamdec_begin: the lengths of the n_targets contigs (the BAM header's l_ref values).  Record starts inside a chunk are found by
 * speculation and then verified; with the lengths a candidate whose position lies outside its contig is dismissed at once, which spares the verifier
 * the rare block it would have to walk record by record.  Results do not depend on it. */
int ssv_bamdec_target_lens(ssv_ctx *ctx, const int32_t *lens);
/* A run of records that ends inside the next chunk (one rank's share of a file, ssvh_bam_raw_begin_range): its records end `inflated_bytes`
 * into the chunk's blocks - a record boundary; what the blocks hold behind it belongs to the next run.  Applies to the next decode call only. */
int ssv_bamdec_limit(ssv_ctx *ctx, uint64_t inflated_bytes);
/* Optional, after ssv_bamdec_begin: chunks that inflate to up to `inflated_bytes` will follow - the decoder's buffers are then sized for them by the
 * first decode, however small its chunk (a driver starts a file with a small chunk so that the GPU gets to work early; growing ~40 buffers when the
 * first full-size chunk arrives cost 0.2 s). */
int ssv_bamdec_expect(ssv_ctx *ctx, uint64_t inflated_bytes);
/* Optional, after ssv_bamdec_begin: on != 0 makes every decode check each inflated block's CRC32 against the one in the block's BGZF trailer (one
 * more pass over bytes that are in HBM anyway) and refuse the chunk on a mismatch.  Off by default, like libbam 0.1.16's reader (sam/sam.h:73), which
 * checks no CRC: a block whose deflate structure is valid but whose bytes were damaged decodes silently there - and here, without this. */
int ssv_bamdec_verify_crc(ssv_ctx *ctx, int on);
/* Optional, after ssv_bamdec_begin: on != 0 accepts a file in any record order (getsv -F reads split alignments in read order): a chunk with more than
 * 65536 contig changes among its mapped-pair records, which is otherwise refused as "not coordinate sorted", is decoded; its contig-change list is then
 * not handed out (ssv_bamdec_info.n_tid_runs = 0).  Off by default. */
int ssv_bamdec_any_order(ssv_ctx *ctx, int on);
/* ... and that starts inside the file: the contig of the last mapped-pair record before it (0 at the start of the file, clip_reads.h:407) -
 * ssv_bamdec_info's contig-change list continues from there.  After ssv_bamdec_begin, before the first decode. */
int ssv_bamdec_prev_tid(ssv_ctx *ctx, int32_t tid);
/* Pinned host buffers (three, which = 0 | 1 | 2; grow-only, owned by the context) to read the compressed bytes of a chunk into, so that a
 * reader thread can fill one while the chunk in the second is on its way to the GPU and the one in the third is being decoded; any host memory
 * works too (page-locked: ssv_host_register - e.g. the file's own pages in a mapping, no staging copy at all).  A buffer is free again when the
 * decode call that was given it returns. */
int ssv_bamdec_staging(ssv_ctx *ctx, int which, size_t bytes, void **host_ptr);
/* Optional: announce a chunk ahead.  Its compressed bytes start their way to the GPU at once, on the context's upload stream, while the chunk
 * before it is being inflated (two chunks may be announced at any time); ssv_bamdec_decode of the same (comp, comp_bytes) then finds them there instead
 * of copying.  The host buffer must stay untouched until that decode call returns; it should be page-locked (ssv_bamdec_staging, ssv_host_alloc) -
 * out of pageable memory the copy is not asynchronous.  Typical loop: prefetch(0); for k: prefetch(k+1); decode(k); ... */
int ssv_bamdec_prefetch(ssv_ctx *ctx, const void *comp, size_t comp_bytes);
/* Give up chunks that were announced and will not be decoded (a pass that stops early): returns when their copies have left the host memory. */
int ssv_bamdec_prefetch_drop(ssv_ctx *ctx);
/* Inflate + decode one chunk.  *out is an SSV_MEM_DEVICE batch owned by the context, valid until the next decode on it (stream
 * ordered: kernels already enqueued on the context's stream may still read it).  n_blocks == 0 = end of input (fails if a record
 * is unfinished).  keep_all_seq as in ssvh_bam_read_batch.  Synchronises the stream. */
int ssv_bamdec_decode(ssv_ctx *ctx, const void *comp, size_t comp_bytes, const ssv_bgzf_block *blocks, int64_t n_blocks, int keep_all_seq, ssv_batch_t *out);
int ssv_bamdec_last(ssv_ctx *ctx, ssv_bamdec_info *info);

/* The read names of a batch, beside ssv_batch_t (which has no field for them): record i's NUL-terminated name (at most 255 bytes with the NUL) starts at
 * base + off[i] + bias.  mem as in ssv_batch_t (SSV_MEM_HOST: base[bytes] and off[n] are copied to the GPU; SSV_MEM_DEVICE: used in place, bytes unused;
 * any other mem, bias < 0, or bytes < 0 with SSV_MEM_HOST: SSV_E_ARG from every call that takes one). */
typedef struct {
	int32_t mem;
	int32_t pad;
	int64_t bias;
	const char *base;
	const uint64_t *off;
	int64_t bytes;
} ssv_names_t;
/* The names of the last chunk ssv_bamdec_decode handed out, in HBM (valid as long as that batch). */
int ssv_bamdec_names(ssv_ctx *ctx, ssv_names_t *out);
/* ---- device-side SAM text decode (getsv -F: `bwa bwasw` writes SAM text; process_bwasw.cpp:12-16 opens every name without ".bam" as text) ----
 * What libbam 0.1.16's sam_read1 does per line on one core, for a whole chunk of the file on the GPU: the caller hands over the file's TEXT as it is
 * (after the header) and gets the records as an SSV_MEM_DEVICE batch, like ssv_bamdec_decode's with keep_all_seq, plus the read names.
 * Grammar: well-formed lines decode to what libbam's text reader gives; everything else is refused (SSV_E_ARG, "Parse error at line N: reason" in
 * ssv_last_error; lines are counted over the whole file, header included) - fewer than 11 fields, an empty line, an '@' line among the records, a
 * name that is empty or longer than 254 bytes, a number that is none or out of range (FLAG decimal - without a leading 0, which is octal to libbam - or 0x hex, up to 65535, POS / PNEXT 0..2^31-1 stored
 * minus 1, MAPQ 0..255, TLEN signed 32 bits with '-' as the only sign: a leading '+' is refused, though libbam's atoi takes it, CIGAR lengths below 2^28), a CIGAR with a character outside MIDNSHP=X, an operation without a length or
 * more than 65535 operations, "CIGAR and sequence length are inconsistent", "sequence and quality are inconsistent", a QUAL byte below 33, a NUL byte.
 * RNAME / RNEXT: '*' and names that are not in the header give -1, RNEXT '=' gives tid.  SEQ bytes: '=' 0, "ACMGRSVTWYHKDBN" in either case 1..15,
 * "0123" 1 2 4 8, every other byte 15; '*' gives l_qseq 0.  CIGAR '*' gives n_cigar 0 and sets flag 4, as libbam does ("mapped sequence without CIGAR").  QUAL '*' gives 0xff bytes.  A '\r' before the newline is dropped.  Optional fields are
 * ignored except XC:i: (xc = 1 when its value is not 0).  '=' and 'X' in a CIGAR are BAM's codes 7 and 8 (libbam's text reader aborts on them). */
typedef struct {
	int32_t n_targets;                 /* contigs of the header (@SQ lines, in order) */
	int32_t pad;
	const char *const *target_names;   /* [n_targets] host, NUL-terminated; read during the call */
	uint64_t first_line;               /* 1-based line number, in the file, of the first line that will be handed to ssv_samdec_decode */
} ssv_samdec_params;

typedef struct {
	int64_t n_records;       /* records of the last decode */
	uint64_t lines_consumed; /* lines decoded since ssv_samdec_begin */
	uint64_t carried_bytes;  /* bytes of the unfinished last line kept for the next decode */
	uint64_t refused_line;   /* 0, or the file line number of the first line that was refused */
	const char *refused_reason; /* NULL, or why (static text) */
} ssv_samdec_info;

int ssv_samdec_begin(ssv_ctx *ctx, const ssv_samdec_params *p);
/* Optional: announce the next chunk (host memory, best page-locked): its bytes start their way to the GPU on the upload stream at once, under the kernels of the
 * chunk before; ssv_samdec_decode of the same (text, bytes) finds them there.  The memory must stay untouched until that decode returns.  Two may be announced. */
int ssv_samdec_prefetch(ssv_ctx *ctx, const void *text, size_t bytes);
/* The next `bytes` bytes of the file, cut ANYWHERE (mem: SSV_MEM_HOST or SSV_MEM_DEVICE).  The unfinished last line is carried inside the context and moved,
 * on the device, in front of the next chunk's bytes: every line is contiguous in HBM.  last != 0: the file ends here - a final line without a newline is a
 * record (bytes == 0 with last flushes); the next call must be ssv_samdec_begin.  *out: an SSV_MEM_DEVICE batch owned by the context, valid until the next
 * decode (stream ordered): hot columns, cigar_ends, record lines (rec), all CIGAR operations, every record's packed bases and qualities; n_tid_runs = 0 (the
 * file is in read order).  carry + bytes must stay below 4 GB.  After a refused line only ssv_samdec_begin is accepted.  Synchronises the stream. */
int ssv_samdec_decode(ssv_ctx *ctx, const void *text, size_t bytes, int mem, int last, ssv_batch_t *out);
/* The read names of the last decoded batch: C strings inside the context's copy of the text (the first tab of every line is overwritten with a NUL),
 * off[i] = where line i starts.  Valid as long as that batch. */
int ssv_samdec_names(ssv_ctx *ctx, ssv_names_t *out);
int ssv_samdec_last(ssv_ctx *ctx, ssv_samdec_info *info);
/* A coordinate-sorted ORIGINAL as SAM text (what getclip and `seeksv run` read; clip_reads.h:363-384 opens every name without ".bam" as text).  Between
 * ssv_samdec_begin and the first ssv_samdec_decode, else SSV_E_ARG; without it every call behaves as described above.  With it each batch is, bit for bit, what
 * ssv_bamdec_decode(keep_all_seq) gives for the BAM of the same records:
 *   keep_all_seq == 0: a record ships ceil(l / 2) + l bytes of bases + qualities when its first or last CIGAR operation is S and nothing otherwise
 *     (seq_off = SSV_NO_SEQ), xc is set for soft-clipped records only, the record lines say the same;
 *   tid_runs / n_tid_runs of the batch are filled (up to 64 runs);
 *   more than 65536 contig changes among a chunk's mapped-pair records: SSV_E_ARG, the text is not coordinate sorted.
 * Consequence: a QUAL byte below 33 is refused only in lines whose qualities are read - lines that ship and UNMAP|MUNMAP lines (libbam refuses none).  The SEQ /
 * QUAL / CIGAR length checks hold for every line. */
int ssv_samdec_sorted(ssv_ctx *ctx, int keep_all_seq);
/* ... and the lists of the last decoded chunk, in the BAM decoder's struct: n_records, last_tid (contigs carried across chunks, 0 before the first record),
 * n_tid_runs / tid_run_index / tid_run_tid, and unmapped_raw / unmapped_bytes: every line whose flag as decoded (a '*' CIGAR sets 4) has UNMAP or MUNMAP, as
 * a BAM record in file order - block_size, the 32 core bytes (bin = 0), name and NUL, CIGAR operations, packed bases, qualities (QUAL '*': 0xff), no optional
 * fields - which ssvh_raw_record_fastq reads like the BAM decoder's.  inflated_bytes: the bytes of text the call was given; tail_offset, repaired_blocks: 0.
 * Lifetimes as for ssv_bamdec_last (unmapped_raw: two page-locked buffers in turn, valid until the decode after the next one).  SSV_E_STATE without the mode. */
int ssv_samdec_lists(ssv_ctx *ctx, ssv_bamdec_info *out);
/* Optional, after ssv_samdec_begin (v9, additive; `seeksv run -u`): text in any record order, with the meaning of ssv_bamdec_any_order.  A chunk with more than
 * 65536 contig changes among its mapped-pair records is then decoded like any other; only its contig-change list (ssv_samdec_lists: n_tid_runs = 0) is not
 * handed out.  Everything else is unchanged; off after every ssv_samdec_begin. */
int ssv_samdec_any_order(ssv_ctx *ctx, int on);

/* ---- the clipped-sequence re-alignments of `getsv` out of a decoded batch (getsv.h:437-446 opens every name without ".bam" as SAM text) ----
 * What the host join (InputSoftInfoStoreBreakpoint + GetAlignInfo, getsv.h:423-541, getsv.cpp:25-71) reads of every record of clip.bam / clip.sam: tid, pos, flag,
 * mapq, the CIGAR, the read name - which is the clipped sequence itself - and a 64-bit hash of that name, the join's first compare.  ssv_aln_pack takes a batch
 * (SSV_MEM_DEVICE: ssv_samdec_decode's or ssv_bamdec_decode's, used in place; SSV_MEM_HOST: staged like any scan call's) and its names (ssv_names_t, as ssv_rt_scan
 * takes them: device names in place, host names copied, `bias` added) and hands these columns out in page-locked HOST memory owned by the context, valid until
 * the next ssv_aln_pack on it: the names packed back to back in record order on the GPU and hashed there over their bytes without the NUL -
 *   h = 0x9E3779B97F4A7C15 ^ n;  per little-endian 8-byte word w (the tail zero padded): h = (h ^ w) * 0xFF51AFD7ED558CCD, h ^= h >> 29;  result h * 0xC4CEB9FE1A85EC53
 * (libseeksv_host's clip_text_hash).  cigar_off[i] indexes this call's cigar[], which holds the batch's n_cigar_total operations.  n == 0 is a valid call (empty
 * columns).  A name is at most 254 bytes without its NUL.  Synchronises the stream.  Its rate has not been measured. */
typedef struct {
	int64_t n, n_cigar_total, name_bytes;
	const int32_t *tid, *pos; const uint16_t *flag, *n_cigar; const uint8_t *mapq;
	const uint32_t *cigar_off, *cigar;   /* cigar_off relative to this call's cigar[] */
	const uint64_t *name_off;            /* record i's name: names + name_off[i], NUL-terminated, names packed back to back in record order */
	const char *names;
	const uint64_t *name_hash;
} ssv_aln_cols;
int ssv_aln_pack(ssv_ctx *ctx, const ssv_batch_t *b, const ssv_names_t *names, ssv_aln_cols *out);

/* Copy a device batch into host arrays owned by the context (valid until the next call): tests and debugging. */
int ssv_batch_to_host(ssv_ctx *ctx, const ssv_batch_t *device_batch, ssv_batch_t *host_batch);

/* ---- measurement --------------------------------------------------------------------------- */

/*
 * Per-kernel launch timing with HIP events on the context's stream.  Enable, run, then read back.
 * name = kernel name as in DESIGN.md ("clip_scan", "getsv_scan", ...).  Returns SSV_E_ARG for an
 * unknown name.  Reading synchronises and resets nothing; ssv_prof_reset clears.
 */
int ssv_prof_enable(ssv_ctx *ctx, int on);
int ssv_prof_reset(ssv_ctx *ctx);
int ssv_prof_get(ssv_ctx *ctx, const char *name, double *total_ms, int64_t *launches, int64_t *units);
/* Names of all timed kernels, '\n' separated. */
const char *ssv_prof_names(void);

/* ---- clipped-sequence re-aligner ----------------------------------------------------------------------
 * Stand-in for the EXTERNAL `bwa mem` step between `seeksv getclip` and `seeksv getsv` (README.md:22-34, example/seeksv.sh:3:
 * `bwa mem ref.fa prefix.clip.fq.gz | samtools view -Sb - > prefix.clip.bam`) on hosts without bwa, for references that behave
 * like random sequence (the synthetic genomes of bench.py / tests).  getsv consumes of each clip.bam record: flag & {4, 16, 256},
 * MAPQ == 0 or not, tid, pos, the CIGAR with its S ends, the read name = the sequence (getsv.cpp:25-71, getsv.h:445-527).
 * K-mer index of the reference in HBM + seed look-ups on both strands + ungapped extension with bwa mem's default scores
 * (match 1, mismatch 4, end clipping 5, minimum 30).  NOT bit-identical to bwa: no gaps unless asked for (one), no chaining, one
 * record per query unless its other loci (ssv_realign_query_alts: up to 1 + 16) or - for whole reads - its second piece as a
 * supplementary record (ssv_realign_query_split: 1 + 1, never a third piece) are asked for. */
typedef struct {
	int32_t tid;         /* -1: unaligned (flag 4) */
	int32_t pos;         /* 0-based reference position of the aligned segment's first base */
	int32_t q_beg, q_end;/* aligned segment [q_beg, q_end) of the query as a BAM record stores it (reverse-complemented when `reverse`): CIGAR = q_beg S, M, rest S */
	int32_t score;       /* matches - 4 * mismatches of the segment */
	int32_t second;      /* best score at another locus (0: none) */
	int32_t n_mismatch;
	uint8_t reverse;     /* flag 16 */
	uint8_t mapq;        /* 0 when another locus scores as well, 60 when the runner-up is >= 10 behind */
	uint8_t pad[2];      /* pad[0]: SSV_RA_F_* of the query's seed set - written by the sorted index only (the hash index writes 0), also for an unaligned query; pad[1]: 0 */
} ssv_realign_hit;
#define SSV_RA_F_MASKED 1   /* a 20-mer of the query occurs more than max_occ times among the indexed positions and gave no seed */
#define SSV_RA_F_OVERFLOW 2 /* the query has more seeds than candidate slots (192): the rarest were followed, some were left out */
#define SSV_RA_F_ALT_CUT 4  /* ssv_realign_query_alts only: more loci qualified as alternates than max_alt */

/* Build the index.  ref2bit: base i of the concatenated contigs at bits [2 (i % 32), +2) of word i / 32, A C G T = 0 1 2 3 (the
 * caller decides what N becomes); target_off[n_targets + 1] = first base of every contig, target_off[0] = 0, target_off[n_targets] =
 * n_bases.  SSV_MEM_DEVICE arrays are used in place and need one readable word after the last one.  *n_dropped (optional) = sampled
 * positions that found no slot within the probe limit (low-complexity sequence). */
int ssv_realign_index(ssv_ctx *ctx, const uint64_t *ref2bit, int32_t mem, int64_t n_bases, const int64_t *target_off, int32_t n_targets, int64_t *n_dropped);
/* The same reference as a SORTED index, for references with repeats: the sampled 20-mers sorted, equal ones next to each other with ascending positions;
 * nothing is dropped and there is no probe limit.  Same arguments, checks and 32-bit sample limit as ssv_realign_index; max_occ in 1..65535 (else
 * SSV_E_ARG) is bwa mem's -c: a query 20-mer with more occurrences gives no seed (SSV_RA_F_MASKED).  Queries on this index admit their seeds rarest first -
 * by class ceil(log2(occurrences)), then strand, query offset, reference position - until the 192 candidate slots are full (SSV_RA_F_OVERFLOW when seeds
 * were left out), and candidates equal in score, strand and diagonal go to the smaller contig id: every field of a hit is a function of the input.
 * Building either kind of index replaces the other; ssv_realign_query uses the one that was built last; ssv_realign_free frees either. */
typedef struct {
	int64_t n_indexed;   /* sampled positions whose 20-mer lies inside one contig */
	int64_t n_distinct;  /* distinct 20-mers among them */
	int64_t occ_max;     /* occurrences of the most frequent one */
	int64_t n_over_cap;  /* distinct 20-mers with more than max_occ occurrences */
} ssv_realign_index_stats;
int ssv_realign_index_sorted(ssv_ctx *ctx, const uint64_t *ref2bit, int32_t mem, int64_t n_bases, const int64_t *target_off, int32_t n_targets, int32_t max_occ,
                             ssv_realign_index_stats *stats /* may be NULL */);
/* Align n ASCII sequences (host memory, concatenated; seq_off[n + 1]) -> hits[n] (host).  Queries shorter than 20 or longer than 1024
 * bases come back unaligned. */
int ssv_realign_query(ssv_ctx *ctx, const char *seqs, const uint64_t *seq_off, int64_t n, ssv_realign_hit *hits);
/* The same with one insertion or deletion per alignment (`seeksv realign -g`).  The first stage keeps candidates that score 20 or more (second still
 * counts those at 30 or more only), then the winner - and only the winner - is tried with one gap of 1..16 bases on either side of its segment
 * (bwa mem's scores: a gap of L costs 6 + L): the winner's segment keeps one end and becomes one piece, the other piece is the best segment on the
 * neighbouring diagonal that starts (ends) at the gap, extended to the query's end by the rule of the ungapped stage.  The gapped alignment replaces
 * the ungapped one when it scores strictly more: pos, q_beg, q_end, score, n_mismatch (inserted bases are not counted) and mapq (from the new score
 * and the unchanged second) are updated, tid, reverse, second and pad[0] stay.  Of equal gapped alignments: the leftmost gap, then the shorter gap,
 * a deletion before an insertion.  A hit below 30 after this is unaligned in every field but pad[0].  Gaps longer than 16 bases, a second gap and
 * the runner-up are not looked at.  Works on the index that was built last; arguments and errors as ssv_realign_query, gaps[n] (host) is required. */
typedef struct {
	int32_t q_at;        /* query base (in the hit's orientation) behind the gap's left edge */
	int32_t len;         /* > 0: deletion of len reference bases before query base q_at; < 0: query bases [q_at, q_at - len) are inserted; 0: none */
} ssv_realign_gap;
int ssv_realign_query_gapped(ssv_ctx *ctx, const char *seqs, const uint64_t *seq_off, int64_t n, ssv_realign_hit *hits, ssv_realign_gap *gaps);
/* ssv_realign_query (gapped == 0) or ssv_realign_query_gapped (gapped != 0) + the query's OTHER loci (`seeksv realign -S`), as bwa mem -a users feed them to
 * getsv: secondary records that still make junctions.  hits[n] (and gaps[n]) are bit for bit those of the plain calls apart from SSV_RA_F_ALT_CUT.
 * Rule: the candidates and their scores are those of the query's first stage on the index that was built last; best = the primary's score there (in gapped
 * mode: before the refinement).  A candidate is an alternate locus when its score is >= 30 and 5 * score >= 4 * best (bwa mem's XA ratio 0.8) and it is not
 * the locus - same strand, same contig, diagonals at most 32 apart: the window of `second` - of the primary or of an alternate chosen before it.  They are
 * chosen greedily by score (descending), strand (forward first), diagonal (ascending), contig id (ascending); at most max_alt (1..16) are kept, and when
 * more loci qualified the primary's pad[0] gets SSV_RA_F_ALT_CUT.  An alternate's hit: tid, pos, q_beg, q_end, score, n_mismatch, reverse of its own
 * diagonal by the primary's rule (best segment inside the seed's contig + end extension), second = best, mapq = 0, pad[0] = the primary's, pad[1] = 0.
 * An unaligned, too short or too long query has none.  Limits: alternates are not gap-refined (with `gapped` they come from the first stage, need 30 or more
 * there, and a primary that the refinement leaves unaligned has none); at most 16; on the hash index a query with more than 192 seeds keeps the candidates
 * it happened to keep (as its primary does), and a primary tied in score, strand and diagonal between two contigs is the lanes' choice there, the other
 * contig's candidate then being an alternate (the sorted index decides both); no supplementary records here (ssv_realign_query_split has them).
 * alt_off[n + 1] (host): query i's alternates are alts[alt_off[i] .. alt_off[i + 1]), in the rule's order; alts (host) needs room for n * max_alt hits,
 * alt_off[n] are written.  Errors as the other query calls; SSV_E_ARG also for max_alt outside 1..16, a NULL alt_off or alts, gapped without gaps.
 * n == 0: SSV_OK and alt_off[0] = 0. */
int ssv_realign_query_alts(ssv_ctx *ctx, const char *seqs, const uint64_t *seq_off, int64_t n, int32_t max_alt, int32_t gapped,
                           ssv_realign_hit *hits, ssv_realign_gap *gaps /* required iff gapped */,
                           int64_t *alt_off /* n + 1 */, ssv_realign_hit *alts /* room for n * max_alt; alt_off[n] are written */);
/* ssv_realign_query for WHOLE reads that may cross a breakpoint (`seeksv realign -P`; its records are what getsv -F reads): the primary and, where the read
 * has one, a second piece of another diagonal as mates[i] (a supplementary record, flag 2048).  Ungapped, on the index that was built last; the candidates,
 * their scores and segments and the primary P are ssv_realign_query's.  Every interval is in the READ's orientation: a segment [b, e) is [b, e) on the
 * forward strand and [n - e, n - b) on the reverse strand; shared(X, Y) = the length of the two intervals' intersection.
 * Mate M: a scored candidate with another (strand, contig, diagonal) than P, score >= 30 after its end extension, ordered against P (P begins before it
 * begins and ends before it ends, or the other way round; neither contains the other, equal begins or equal ends do not count) and with at least 20 bases
 * of its own on both sides: len(P) - shared >= 20 and len(M) - shared >= 20.  The pieces may overlap (getsv reads that as microhomology) or leave a gap; the
 * locus window of `second` plays no part (a 20-base deletion gives a mate).  Of several: the largest score, then the forward strand, the smaller diagonal,
 * the smaller contig id.  With a mate, `second` of X in {P, M} is the largest score among the scored candidates that are not X's locus (window 32), are not
 * the other piece and share >= 20 bases of the read with X (0: none), and mapq follows from it: hits[i].second / mapq may then differ from the plain
 * call's, no other field does.  mates[i]: tid, pos, q_beg, q_end, score, n_mismatch, reverse of its own diagonal by the primary's rule, second and mapq as
 * above, pad[0] = the primary's, pad[1] = 0.  Without a mate (also: unaligned, too short, too long) mates[i] is the unaligned hit with the primary's pad[0]
 * and hits[i] is bit for bit ssv_realign_query's.  Limits: two pieces only; the mate needs a 20-mer seed of its own (23 matching bases in a row); pieces
 * are not gap-refined; on the hash index the candidates of a query with more than 192 seeds and a tie between two contigs are the lanes' choice as before.
 * Arguments and errors as ssv_realign_query; mates[n] (host) is required (NULL: SSV_E_ARG).  n == 0: SSV_OK. */
int ssv_realign_query_split(ssv_ctx *ctx, const char *seqs, const uint64_t *seq_off, int64_t n, ssv_realign_hit *hits, ssv_realign_hit *mates);
/* ssv_realign_query_split + its records, built on the device (`seeksv run -P`): what `seeksv realign -P` writes into its BAM, as an SSV_MEM_DEVICE batch of the
 * kind ssv_samdec_decode hands out - hot columns, cigar_ends, record lines, every CIGAR operation, every record's packed bases + qualities, 8 readable bytes
 * behind seqqual, n_tid_runs = 0, max_ref_span = 1024 - which ssv_rt_scan (of any context on the same GPU) takes in place.  *out and *out_names are owned by
 * the context and stay valid until its next ssv_realign_* call.  hits[n] and mates[n] (host, both required) are bit for bit ssv_realign_query_split's.
 *   quals      NULL, or seq_off[n] bytes: read i's qualities (phred + 33) at seq_off[i], as long as its bases
 *   names      read i's NUL-terminated name at names + name_off[i]; name_off[n] = the bytes of names.  *out_names is the uploaded blob; a read's two records
 *              share one offset
 *   rows       read i gives one record, and a second one directly behind it when mates[i].tid >= 0; row order is read order.  flag 0 / 16 / 4, | 2048 on the
 *              mate's record; mapq the hit's (0 when unaligned); tid / pos the hit's or -1 / -1; l_qseq = L; mtid = mpos = -1; isize = 0; xc = 0; CIGAR q_beg S
 *              (when > 0), (q_end - q_beg) M, (L - q_end) S (when > 0) - none, and cigar_ends 0xff, when unaligned.  Bases: A C G T in either case 1 2 4 8, every
 *              other byte 15; a flag-16 record holds the reversed complement and the reversed qualities; the low nibble behind an odd L is 0.  Qualities:
 *              byte - 33, 0xff throughout when quals is NULL.  Reads shorter than 20 or longer than 1024 bases are unaligned records with all their bases.
 *              seq_off values are the library's choice (every record's bytes start dword aligned).
 * Errors as ssv_realign_query_split; SSV_E_ARG also for a NULL names, name_off, out or out_names and - found on the host before anything is launched - for a
 * name of 0 or more than 254 bytes; SSV_E_STATE before an index is built; n == 0: SSV_OK and out->n == 0.  Synchronises the stream.  Timed as `realign_rows`
 * (the query itself: `realign_query`). */
int ssv_realign_split_batch(ssv_ctx *ctx, const char *seqs, const uint64_t *seq_off, int64_t n, const char *quals, const char *names, const uint64_t *name_off,
                            ssv_realign_hit *hits, ssv_realign_hit *mates, ssv_batch_t *out, ssv_names_t *out_names);
int ssv_realign_free(ssv_ctx *ctx);

/* ---- getsv -F: junctions from read-through split alignments: replaces FindJunction (process_bwasw.cpp:5-227, seeksv.cpp:221-225) -----------
 * The file's records go through ssv_rt_scan batch by batch in file order (their bases are needed: keep_all_seq).  A record is kept unless
 * mapq < min_mapq, it is unmapped or a duplicate, its first or last CIGAR operation is H, both are S or both are M (code 0), it has no CIGAR or its
 * tid is not a contig.  Kept records are paired by read name in file order as the reference's std::map does; ssv_rt_finish returns one line per pair
 * in the order of the record that completed it: the junction, its microhomology, the two seqs and the CIGAR sources of the two SeqInfo values.  The
 * caller applies them to its junction map in that order (find: insert, or count against the found entry's seq lengths).  Calls out of sequence:
 * SSV_E_STATE. */
typedef struct {
	int32_t min_mapq;          /* -w, default 1 */
	int32_t n_targets;
	const int32_t *name_rank;  /* [n_targets] host: the contig's place when the header's names are sorted byte-wise (make_pair(chr, pos) < compares names) */
} ssv_rt_params;
typedef struct {
	int32_t up_tid, up_pos, down_tid, down_pos; /* the junction (1-based positions) */
	int8_t up_strand, down_strand;              /* '+' / '-' */
	int16_t kind;                               /* construction case, process_bwasw.cpp:94-197: 0/1 same strand (microhomology / none), 2/3 opposite, 5' sides, 4/5 opposite, 3' sides */
	int32_t microhomology;
	int32_t up_left_clipped, up_right_clipped, down_left_clipped, down_right_clipped;
	int32_t up_len, down_len;                   /* the seqs: up at seqs + seq_off, down right behind it */
	int32_t up_cig_n, down_cig_n;               /* the CIGAR sources (GenerateCigar: S and H dropped): up at cigars + cig_off, down behind it, BAM encoding */
	int32_t up_cig_edit, down_cig_edit;         /* 0 as is, 1 MinusCigarRight(microhomology), 2 AddCigarLeft(microhomology) (clip_reads.cpp:507-558) */
	uint64_t seq_off, cig_off;
	int64_t first_record, second_record;        /* file-order indices of the held record and of the one that completed the pair */
} ssv_rt_pair;
typedef struct {
	int64_t n_pairs;
	int64_t n_candidates;                       /* kept records */
	const ssv_rt_pair *pairs;                   /* host memory owned by the context, valid until the next ssv_rt_begin */
	const char *seqs;
	const uint32_t *cigars;
} ssv_rt_result;
int ssv_rt_begin(ssv_ctx *ctx, const ssv_rt_params *p);
int ssv_rt_scan(ssv_ctx *ctx, const ssv_batch_t *b, const ssv_names_t *names);
int ssv_rt_finish(ssv_ctx *ctx, ssv_rt_result *out);

/* ---- run -A: junctions from the supplementary alignments of the original itself (v9, additive) --------------------------------------------
 * ssv_rt_begin_original opens the session of ssv_rt_begin in another mode: ssv_rt_scan, ssv_rt_finish, ssv_rt_pair and ssv_rt_result are the same calls
 * with the same rows, and a session opened with ssv_rt_begin behaves byte for byte as before.  The batches are the ORIGINAL's (an aligner's output: a read
 * that spans a breakpoint is a primary record plus a supplementary record, flag 2048, each clipped on one side) in input order, decoded in the decoders'
 * default form (keep_all_seq == 0 ships the bases of every record with S at an end, which is every record that carries the read).  The rule is this
 * project's own: FindJunction's geometry, kept byte for byte, with a selection and a key of its own.
 *
 * A record takes part when all of these hold:
 *   - it has a CIGAR;
 *   - tid is a contig of the header;
 *   - mapq >= min_mapq;
 *   - none of 0x4, 0x100, 0x400 is set, as the input has them;
 *   - exactly one of its two ends is clipped.  An end is clipped when its outermost operation is S or H.
 * S..S, H..S, H..H and records with no clipped end are not taken, 10I90M and 100= included (FindJunction sends those last two through its 3' branch).
 *
 * Lengths come from the CIGAR alone:
 *   - R is the sum of M I S = X H;
 *   - the clip length of the clipped end is the sum of the run of S / H operations at that end (5H10S85M: 15);
 *   - a 5' clipped record (first operation a clip): side '5', left = clip, right = R - left, pos = pos0 + 1;
 *   - otherwise: side '3', right = clip, left = R - right, pos = pos0 + ref_len, with GenerateCigar's ref_len (M D = N, not X).
 *
 * A record carries the read when it has no H, its bases are present (seq_off != SSV_NO_SEQ) and l_qseq == R.
 *
 * The key is (read name, flag & 0xC0) in the place of the read name alone: mates never meet; single-end reads have 0 there.
 *
 * Hold / pair / drop runs in input order per key, as for ssv_rt_begin.  A held A and a new B pair when all of these hold, looked at in this order:
 *   - same strand and different sides, or opposite strands and the same side;
 *   - R_A == R_B (else B counts as dropped_length);
 *   - at least one of the two carries the read (else B counts as dropped_no_carrier).
 * Otherwise B is dropped and A stays held.
 *
 * Junction, microhomology, kind, clipped lengths, CIGAR sources and edits are ssv_rt_begin's case analysis unchanged.  The two seqs are the slices
 * (source record, begin, len, rc) that case analysis names; when the source carries the read they are read as for ssv_rt_begin, when it does not the
 * same bases are read from its partner: (begin, len, rc) on the same strand, (R - begin - len, len, !rc) on opposite strands.  Complementing swaps
 * A C G T only.  A record whose R is above 2^30 never pairs.
 *
 * What the pass does not see: marks made later (-M / -D), a restriction (-L / -X), a sort (-u: it runs in input order, which matters only for
 * opposite-strand pairs at equal (contig, position), where the completing record is up, and for keys with more than two candidates).  A read of three
 * or more pieces gives what hold / pair / drop gives: no chaining.
 * Errors as ssv_rt_begin's; calls out of sequence: SSV_E_STATE.  ssv_rt_original_stats: the counts of the last finished session of this mode
 * (SSV_E_STATE before one has finished, after a session of the other mode, or after the next begin). */
typedef struct {
	int64_t candidates;          /* records that took part */
	int64_t hard_clipped;        /* ... of which with an H */
	int64_t pairs;
	int64_t pairs_borrowed;      /* pairs of which a seq was read from the partner of its source */
	int64_t dropped_no_carrier;  /* records dropped at the pairing because neither record carried the read */
	int64_t dropped_length;      /* records dropped at the pairing because R_A != R_B */
	int64_t store_bytes;         /* device memory the candidates took at the finish: lines, hashes, names, bases and operations */
} ssv_rt_original_counts; /* (a typedef and a function cannot share a name in C) */
int ssv_rt_begin_original(ssv_ctx *ctx, const ssv_rt_params *p);
int ssv_rt_original_stats(ssv_ctx *ctx, ssv_rt_original_counts *out);

/* ---- run -A -S: junctions from SA tags whose supplementary record is absent (v9, additive) ----------------------------------------------------
 * ssv_rt_begin_original_sa opens the session of ssv_rt_begin_original in one more mode: a record that carries the read and has an SA value of exactly one
 * entry also contributes a VIRTUAL CANDIDATE built from that entry, which is used only when its source record found no real partner.  Batches go through
 * ssv_rt_scan_aux (ssv_rt_scan with a descriptor of where the records' optional fields lie: ssv_aux_t, from ssv_bamdec_aux / ssv_samdec_aux or the
 * caller's own); ssv_rt_finish, ssv_rt_pair, ssv_rt_result and ssv_rt_original_stats are the same calls with the same rows.  A session opened with
 * ssv_rt_begin or ssv_rt_begin_original behaves byte for byte as before and launches nothing of this mode.
 *
 * 1. Who gets a virtual candidate.  A SOURCE is a record that takes part under ssv_rt_begin_original's rule and carries the read (no H, bases present,
 *    l_qseq == R).  Only a source has its optional fields looked at.  A hard-clipped record never gets a virtual candidate: a virtual candidate never
 *    carries the read, so the pair would have no bases.
 * 2. Finding the value.
 *    BAM: the typed fields are walked as libbam does: A c C s S i I f d Z H B; an unknown type ends the walk.  The first field with tag SA and type Z is
 *    taken; SA with another type is passed over.  Nothing is read beyond the record's block_size: a Z or H value with no NUL before the record's end, or a
 *    B array that runs over it, ends the walk with no value.
 *    SAM text: optional fields start at field 12.  A field matches only when it begins with "SA:Z:" directly behind a tab ("XA:Z:...SA:Z:..." inside
 *    another value is no match).  The value ends at the tab, at a '\r' before the newline, at the newline, or at the end of the last line.
 * 3. The value's grammar: rname,pos,strand,CIGAR,mapQ,NM; - one entry, parsed as written:
 *      - rname runs up to the first ','; it may hold ';', ':' and '*';
 *      - pos is decimal, 1 to 2^31-1, stored minus 1;
 *      - strand is '+' or '-';
 *      - CIGAR is one or more operations of MIDNSHP=X, each with a length below 2^28, at most 65535 of them;
 *      - mapQ is decimal, 0 to 255;
 *      - NM is a run of digits (at least one) and is ignored;
 *      - the entry ends with ';'; a missing final ';' at the value's end is accepted.
 *    Anything else is sa_refused: no virtual candidate and no error.  Bytes behind the first entry's ';' make it sa_multi: no virtual candidate (a read of
 *    three or more pieces stays unchained).  rname must be a contig of the header, by exact name: else sa_refused.
 * 4. The virtual candidate is what a record with that tid, pos0, strand and CIGAR would give under ssv_rt_begin_original's rule.  S in an SA CIGAR stands
 *    for the record's H; both are clips.
 *      - exactly one end must be clipped, and mapQ >= min_mapq: failing either is sa_refused;
 *      - R, the clip run, ref_len, side, left, right and pos come from the same formulas;
 *      - it shares its source's name, key, mate bits and record index;
 *      - it has no bases and never carries the read; it holds its non-clip operations; it is marked, and knows its source.
 * 5. Pairing.  Under one key, pairing has two phases.
 *    Phase 1: hold / pair / drop over the real candidates alone, in input order: every outcome and every count is exactly ssv_rt_begin_original's with the
 *    virtual candidates absent.
 *    Phase 2: every real candidate that left phase 1 with no partner and is nobody's partner (held, or dropped), if it owns a virtual candidate, pairs with
 *    it when the strand / side test passes and R_source == R_virtual (unequal: sa_dropped_length).  The source is A, the held record; the virtual candidate
 *    is B, the completing record, and its row stands where a record right behind the source would have completed it.  A virtual candidate whose source
 *    found a real partner is sa_redundant.
 *    The result does not depend on where the input is cut into batches: that is why virtual candidates stay out of phase 1.
 * 6. Everything behind the pairing is unchanged: junction, microhomology, kind and CIGAR sources by ssv_rt_begin's case analysis; a seq that names the
 *    virtual side is read from the source by ssv_rt_begin_original's slice rule (it counts among pairs_borrowed).
 *
 * Contig names: target_names[n_targets], host, NUL-terminated, read during the call.  Errors as ssv_rt_begin_original's; out of sequence: SSV_E_STATE -
 * ssv_rt_scan_aux outside a session of this mode, ssv_rt_scan inside one, ssv_rt_original_sa_stats before such a session has finished or after the next
 * begin; a descriptor that does not belong to the batch (n != batch n, bad mem or encoding, a host span outside bytes): SSV_E_ARG. */
enum { SSV_AUX_BAM = 0, SSV_AUX_SAM = 1 };
/* Where the optional fields of a batch's records lie, beside ssv_batch_t and ssv_names_t: record i's are the len[i] bytes at base + off[i], BAM's typed
 * fields (up to the record's block_size) or SAM text (from field 12 to the line's end).  mem as in ssv_names_t (SSV_MEM_HOST: base[bytes], off[n] and len[n]
 * are copied to the GPU; SSV_MEM_DEVICE: used in place, bytes unused). */
typedef struct {
	int32_t mem;
	int32_t encoding;       /* SSV_AUX_BAM / SSV_AUX_SAM */
	int64_t n;              /* records described: the batch's n */
	const uint8_t *base;
	const uint64_t *off;
	const uint32_t *len;
	int64_t bytes;
} ssv_aux_t;
/* The optional fields of the last chunk ssv_bamdec_decode / ssv_samdec_decode handed out, in HBM (valid as long as that batch).  Computed by a kernel of
 * its own on the context's stream when the call is made; a run that never asks launches nothing. */
int ssv_bamdec_aux(ssv_ctx *ctx, ssv_aux_t *out);
int ssv_samdec_aux(ssv_ctx *ctx, ssv_aux_t *out);
typedef struct {
	int64_t sa_tags;            /* sources with an SA:Z value: sa_multi + sa_refused + virtuals */
	int64_t sa_multi;           /* ... whose value holds more than one entry */
	int64_t sa_refused;         /* ... whose entry is not in the grammar, names no contig, fails the ends rule or the MAPQ floor */
	int64_t virtuals;           /* virtual candidates made */
	int64_t sa_redundant;       /* ... whose source found a real partner */
	int64_t pairs_from_sa;      /* ... that completed a pair (counted in ssv_rt_original_counts.pairs too) */
	int64_t sa_dropped_length;  /* ... dropped because R_source != R_virtual */
} ssv_rt_original_sa_counts;
int ssv_rt_begin_original_sa(ssv_ctx *ctx, const ssv_rt_params *p, const char *const *target_names);
int ssv_rt_scan_aux(ssv_ctx *ctx, const ssv_batch_t *b, const ssv_names_t *names, const ssv_aux_t *aux);
int ssv_rt_original_sa_stats(ssv_ctx *ctx, ssv_rt_original_sa_counts *out);

/* ---- duplicate read pairs marked while the sample is retained (v9, additive; `seeksv run -M`, `seeksv somatic -K -M`) ----------------------
 * Every pass honours the duplicate flag 0x400; this stage sets it, in the retained copy only, before any pass reads a flag.  The rule is this library's own (it
 * follows `samtools rmdup` where it can; no external duplicate marker was run or matched).  Records come in file order, coordinate sorted; a RUN is a maximal
 * stretch of consecutive records with equal (tid, pos).
 *   takes part  flag & 0x1 set, none of 0x4 | 0x8 | 0x100 | 0x800 | 0x400 set, tid >= 0 and mtid >= 0 (a record that arrives with 0x400 stays marked and takes
 *               no part); every other record is never touched
 *   head        takes part and (tid, pos) < (mtid, mpos), or the two are equal and flag & 0x40; every other record that takes part is a tail
 *   group       heads with equal (tid, pos, mtid, mpos, flag & 0x10, flag & 0x20): inside one run
 *   score       0 when l_qseq == 0 or the first quality byte is 0xff, else the sum of the quality bytes that are >= 15 (32 bits)
 *   keeper      the group's highest score, among equal scores the earliest in the file; every other head of the group gets flag |= 0x400
 *   digest      64-bit FNV-1a (offset 1469598103934665603, prime 1099511628211) over the read name's bytes without the NUL, then over four little-endian
 *               int32: a head's (tid, pos, mtid, mpos), a tail's (mtid, mpos, tid, pos) - a tail computes its head's digest from its own fields
 *   tail        gets flag |= 0x400 iff its digest equals that of some marked head whose run is not later than the tail's own run
 * SSV_DUP_DIGEST_BITS=k in the environment at ssv_dup_begin keeps the digest's low k bits (tests: forced collisions follow the same rule).
 * Limits: aligned pos / mpos, not unclipped 5' ends (two copies clipped differently are not found); single reads and pairs with an unmapped end are never
 * marked; libraries (RG / LB) are not told apart; a pair is scored by its head alone.
 *
 * ssv_dup_retain takes the place of ssv_batch_retain for a stream of device batches in file order (names: the batch's read names, as ssv_rt_scan takes them).
 * The last run of a batch may go on in the next one, and its keeper may lie there: the call holds back the batch's trailing run (the maximal suffix with the
 * last record's (tid, pos); none when that record has tid < 0 - such records take no part) and puts it in front of the next call's records.  *out is a
 * retained batch like ssv_batch_retain's (given back with ssv_batch_release): the *carried records held back before, then this batch's records up to its own
 * trailing run - with last != 0 everything.  Every flag in *out is final on return; out->n may be 0; cigar_off / seq_off are those of *out's own arrays;
 * max_ref_span covers both parts; tid_runs is NULL.  The concatenation of all *out is the input, record for record, with the rule's flags, however the stream
 * was cut.  *out keeps bases + qualities only for records whose first or last CIGAR operation is S (the others get SSV_NO_SEQ): the input must carry the
 * qualities of every record that takes part (decode with keep_all_seq).
 * Errors leave everything as it was: NULL arguments, a host batch, a record that takes part without its qualities: SSV_E_ARG; (tid, pos) going down between two
 * neighbouring records with tid >= 0 (the held-back run included): SSV_E_ARG "not coordinate sorted"; no ssv_dup_begin, or a call after `last`: SSV_E_STATE.
 * SSV_DUP_SET_SLOTS=n (tests): the digest set starts with n slots (a power of two; it is kept at most half full and doubles).
 * Timed as dup_select, dup_mark, dup_retain. */
typedef struct {
	int64_t records;      /* records handed out in all *out so far */
	int64_t taking_part;  /* of them: records that take part */
	int64_t groups;       /* groups that were looked at: those with a head in a run of two or more records */
	int64_t heads_marked, tails_marked;
	int64_t set_entries;  /* distinct digests in the set */
	int64_t held_max;     /* the longest hold-back, in records */
} ssv_dup_stats;
int ssv_dup_begin(ssv_ctx *ctx);
int ssv_dup_retain(ssv_ctx *ctx, const ssv_batch_t *device_batch, const ssv_names_t *names, int last, ssv_batch_t *out, int64_t *carried);
/* Ends the stream (also one that was not ended with `last`: what is still held back is dropped) and hands the counts out. */
int ssv_dup_finish(ssv_ctx *ctx, ssv_dup_stats *out);

/* ---- an original in any record order, coordinate sorted while it is retained (v9, additive; `seeksv run -u`) -----------------------------------
 * THE RULE.  The records of in[0 .. n_in) are one sequence: batch order first, then record order.  A record's key is (t, p): t = tid < 0 ? n_targets : tid
 * (unplaced records come last), p = (uint32_t)(pos + 1) (position -1 in front of position 0).  The output is that sequence stably sorted by (t, p): records
 * with equal keys keep their input order.  This is the comparison of libbam 0.1.x's sorter (contig, then position, nothing else); newer samtools also breaks
 * ties by strand.  No external sorter was run or matched, and equality with the output of any one of them is not claimed.  (seeksv's results depend on the
 * order of ties only through BAM order inside a clip bin.)
 *
 * in: batches of ssv_batch_retain / ssv_dup_retain / an earlier ssv_batch_sort (anything else: SSV_E_ARG).  A contig id >= n_targets: SSV_E_ARG; 2^32 records
 * or more in total: SSV_E_RANGE (the sort carries a record's index as 32 bits); no memory: SSV_E_NOMEM.  On failure the inputs are untouched and still the
 * caller's.  On success they are released by the call (in[] is zeroed) and out->batches are the caller's, each given back with ssv_batch_release like any
 * retained batch: the records in sorted order, cut into batches of at most max_out_records records (0: 16 M, or SSV_SORT_BATCH_RECORDS from the environment -
 * tests), earlier where a batch would reach 2^31 records or 2^32 CIGAR operations.  Every field of every record is unchanged - hot columns, cigar_ends, the
 * whole line with xc and cigar_head, all operations, the bases + qualities of the records that had them (packed back to back as the decoders pack them;
 * SSV_NO_SEQ stays SSV_NO_SEQ) - except cigar_off / seq_off, which are those of the new batch.  max_ref_span: the maximum over the inputs (0 when one of them
 * did not know); tid_runs: filled up to the decoders' 64 runs, NULL above.
 * Already sorted - (t, p) never goes down, inside and across the batches: the inputs are handed back as out->batches (the same device memory, nothing copied,
 * no sort or gather kernel launched), already_sorted = 1.
 * change_*: the contig changes among the records without UNMAP|MUNMAP (flag & 12 == 0), the list ssv_bamdec_info.tid_run_index / tid_run_tid carries, continued
 * across the output batches from contig 0: batch b's changes are [change_first[b], change_first[b + 1]), change_index counts inside ITS batch.
 * Memory: inputs and outputs are resident together (twice the retained sample) plus 24 bytes a record of keys and indices.  Synchronises the stream.
 * Timed as sort_keys (check, keys, change lists), sort_radix, sort_gather (sizes, scans, gather). */
typedef struct {
	int64_t n_records, n_batches;
	int32_t already_sorted, pad;
	ssv_batch_t *batches;          /* [n_batches] host array owned by the context until the next ssv_batch_sort */
	const int64_t *change_first;   /* [n_batches + 1] into change_index / change_tid */
	const uint32_t *change_index;  /* record index inside its batch ... */
	const int32_t *change_tid;     /* ... and its contig */
} ssv_sorted;
int ssv_batch_sort(ssv_ctx *ctx, ssv_batch_t *in, int64_t n_in, int32_t n_targets, int64_t max_out_records, ssv_sorted *out);

/* ---- duplicate read pairs by the unclipped 5' ends of both reads, in any record order (v9, additive; `seeksv run -D`, `seeksv somatic -K -D`) ----
 * A second rule beside ssv_dup_retain's, for what that one cannot see: copies of one fragment that the aligner clipped differently, and input that is not
 * coordinate sorted.  Mates are joined by read name, so nothing here depends on record order.  This is Picard's comparison in outline; the rule is this
 * library's own, no external duplicate marker was run or matched.
 * THE RULE.  The records of all batches are one sequence in input order: batch order first, then record order.  A record's index in it is g (< 2^32, else
 * SSV_E_RANGE).
 *   takes part  flag & 0x1 set, none of 0x4 | 0x8 | 0x100 | 0x800 | 0x400 set, tid >= 0, mtid >= 0 and n_cigar > 0 (a record that arrives with 0x400 keeps it
 *               and takes no part); every other record is never touched
 *   end u       64-bit signed, may be negative.  Forward (!(flag & 0x10)): pos minus the lengths of the leading run of S / H operations.  Reverse: pos +
 *               reference span (M D N = X) - 1 + the lengths of the trailing run of S / H operations
 *   name hash   64-bit FNV-1a (offset 1469598103934665603, prime 1099511628211) over the read name's bytes without the NUL; SSV_DUP_DIGEST_BITS=k in the
 *               environment keeps the low k bits (tests: names that collide follow the same rule)
 *   mates       the records that take part and have equal name hash form a name group.  A name group is a PAIR iff it has exactly two records, exactly one of
 *               them has 0x40, each record's (mtid, mpos) equals the other's (tid, pos), and each record's 0x20 agrees with the other's 0x10.  The records
 *               of every other name group are left untouched and counted as `unpaired`
 *   key         a = the record with the smaller (tid, u, reverse), on a tie the one with 0x40; b = the other.  key = (tid_a, u_a, rev_a, tid_b, u_b, rev_b),
 *               compared exactly (the pairs are ordered by the key itself, not by a hash of it)
 *   score       the sum over both records of the quality bytes >= 15 (32 bits); a record with l_qseq == 0 or first quality byte 0xff adds 0
 *   keeper      the group's (pairs of equal key) highest score; among equal scores the pair whose smaller g is smallest.  Both records of every other pair
 *               of the group get flag |= 0x400
 * When no two pairs of a group have equal scores, the set of marked records does not depend on the input order.
 * Limits: libraries (RG / LB) are not told apart; which mate is first of pair is not part of the key; single reads and pairs with an unmapped end are never
 * marked; a name that occurs on more than two primary records is left alone.
 *
 * ssv_pairdup_retain takes the place of ssv_batch_retain for a batch decoded with keep_all_seq, and its names (ssv_bamdec_names or ssv_samdec_names; as
 * ssv_rt_scan takes them).  *out has the form of ssv_dup_retain's output: bases + qualities only for records whose first or last operation is S (the others
 * get SSV_NO_SEQ), cigar_off / seq_off those of *out's own arrays, tid_runs as the decoder gave them; given back with ssv_batch_release.  Behind the other
 * parts of the batch's memory sits one 24-byte row per record - { uint64 name_hash; int64 u; uint32 score; uint32 kind } - kind 1: the record takes part,
 * 0: it does not and the row is all zero.  ssv_pairdup_rows hands out where they lie (device memory; tests).  Errors leave everything as it was: NULL
 * arguments, a host batch, a record that takes part without its qualities: SSV_E_ARG; no memory: SSV_E_NOMEM.
 *
 * ssv_pairdup_mark works over all retained batches at once, in place: the flags of the rule are written into the record lines of batches[0 .. n).  Batches
 * that are not ssv_pairdup_retain's, one given twice, or batches a call has marked already: SSV_E_ARG; no memory: SSV_E_NOMEM; on any failure nothing is
 * changed.  Afterwards the rows are dead and the batches are ordinary retained batches (ssv_batch_sort takes them and carries their flags like every
 * other field).  Memory: 8 bytes a record, 32 bytes a record that takes part and 32 bytes a pair of temporaries, given back on return together with what the retain calls kept between them (20 bytes a record of the largest batch).  No pass is
 * quadratic in the size of a group.  Synchronises the stream.  Timed as pairdup_ends (retain), pairdup_join (compaction, name sort, join, pairs),
 * pairdup_mark (key sorts, pick and scatter). */
typedef struct {
	int64_t records;      /* records in all batches */
	int64_t taking_part;  /* of them: records that take part */
	int64_t unpaired;     /* of those: records whose name group is no pair */
	int64_t pairs;
	int64_t groups_many;  /* groups of two or more pairs */
	int64_t pairs_marked; /* pairs whose two records got 0x400 */
} ssv_pairdup_stats;
int ssv_pairdup_retain(ssv_ctx *ctx, const ssv_batch_t *device_batch, const ssv_names_t *names, ssv_batch_t *out);
int ssv_pairdup_rows(ssv_ctx *ctx, const ssv_batch_t *batch, const void **dev_rows);
int ssv_pairdup_mark(ssv_ctx *ctx, ssv_batch_t *batches, int64_t n, ssv_pairdup_stats *stats);

/* ---- the records that stay resident restricted to a list of regions (v9, additive; `seeksv run -L`, `-X`, `seeksv somatic -K -L`, `-X`) ----------------
 * THE RULE.  It follows `samtools view -L` in outline; the rule is this library's own, no external tool was run or matched.
 *   regions     a region is (tid, s, t), 0-based half-open as in BED, 0 <= s < t.  The list that goes to the device is NORMALISED per contig by the host:
 *               sorted by s, regions that overlap or abut merged, t clipped to the contig's length, a region left empty by the clipping dropped
 *   interval    a record's interval is [pos, e), all of it in 64 bits: span = the sum of the lengths of its M, D, N, = and X operations, e = pos + max(span, 1).
 *               A record without CIGAR, or whose operations consume no reference, covers one base; so does an unmapped read placed at its mate's
 *               position.  pos == -1 gives [-1, 0), whatever the CIGAR says: it overlaps nothing
 *   overlap     a record overlaps the list iff tid >= 0 and some region of contig tid has s < e and pos < t.  A record with tid < 0 (or tid >= n_targets)
 *               overlaps nothing.  No flag bit takes part in the decision
 *   include     (exclude == 0, -L) a record is kept iff it overlaps
 *   exclude     (exclude != 0, -X) a record is kept iff it does not overlap; unplaced records stay
 *   output      kept records keep their order and every field - hot columns, cigar_ends, the whole line with xc and cigar_head, all operations, the bases +
 *               qualities of the records that had them (SSV_NO_SEQ stays SSV_NO_SEQ) - except cigar_off / seq_off, which are those of the output's own
 *               arrays, packed back to back as the decoders pack them
 * After merging, the last region of the contig with s < e decides: the record overlaps iff that region exists and its t > pos.
 *
 * ssv_regions_set takes the host list, already normalised (n == 0 is a valid list: -L then keeps nothing, -X everything).  A list that is not - unsorted,
 * overlapping or abutting entries, s >= t, s < 0, tid outside [0, n_targets) - gives SSV_E_ARG and leaves the list of before.  ssv_regions_clear removes the
 * list and gives the stage's memory back.  On the device the list is an offsets array of n_targets + 1 entries and two arrays s[], t[]; a contig's regions
 * are staged in LDS while a tile of records stays on that contig, up to ssv_region_lds_capacity() of them, and searched in global memory otherwise.
 *
 * ssv_region_retain takes the place of ssv_batch_retain for a decoder's batch: *out is a retained batch (ssv_batch_release) that holds only the kept records;
 * the input is untouched.  When every record is kept *out equals ssv_batch_retain's output part for part.
 * ssv_batch_select takes a retained batch - of ssv_batch_retain, ssv_dup_retain, an earlier ssv_batch_sort or ssv_batch_select, or ssv_pairdup_retain AFTER
 * ssv_pairdup_mark (before the mark its rows would be orphaned: SSV_E_ARG; anything else: SSV_E_ARG).  On success `in` is released by the call and zeroed.
 * When every record is kept `in` is handed back as *out: the same device memory, no gather launched, info->uncopied = 1.
 * Both: info carries the counts, the contig changes of *out among its records without UNMAP|MUNMAP (flag & 12 == 0; index inside *out, contig - the list
 * ssv_bamdec_info.tid_run_index / tid_run_tid carries; host memory of the context's, valid until the next of these calls) and the contig of the last such
 * record, which the caller passes back as last_tid with the next batch (0 at the start, as in the decoders).  out->n may be 0: the batch is empty and is
 * still given back with ssv_batch_release.  max_ref_span is the input's; tid_runs are filled as ssv_batch_sort fills them.  No list set: SSV_E_STATE; a host
 * batch or NULL arguments: SSV_E_ARG; no memory: SSV_E_NOMEM; every error leaves the input valid and the caller's.  Memory between calls: up to 15 bytes
 * a record of the largest input and 34 bytes a kept record of temporaries, until ssv_regions_clear.  Synchronises the stream.  Timed as region_select (flags, scan,
 * sizes, change lists) and region_gather. */
typedef struct { int32_t tid, s, t; } ssv_region;
typedef struct {
	int64_t n_in, n_kept;
	int32_t uncopied;              /* 1: ssv_batch_select handed its input back */
	int32_t last_tid;              /* contig of the last record without UNMAP|MUNMAP so far */
	uint32_t n_changes, pad;
	const uint32_t *change_index;  /* record index inside *out ... */
	const int32_t *change_tid;     /* ... and its contig */
} ssv_region_info;
int ssv_regions_set(ssv_ctx *ctx, const ssv_region *regions, int64_t n, int32_t n_targets, int exclude);
int ssv_regions_clear(ssv_ctx *ctx);
int ssv_region_lds_capacity(void);
int ssv_region_retain(ssv_ctx *ctx, const ssv_batch_t *device_batch, int32_t last_tid, ssv_batch_t *out, ssv_region_info *info);
int ssv_batch_select(ssv_ctx *ctx, ssv_batch_t *in, int32_t last_tid, ssv_batch_t *out, ssv_region_info *info);

#ifdef __cplusplus
}
#endif
#endif /* SEEKSV_HIP_H_ */
