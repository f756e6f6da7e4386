/*
 * yams_mi355x_accel.h — C ABI of libyams_mi355x_accel.so, the MI355X (gfx950) drop-in for the
 * YAMS vector-scan / SHA-256 / content-defined-chunking hot path.
 *
 * Two layers, both plain C (pointers + sizes, no C++ or torch types):
 *
 *   1. The flat `yams_accel_*` / `yams_scan_*` / `yams_sha256_*` / `yams_cdc_*` functions below.
 *      Data pointers marked "device" are HIP device addresses (e.g. a torch tensor's data_ptr());
 *      pointers marked "host" are ordinary memory.  All work is enqueued on the context's HIP
 *      stream; functions that hand results back to the host synchronise that stream themselves.
 *
 *   2. The YAMS plugin surface (include/yams/plugins/abi.h:26-34 in the reference): the eight
 *      `yams_plugin_*` entry points plus three vtables — `vector_scan_v1`, `content_hash_v1`,
 *      `chunker_v1` — written to the conventions of the reference's
 *      include/yams/plugins/model_provider_v1.h:44-49 (first field abi_version, second `self`,
 *      every function returns yams_status_t, plugin-allocated buffers are released only through
 *      the paired free_* of the same vtable).  The reference has no plugin interface for these
 *      three seams today (its seams are the C++ classes IVectorBackend / IContentHasher /
 *      IChunker); INTEGRATION.md shows the host-side adapter a maintainer adds.
 *
 * What each entry point replaces in the reference (paths under /root/reference):
 *   yams_scan_topk_*          SqliteVecBackend::Impl::bruteForceSearchUnlocked fast path,
 *                             src/vector/sqlite_vec_backend.cpp:4115-4135,4204-4331, batched as
 *                             searchSimilarBatch (:1612-1647), and for YAMS_SCAN_L2 the vec0 path
 *                             vec0SearchUnlocked (:4450-4530).
 *   yams_sha256_*             crypto::SHA256Hasher::hash / init / update / finalize,
 *                             src/crypto/sha256_hasher.cpp:81-109,167-195.
 *   yams_cdc_chunk_*          RabinChunker::chunkDataLazy (src/chunking/rabin_chunker.cpp:63-152)
 *                             and StreamingChunker::chunkData (include/yams/chunking/
 *                             streaming_chunker.h:146-204, src/chunking/streaming_chunker.cpp:37-137).
 *   yams_scan_doc_topk_*      the exact arm of document-level selection, sqlite_vec_backend.cpp:1508-1518 + :86-125
 *                             (retainBestRecordPerDocument), with the reduction on the device.
 *   yams_ingest_*             the hash + chunk_file phases of ContentStore::store,
 *                             src/api/content_store_impl.cpp:199-231 (caller contract only).
 *
 * There is NO CPU fallback behind this ABI: without a gfx950 device every compute entry point
 * returns YAMS_ERR_UNSUPPORTED.
 */
#ifndef YAMS_MI355X_ACCEL_H
#define YAMS_MI355X_ACCEL_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__) || defined(__clang__)
#define YAMS_ACCEL_API __attribute__((visibility("default")))
#else
#define YAMS_ACCEL_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes: numerically identical to yams_status_e, model_provider_v1.h:17-25. */
typedef int yams_status_t;
#ifndef YAMS_PLUGINS_MODEL_PROVIDER_V1_H
enum yams_status_e {
    YAMS_OK = 0,
    YAMS_ERR_INVALID_ARG = 1,
    YAMS_ERR_NOT_FOUND = 2,
    YAMS_ERR_IO = 3,
    YAMS_ERR_INTERNAL = 4,
    YAMS_ERR_UNSUPPORTED = 5,
    YAMS_ERR_TIMEOUT = 6,            /* a sharded batch missed its deadline: the handle is stuck (see yams_scan_sharded_wait) */
    YAMS_ERR_RESOURCE_EXHAUSTED = 7  /* device (or pinned host) memory could not be had; the object is left as it was */
};
#endif

#define YAMS_ACCEL_VERSION_STRING "0.7.0" /* yams_route_index_* / yams_route_dense_*: the cluster router's dense signal over a resident index */

/* ------------------------------------------------------------------------------------------ */
/* Context                                                                                      */
/* ------------------------------------------------------------------------------------------ */
typedef struct yams_accel_ctx yams_accel_ctx;

/* Number of visible HIP devices (0 when there is no GPU or no driver). */
YAMS_ACCEL_API int yams_accel_device_count(void);
/* Create a context bound to `device`.  `hip_stream` may be NULL (the context creates its own
 * non-blocking stream) or an existing hipStream_t on which all work of this context is enqueued.
 * NOTE: the handle of HIP's legacy default stream IS the null pointer — a caller that passes it
 * (torch.cuda.current_stream().cuda_stream is 0 unless a torch.cuda.Stream is current) gets the
 * context's own stream, and work it queued on the default stream (tensors still being filled) is
 * NOT ordered with the context's: synchronise first, or pass a created stream.  A context is
 * single-threaded; create one per host thread (mirrors "one SHA256Hasher per thread",
 * src/crypto/sha256_hasher.cpp:34). */
YAMS_ACCEL_API yams_status_t yams_accel_ctx_create(int device, void* hip_stream,
                                                   yams_accel_ctx** out_ctx);
YAMS_ACCEL_API void yams_accel_ctx_destroy(yams_accel_ctx* ctx);
YAMS_ACCEL_API yams_status_t yams_accel_ctx_synchronize(yams_accel_ctx* ctx);
/* Sweep gate: contexts of ONE device that serve concurrent search calls share a gate, and their big filter
 * sweeps then run one after the other on the GPU (stream-ordered: the host never waits) while everything
 * around them — query preparation, candidate selection, the fp64 re-score — overlaps the other context's
 * sweep.  Without a gate two concurrent sweeps interleave workgroup by workgroup and evict each other's
 * tiles from L2.  The plugin's pool of search contexts shares one gate per device (plugin.cpp); the
 * reference serves concurrent searches under a shared lock (vector_database.cpp:539,618).
 * A gate must outlive the contexts attached to it; attach with NULL to detach. */
typedef struct yams_accel_gate yams_accel_gate;
YAMS_ACCEL_API yams_status_t yams_accel_gate_create(int device, yams_accel_gate** out_gate);
YAMS_ACCEL_API void yams_accel_gate_destroy(yams_accel_gate* gate);
YAMS_ACCEL_API yams_status_t yams_accel_ctx_set_gate(yams_accel_ctx* ctx, yams_accel_gate* gate);
/* Sweep hold — for callers that put a COLLECTIVE behind every batch themselves (one process per GPU:
 * yams_scan_topk_device, then an RCCL all-gather of the record on a side stream, then the merge).  The filter sweep is
 * a persistent grid that owns every CU of the device; a collective kernel enqueued while another context's sweep runs
 * would wait for a CU under it and keep its peers on the other GPUs spinning meanwhile.  With the hold on, the gate
 * stays CLOSED behind this context's sweeps: no other context of the gate starts a sweep until this one calls
 * yams_accel_ctx_release_sweep_hold(ctx, stream) — after it has enqueued its collective (+ merge) on `stream`; the next
 * sweep then starts behind that work.  (yams_scan_sharded_* does the same for its own lanes: YAMS_SHARDED_FENCE_AUTO.)
 * Release on every path, also after a failed scan; releasing without a hold is a no-op. */
YAMS_ACCEL_API yams_status_t yams_accel_ctx_set_sweep_hold(yams_accel_ctx* ctx, int on);
YAMS_ACCEL_API yams_status_t yams_accel_ctx_release_sweep_hold(yams_accel_ctx* ctx, void* hip_stream);
/* Human-readable description of the last failure on this context (static storage, never NULL). */
YAMS_ACCEL_API const char* yams_accel_last_error(const yams_accel_ctx* ctx);
/* Device properties as a JSON string (malloc'd; release with yams_accel_free_string). */
YAMS_ACCEL_API yams_status_t yams_accel_device_info_json(yams_accel_ctx* ctx, char** out_json);
YAMS_ACCEL_API void yams_accel_free_string(char* s);
/* The library keeps the call-sized device buffers of its host-streaming entry points (yams_ingest_host: up to four of 8 GiB)
 * in a process-wide pool between calls — allocating them anew cost every call hundreds of milliseconds — up to 40 GiB per
 * process; the pool is emptied when one of the library's own allocations fails, and by this call.  device < 0: every device.
 * Returns the bytes handed back to the driver. */
YAMS_ACCEL_API uint64_t yams_accel_trim(int device);
/* Plain device memory helpers for hosts that do not bring their own allocator. */
YAMS_ACCEL_API yams_status_t yams_accel_malloc(yams_accel_ctx* ctx, size_t bytes, void** out_dev);
YAMS_ACCEL_API void yams_accel_free(yams_accel_ctx* ctx, void* dev);
YAMS_ACCEL_API yams_status_t yams_accel_upload(yams_accel_ctx* ctx, void* dst_dev,
                                               const void* src_host, size_t bytes);
YAMS_ACCEL_API yams_status_t yams_accel_download(yams_accel_ctx* ctx, void* dst_host,
                                                 const void* src_dev, size_t bytes);
/* HIP-event timing of the most recent call's dominant kernel on the context's stream:
 * average milliseconds per launch and number of launches (bench.py's roofline leg). */
YAMS_ACCEL_API yams_status_t yams_accel_last_kernel_ms(const yams_accel_ctx* ctx,
                                                       const char* kernel, double* out_ms_per_launch,
                                                       uint64_t* out_launches);
YAMS_ACCEL_API yams_status_t yams_accel_enable_kernel_timing(yams_accel_ctx* ctx, int enable);

/* ------------------------------------------------------------------------------------------ */
/* Exact vector scan (batched cosine / L2 top-k)                                                */
/* ------------------------------------------------------------------------------------------ */
typedef enum yams_scan_metric_e {
    YAMS_SCAN_COSINE = 0, /* exact_scan engine, sqlite_vec_backend.cpp:4204-4331 */
    YAMS_SCAN_L2 = 1      /* vec0_l2 engine,    sqlite_vec_backend.cpp:4450-4530 */
} yams_scan_metric_t;

/* A dense device mirror of `vectors WHERE embedding_dim = dim ORDER BY rowid`
 * (sqlite_vec_backend.cpp:4140-4175): row-major fp32, raw (not normalised). */
typedef struct yams_scan_corpus_s {
    const float* rows;         /* device, [n_rows][dim], 16-byte aligned                          */
    uint64_t n_rows;           /* < 2^32 per shard                                                */
    uint32_t dim;              /* embedding dimension                                             */
    uint32_t reserved;
    const uint32_t* tie_rank;  /* device, nullable: tie_rank[row] = rank of the row's chunk_id in
                                  lexicographic order (the reference's secondary sort key,
                                  :4218-4223).  NULL means rank == row_base + row.               */
    const uint32_t* rank_row;  /* device, nullable iff tie_rank is: inverse permutation within this
                                  shard for single-shard corpora (rank_row[tie_rank[r]] == r)     */
    int64_t row_base;          /* added to local row ordinals in the outputs (shard base)         */
    const uint32_t* row_mask;  /* device, nullable: bit (r & 31) of word (r >> 5) set = row r takes
                                  part in the search.  This is the `AND document_hash = ?` /
                                  `AND document_hash IN (...)` restriction of the reference's scan
                                  (sqlite_vec_backend.cpp:4137-4175): masked-out rows are neither
                                  visited nor evaluated.  ceil(n_rows / 32) words.               */
    uint64_t row_mask_count;   /* number of set bits (the host built the mask, it knows)          */
    const uint16_t* rows_bf16; /* device, nullable: the SHADOW of `rows` built by
                                  yams_scan_build_shadow_device — [n_rows][dim] bf16 (round to
                                  nearest even) of the unit-normalised rows, 16-byte aligned.  Only the MFMA filter reads it
                                  (half the bytes, no conversion in the loop); the fp64 re-score
                                  that decides the result always reads `rows`.  Results are
                                  bit-identical with and without it.                              */
    const float* rows_nsq;     /* device, nullable iff rows_bf16 is: [n_rows] fp32 squared norms  */
    const int8_t* rows_i8;     /* device, nullable: the INT8 SHADOW built by
                                  yams_scan_build_shadow_i8_device — YAMS_SCAN_I8_SHADOW_BYTES(n_rows,
                                  dim) bytes of int8 = round(unit-normalised row / s_b), in the
                                  blocked layout that call writes (opaque to callers), 16-byte
                                  aligned, dim % 64 == 0, dim >= 256.
                                  Read by the first filter tier of cosine searches (half the bytes
                                  of the bf16 shadow, twice its matrix rate); like every filter
                                  tier it only proposes candidates, the fp64 re-score over `rows`
                                  decides: results are bit-identical with and without it.
                                  L2 searches take the same tier when the view also carries rows_nsq
                                  (i.e. both shadows), the row norms of the shard are within a factor
                                  of two of each other and at most 64 rows have a squared norm outside
                                  (1e-30, 1e30) (zero / overflowing / non-finite rows: carried along as
                                  unconditional candidates); checked per call, otherwise L2 stays on
                                  the bf16 tier.                                                      */
    const float* rows_i8_meta; /* device, nullable iff rows_i8 is: [ceil(n_rows / 64)][2] =
                                  {s_b, e_b} per block of 64 rows: the block's quantisation scale
                                  and the largest measured residue |x/|x| - s_b * int8 row| of
                                  its rows                                                         */
    uint32_t stripe_rows;      /* 0: a contiguous shard, global id = row_base + local row.  Else the
                                  corpus is dealt to n_stripes shards in stripes of stripe_rows
                                  rows (how a growing mirror stays balanced over devices): local
                                  row L of this shard is global row  row_base +
                                  ((L / stripe_rows) * n_stripes + stripe_index) * stripe_rows +
                                  L % stripe_rows.  Local order == global order within a shard,
                                  so the default tie-break (row id) stays the reference's.        */
    uint32_t n_stripes;
    uint32_t stripe_index;
    uint32_t i8_flags;         /* YAMS_SCAN_I8_*: the layout rows_i8 was built in — what
                                  yams_scan_build_shadow_i8_layout_device was given (0 for
                                  yams_scan_build_shadow_i8_device).  (was: reserved2, 0)            */
} yams_scan_corpus_t;

/* int8 shadow layouts.  ROTATED: rows (and, per batch, queries) go through a fixed orthogonal map — sign flips and two
 * overlapping Walsh-Hadamard transforms — before they are quantised: dot products and norms stay where they were, the
 * energy of a few large components (outlier dimensions of an embedding model, a power-law spectrum) spreads over all of
 * them and the measured residue — the width of the filter's bound — drops from ~0.05 to ~0.01.  Rows with uniform
 * components quantise better WITHOUT it; yams_scan_choose_i8_layout_device measures both on a sample.  256 <= dim <= 4096.
 * Like every filter property it changes candidate counts, never results. */
#define YAMS_SCAN_I8_ROTATED 1u

#define YAMS_SCAN_FLAG_DEFER_THRESHOLD 1u /* L2 only: do not apply similarity_threshold (a sharded
                                             caller applies it after merging per-shard lists)  */
#define YAMS_SCAN_FLAG_FORCE_EXACT 2u     /* skip the MFMA filter, score every row in fp64       */
#define YAMS_SCAN_FLAG_F32_FILTER 4u      /* use the exact-f32 MFMA filter instead of the bf16 ones */
#define YAMS_SCAN_FLAG_SPLIT_FILTER 8u    /* start with the split-bf16 (3-pass) filter instead of
                                             the single-pass bf16 one                            */
#define YAMS_SCAN_FLAG_RECORD_PATH 16u    /* cosine: the reference's record path, taken when a search
                                             carries metadata_filters (sqlite_vec_backend.cpp:
                                             4333-4409).  Same fp64 arithmetic
                                             (computeCosineSimilarity), but rows are dropped when
                                             norm^2 < 1e-10 (isZeroNormEmbedding, :204-211) instead of
                                             <= 1e-12 (:4267-4269).  The caller turns the metadata
                                             predicate into the row allow-mask.                  */
#define YAMS_SCAN_FLAG_WIDE_TILE 32u      /* keep the 256-query MFMA tile for batches of <= 128
                                             queries (default: the narrow, HBM-bound kernel form);
                                             results are identical, only the kernel form differs  */
#define YAMS_SCAN_FLAG_NO_I8_FILTER 64u   /* do not use the int8 shadow even when the view carries one */
#define YAMS_SCAN_FLAG_RESIDENT_QUERIES 128u /* int8 tier: take the resident-query kernel form whenever its
                                             preconditions hold (dim % 128 == 0, dim <= 768), also on shards
                                             too small for it to balance (default: the library chooses);
                                             with YAMS_SCAN_FLAG_WIDE_TILE: never take it.  Results are
                                             identical, only the kernel form differs              */
/* L2 only — the arithmetic of vec0's distance.  It lives in the ABSENT third_party/sqlite-vec-cpp, so it cannot be
 * pinned from the reference checkout; every definition that dependency can plausibly have is served and
 * the HOST picks the one its build of the library uses (plugin config "l2_accumulate"):
 *   F64    (default) sum (x_i - q_i)^2 in fp64, sequentially, sqrt, round to fp32 — this repository's own definition;
 *   F32    fp32 difference, fp32 product, fp32 sequential sum, sqrtf — the public sqlite-vec's scalar loop;
 *   F32X8  / F32X16  the same with 8 / 16 round-robin partial sums (element i goes to lane i % 8 / 16) added left to
 *          right at the end — its AVX / AVX-512 forms;
 *   ... | FUSED  the three fp32 forms with the square accumulated by one fused multiply-add — those loops as a compiler
 *          emits them under -mfma, the flag the reference's build gives that dependency on x86.
 * include/yams_accel/l2_calibration.hpp finds out which one a host's build uses by asking its own distance function.
 * Each is tested bit for bit against a CPU restatement of that arithmetic (tests/): the order (distance
 * asc, chunk_id asc), the cosine re-score and the threshold-after-top-k of sqlite_vec_backend.cpp:4464-4512 are
 * unchanged.  The filter tiers are the same; the completeness proof widens its margin by the fp32 summation bound. */
#define YAMS_SCAN_FLAG_L2_ACC_F64 0u
#define YAMS_SCAN_FLAG_L2_ACC_F32 256u
#define YAMS_SCAN_FLAG_L2_ACC_F32X8 512u
#define YAMS_SCAN_FLAG_L2_ACC_F32X16 768u
#define YAMS_SCAN_FLAG_L2_ACC_MASK 768u
#define YAMS_SCAN_FLAG_L2_ACC_FUSED 2048u  /* with F32 / F32X8 / F32X16: every square is accumulated by ONE fused multiply-add,
                                                p = fma(d, d, p) with d = fl(x - q) — what `sum += d * d` and
                                                _mm256_add_ps(sum, _mm256_mul_ps(d, d)) compile to under -mfma, which is how the
                                                reference builds sqlite-vec-cpp on x86 (src/vector/meson.build:80-88).  Ignored with F64. */
#define YAMS_SCAN_FLAG_L2_ACC_EXPLICIT 1024u /* vtable callers: the L2_ACC bits of THIS call are the caller's decision even when
                                                they read F64 (= 0) — the plugin's configured default is not applied.  Set by the
                                                adapters after l2_calibration.hpp has asked the host's own distance function. */
#define YAMS_SCAN_MAX_K 1024u  /* results per query and call; larger k: rounds behind the allow-mask, as
                                  AccelVectorIndex::searchPeeled does (include/yams_accel/vector_index.hpp) */
#define YAMS_SCAN_MAX_DIM 8192u /* the fp64 re-score stages a query and its candidate rows in LDS */

typedef struct yams_scan_params_s {
    uint32_t k;                 /* results per query; 0 => empty result (:4123-4126)             */
    float similarity_threshold; /* rows with similarity < threshold are dropped (:4277-4279)     */
    uint32_t metric;            /* yams_scan_metric_t                                            */
    uint32_t flags;
} yams_scan_params_t;

/* Per-call work counters: the VectorSearchDiagnostics subset the exact scan fills
 * (include/yams/vector/vector_types.h:181-204; set at sqlite_vec_backend.cpp:4131-4135,
 * 4229-4251,4327-4329) plus this implementation's own filter statistics. */
typedef struct yams_scan_diag_s {
    uint32_t used_exact_scan;             /* always 1                                            */
    uint32_t rows_visited_observed;       /* always 1                                            */
    uint64_t rows_visited;                /* per query: n_rows (summed over the batch)           */
    uint64_t exact_distance_evaluations;  /* per query: n_rows (summed over the batch)           */
    uint64_t returned_rows;
    uint64_t filter_candidates;           /* rows that passed the MFMA filter (any tier)           */
    uint64_t rescored_rows;               /* rows re-scored in fp64                              */
    uint32_t widened_queries;             /* queries whose candidate set had to be widened       */
    uint32_t exact_fallback_queries;      /* queries that took the full fp64 scan                */
    uint32_t path;                        /* 0 = mfma filter + fp64 re-score, 1 = full fp64 scan: every allowed row is
                                             scored in fp64, no filter.  Which one yams_scan_topk_* takes is a contract
                                             (tests/_score_edges.py restates it), the result is the same bit for bit:
                                             1 from the FUSED ONE-LAUNCH scan (its launch is the timed region
                                             "small_scan" of yams_accel_last_kernel_ms), taken exactly when
                                               1 <= n_rows <= 16384 and n_queries <= 16;
                                               dim % 32 == 0, dim <= 1024, `rows` 16-byte aligned;
                                               k <= 256 and ceil(n_rows / 256) * min(k, 256) <= 1024;
                                               none of FORCE_EXACT, F32_FILTER, SPLIT_FILTER, WIDE_TILE, NO_I8_FILTER,
                                               RESIDENT_QUERIES; under YAMS_SCAN_L2 no fp32-accumulate flag
                                               (YAMS_SCAN_FLAG_L2_ACC_* other than F64);
                                             1 from the exhaustive multi-launch pipeline otherwise when FORCE_EXACT is
                                             set, n_rows < 4096, `rows` is not 16-byte aligned or dim % 4 != 0, an
                                             allow-mask admits fewer than 16384 rows, or (L2) a query norm lies outside
                                             [1e-15, 1e15); 0 in every other case.                                    */
    uint32_t escalated_queries;           /* queries re-filtered with the split (3-pass) filter  */
    uint32_t filter_tier;                 /* first filter tier of the call: 0 none (fp64 scan),
                                             1 int8, 2 bf16, 3 split bf16, 4 f32                  */
    uint32_t retried_queries;             /* int8 tier: queries filtered a second time with the threshold their proof asked for
                                             (the k-th best exact score found), before any escalation (was: reserved)  */
} yams_scan_diag_t;

/* Builds the filter shadow of `n_rows` rows (call it when rows are uploaded or appended; pass
 * pointers offset to the first new row to extend an existing shadow).  One pass: reads 4*dim bytes
 * and writes 2*dim + 4 bytes per row.  dim must be a multiple of 4; rows 16-byte aligned. */
YAMS_ACCEL_API yams_status_t yams_scan_build_shadow_device(yams_accel_ctx* ctx, const float* rows,
                                                           uint64_t n_rows, uint32_t dim,
                                                           uint16_t* out_rows_bf16,
                                                           float* out_rows_nsq);

/* (Re)builds the INT8 shadow of the mirror at `rows` for every block of 64 rows that intersects
 * [first_row, first_row + n_rows) — call it when those rows were uploaded or appended (the rows of a
 * block share one quantisation scale, so an append that starts inside a block re-quantises that
 * block's earlier rows too; all pointers are the BASES of the mirror's arrays, not offset ones).
 * dim must be a multiple of 64 and at least 256, rows 16-byte aligned.  For a mirror of n rows:
 * out_rows_i8 holds YAMS_SCAN_I8_SHADOW_BYTES(n, dim) bytes — the shadow is padded to whole blocks of 64 rows
 * and stored in the order the filter's DMA reads it ([row / 16][dim / 64][16 rows][64 bytes], the 16-byte
 * chunks of a row permuted for conflict-free LDS reads): opaque, build it with this call only; out_meta:
 * [ceil(n / 64)][2] fp32.  out_mean_err (host, nullable): mean residue bound
 * over the rebuilt blocks — a host that sees a large value (say > 0.02: heavy-tailed rows quantise
 * badly) may leave the int8 shadow out of the view and keep the bf16 one; asking for it
 * synchronises the stream. */
#define YAMS_SCAN_I8_SHADOW_ROWS(n_rows) ((((uint64_t)(n_rows)) + 63u) / 64u * 64u)
#define YAMS_SCAN_I8_SHADOW_BYTES(n_rows, dim) (YAMS_SCAN_I8_SHADOW_ROWS(n_rows) * (uint64_t)(dim))
YAMS_ACCEL_API yams_status_t yams_scan_build_shadow_i8_device(yams_accel_ctx* ctx, const float* rows,
                                                              uint64_t first_row, uint64_t n_rows,
                                                              uint32_t dim, int8_t* out_rows_i8,
                                                              float* out_meta, double* out_mean_err);

/* The same with the layout named (YAMS_SCAN_I8_* bits; the view must carry the same bits in i8_flags).  Blocks of one mirror
 * must all be built in one layout: a host that changes its mind rebuilds from row 0. */
YAMS_ACCEL_API yams_status_t yams_scan_build_shadow_i8_layout_device(yams_accel_ctx* ctx, const float* rows,
                                                                     uint64_t first_row, uint64_t n_rows,
                                                                     uint32_t dim, uint32_t i8_flags, int8_t* out_rows_i8,
                                                                     float* out_meta, double* out_mean_err);

/* Which layout quantises these rows better: the mean residue of up to 256 blocks of 64 rows spread over [0, n_rows) under
 * both layouts (host, nullable outputs; nothing on the device is written), *out_i8_flags = YAMS_SCAN_I8_ROTATED when the
 * rotated one is at least a fifth smaller, else 0.  Synchronises the stream.  A host decides once per mirror (first upload). */
YAMS_ACCEL_API yams_status_t yams_scan_choose_i8_layout_device(yams_accel_ctx* ctx, const float* rows, uint64_t n_rows,
                                                               uint32_t dim, uint32_t* out_i8_flags,
                                                               double* out_mean_err_plain, double* out_mean_err_rotated);

/* Batched exact top-k, everything device-resident.  Any batch size: more than 4096 queries run as
 * slices of 4096 (the per-batch workspace grows with the query count); diagnostics are summed.
 *   queries      device [n_queries][dim] fp32 (raw)
 *   out_scores   device [n_queries][k] fp32: cosine similarity (relevance_score, :4323-4326),
 *                best first; unused slots hold -inf
 *   out_rows     device [n_queries][k] int64: row_base + row ordinal; unused slots hold -1
 *   out_counts   device [n_queries] uint32
 *   out_dist     device [n_queries][k] fp32, nullable: L2 distance (YAMS_SCAN_L2 only)
 *   out_ranks    device [n_queries][k] uint32, nullable: tie rank of each hit = corpus.tie_rank[row]
 *                (the row ordinal without a rank table).  SHARD-LOCAL unless the shard's tie_rank table
 *                holds corpus-wide ranks: see yams_scan_merge_topk_device before merging by it
 * Returns YAMS_ERR_INVALID_ARG if any query is non-finite or has norm^2 < 1e-10 (:4127-4130;
 * a batch fails as a whole, :1635-1647), or on a dimension / alignment violation.
 * The call synchronises the context's stream before returning. */
YAMS_ACCEL_API yams_status_t yams_scan_topk_device(yams_accel_ctx* ctx,
                                                   const yams_scan_corpus_t* corpus,
                                                   const float* queries, uint32_t n_queries,
                                                   const yams_scan_params_t* params,
                                                   float* out_scores, int64_t* out_rows,
                                                   uint32_t* out_counts, float* out_dist,
                                                   uint32_t* out_ranks, yams_scan_diag_t* diag);

/* Same, with host-resident queries and outputs (the corpus stays a device mirror). */
YAMS_ACCEL_API yams_status_t yams_scan_topk_host(yams_accel_ctx* ctx,
                                                 const yams_scan_corpus_t* corpus,
                                                 const float* queries_host, uint32_t n_queries,
                                                 const yams_scan_params_t* params,
                                                 float* out_scores_host, int64_t* out_rows_host,
                                                 uint32_t* out_counts_host, float* out_dist_host,
                                                 yams_scan_diag_t* diag);

/* k-way merge of per-shard top-k lists (the step after an RCCL all-gather): inputs are
 * device [n_shards][n_queries][k] arrays laid out exactly as yams_scan_topk_device writes them
 * (ranks nullable => row ids break ties).  Order: similarity desc / distance asc, then rank asc.
 * in_ranks MUST be comparable ACROSS shards, i.e. positions in one corpus-wide chunk_id ordering
 * (:4218-4223) — ranks that each shard numbered on its own (a per-shard tie_rank table, or the row
 * ordinals a shard reports without one) order exact cross-shard ties wrongly.  Callers without a
 * corpus-wide ranking pass in_ranks = NULL (global row ids break ties: right whenever rows were
 * appended in chunk_id order) or use yams_scan_merge_records_device with rank_of_row.
 * For YAMS_SCAN_L2 the similarity_threshold is applied after the merge (:4508-4510): the k nearest first, then the
 * entries with similarity < threshold are dropped and the survivors keep their order (the freed slots are padding, not
 * refilled from behind position k).  THIS entry always applies it: YAMS_SCAN_FLAG_DEFER_THRESHOLD in params->flags is
 * IGNORED here, while yams_scan_merge_records_device honours it (nothing is dropped).  Under cosine the threshold plays
 * no part in either entry (each shard has applied it), and under L2 the ranks play none (equal distances: row id asc).
 * Entries equal in every key (one row id in two shards) keep shard order, then list position.  Lists may be shorter
 * than k or empty (slots at or behind in_counts are never read); n_shards * k <= 8192, else YAMS_ERR_UNSUPPORTED.
 * out_dist (nullable): in_dist of the entry, or 1 - similarity when in_dist is NULL; unused output slots hold
 * -inf / -1 / +inf.  tests/_merge_model.py states this contract in numpy; tests/stress_merge.py holds the kernel to it. */
YAMS_ACCEL_API yams_status_t yams_scan_merge_topk_device(
    yams_accel_ctx* ctx, uint32_t n_shards, uint32_t n_queries, const yams_scan_params_t* params,
    const float* in_scores, const int64_t* in_rows, const uint32_t* in_counts,
    const float* in_dist, const uint32_t* in_ranks, float* out_scores, int64_t* out_rows,
    uint32_t* out_counts, float* out_dist);

/* The packed per-shard result record: what one shard's search writes and what travels between
 * devices (RCCL all-gather in the one-process-per-GPU form, peer copies in the in-process form):
 *   scores f32 [n_queries][k] | rows i64 [n_queries][k] | counts u32 [n_queries]
 *   (| dist f32 [n_queries][k]) (| ranks u32 [n_queries][k]),   every part 16-byte aligned.
 * An absent part has offset UINT64_MAX. */
typedef struct yams_scan_record_layout_s {
    uint64_t scores_off, rows_off, counts_off, dist_off, ranks_off, bytes;
} yams_scan_record_layout_t;
YAMS_ACCEL_API void yams_scan_record_layout(uint32_t n_queries, uint32_t k, int with_dist,
                                            int with_ranks, yams_scan_record_layout_t* out);

/* k-way merge of `n_shards` records lying `record_stride` bytes apart in device memory (e.g. the
 * output of one all-gather, untouched).  Order: similarity desc / distance asc, then the tie rank:
 * the records' own ranks if present, else rank_of_row[row - rank_row_base] if given (device; the
 * corpus-wide chunk_id ranking, :4218-4223), else the global row id. */
YAMS_ACCEL_API yams_status_t yams_scan_merge_records_device(
    yams_accel_ctx* ctx, uint32_t n_shards, uint32_t n_queries, const yams_scan_params_t* params,
    const void* records, uint64_t record_stride, const yams_scan_record_layout_t* layout,
    const uint32_t* rank_of_row, int64_t rank_row_base, float* out_scores, int64_t* out_rows,
    uint32_t* out_counts, float* out_dist);

/* One search over a corpus row-sharded across the devices of this node — what a host's
 * searchSimilarBatch (sqlite_vec_backend.cpp:1612-1647) calls when the corpus does not fit one GPU.
 * ONE process, one RCCL communicator over the shard devices (ncclCommInitAll; librccl.so.1 is bound
 * with dlopen when the first communicator is needed), per batch: every shard's exact top-k into a packed
 * record, ONE ncclAllGather of the records on a side stream, merge_topk_kernel on the first shard's
 * device, the merged result downloaded into pinned memory.  A persistent worker thread per (shard, lane)
 * drives its device; `lanes` batches are in flight: the upload, the query preparation and the sample pass of
 * batch i + 1 run under the sweep of batch i, and the exchange of batch i runs in the gap before the sweep of
 * batch i + 1 (see YAMS_SHARDED_FENCE_* below; submit / wait below; yams_scan_sharded_topk_host is submit + wait).
 * `devices[i]` is the HIP device of shard i.  Shards that SHARE a device cannot form a communicator (RCCL
 * refuses two ranks on one device): such handles — the parity tests of a one-GPU box — move their records
 * with device-to-device copies instead.  shards[i] is shard i's view (device pointers valid on devices[i];
 * row_base / stripe fields give global ids); upload and build shadows through yams_scan_sharded_ctx(s, i).
 * rank_of_row (nullable): device array on devices[0], the global tie ranking — needed only when
 * the shards carry tie_rank arrays (then each shard's tie_rank must be a local permutation that
 * preserves the global order). */
typedef struct yams_scan_sharded yams_scan_sharded;
#define YAMS_SHARDED_COLLECTIVE_AUTO 0u /* RCCL when there are >= 2 shards, each on its own device, and the
                                           communicator can be formed; else device-to-device copies of the
                                           records (one shard: nothing to exchange)                         */
#define YAMS_SHARDED_COLLECTIVE_RCCL 1u /* require the communicator — also for ONE shard (a communicator of one
                                           rank: all-gather + merge still run); creation fails with
                                           YAMS_ERR_UNSUPPORTED when the library cannot be loaded or initialised,
                                           YAMS_ERR_INVALID_ARG when shards share a device and the default
                                           library is used (RCCL refuses two ranks on one device; a library named
                                           in `rccl_library` decides for itself)                            */
#define YAMS_SHARDED_COLLECTIVE_PEER 2u /* never RCCL: device-to-device copies                               */
/* The filter sweep is a persistent grid that owns every CU of its device (one 160 KiB-LDS, 8 x 256-VGPR
 * workgroup per CU), and a collective is a CU-resident kernel that spins on its peers.  Left to float, the
 * all-gather of batch i on GPU g would have to find a CU under the sweep of batch i + 1 and then wait for GPU
 * h's copy of the kernel, itself queued behind h's sweep: the sweeps of different GPUs get coupled through the
 * few CUs the collective holds.  So with >= 2 shards the exchange is FENCED: on every shard the sweep of batch
 * i + 1 begins only after that shard's part of the exchange of batch i (on the root shard also the merge and the
 * download) has completed — the collective never shares a device with a sweep.  Everything in front of the sweep
 * (query upload, preparation, the sample pass) still overlaps — the sample pass in its half-tile form while a
 * fence (or a sweep hold) is installed: its resident-query form would be a second grid that owns every CU, and
 * the exchange of batch i may still be on the device when it starts.  YAMS_SHARDED_FENCE_OFF lifts the fence
 * (measurements only). */
#define YAMS_SHARDED_FENCE_AUTO 0u
#define YAMS_SHARDED_FENCE_OFF 1u
typedef struct yams_scan_sharded_options_s {
    uint32_t struct_size; /* sizeof(yams_scan_sharded_options_t); the 16-byte round-3 struct is accepted */
    uint32_t lanes;       /* batches in flight, 1..16; 0 = 2                                      */
    uint32_t collective;  /* YAMS_SHARDED_COLLECTIVE_*                                            */
    uint32_t fence;       /* YAMS_SHARDED_FENCE_*                                                 */
    const char* rccl_library; /* nullable: the collective library to dlopen instead of librccl.so.1 — any library
                                 that exports ncclGetVersion / ncclCommInitAll / ncclAllGather / ncclCommDestroy /
                                 ncclGetErrorString with RCCL's signatures (a site build of RCCL; the test suite's
                                 stream-ordered stand-in, which lets several ranks share one device).  The string
                                 is copied. */
    uint32_t exchange_timeout_ms; /* deadline of wait(): a batch whose scan + exchange has not completed by then makes
                                 wait() return YAMS_ERR_TIMEOUT with a diagnosis in ..._last_error, the communicator is
                                 aborted and the handle is STUCK (submit fails, destroy does not block).  0 = 30000;
                                 UINT32_MAX = wait for ever (the round-4 behaviour) */
    uint32_t reserved0;
} yams_scan_sharded_options_t;
YAMS_ACCEL_API yams_status_t yams_scan_sharded_create(const int* devices, uint32_t n_shards,
                                                      yams_scan_sharded** out);
YAMS_ACCEL_API yams_status_t yams_scan_sharded_create_ex(const int* devices, uint32_t n_shards,
                                                         const yams_scan_sharded_options_t* options,
                                                         yams_scan_sharded** out);
YAMS_ACCEL_API uint32_t yams_scan_sharded_lanes(const yams_scan_sharded* s);
/* {"shards":n,"lanes":l,"devices":[..],"collective":"rccl"|"peer_copy"|"none","fenced":true|false,"rccl_version":..,
 *  "rccl_library":"<path the symbols came from>","communicator_ranks":<ncclCommCount of the root's communicator>,
 *  "batches":..,"collectives":..,"exchanges_timed":..,"exchange_ms":<mean device time of all-gather + merge + download
 *  on the root shard's side stream, the wait for the slowest peer included>,"exchange_ms_max":..,
 *  "exchange_timeout_ms":..,"stuck":true|false}; malloc'd, release with yams_accel_free_string. */
YAMS_ACCEL_API yams_status_t yams_scan_sharded_info_json(yams_scan_sharded* s, char** out_json);
/* The context lane `lane` uses on shard `shard` (kernel timings of a pipelined run; the plugin's per-call
 * row masks live in its workspace).  yams_scan_sharded_ctx(s, i) is lane 0's. */
YAMS_ACCEL_API yams_accel_ctx* yams_scan_sharded_lane_ctx(yams_scan_sharded* s, uint32_t shard, uint32_t lane);
/* Pipelined use: acquire a lane (wait != 0: block until one is free; else YAMS_ERR_NOT_FOUND when every lane
 * has a batch in flight), submit a batch on it — the queries are copied into the lane's pinned staging, the
 * call returns at once —, submit the next batch on another lane, wait() for the first: it returns the merged
 * result and frees the lane.  The shard views, and rank_of_row, must stay valid until wait() returns.
 * A batch fails as a whole (:1635-1647); a failed batch still takes part in its collective, so the handle
 * stays usable.  Lanes are independent: different host threads may drive different lanes concurrently. */
#define YAMS_SHARDED_SUBMIT_DIAG 1u /* fill the diagnostics wait() returns (costs one more look at the result counts) */
YAMS_ACCEL_API yams_status_t yams_scan_sharded_lane_acquire(yams_scan_sharded* s, int wait, uint32_t* out_lane);
YAMS_ACCEL_API void yams_scan_sharded_lane_release(yams_scan_sharded* s, uint32_t lane); /* a lane acquired but not submitted */
YAMS_ACCEL_API yams_status_t yams_scan_sharded_submit(
    yams_scan_sharded* s, uint32_t lane, const yams_scan_corpus_t* shards, const float* queries_host,
    uint32_t n_queries, const yams_scan_params_t* params, const uint32_t* rank_of_row,
    int64_t rank_row_base, uint32_t flags);
YAMS_ACCEL_API yams_status_t yams_scan_sharded_wait(
    yams_scan_sharded* s, uint32_t lane, float* out_scores_host, int64_t* out_rows_host,
    uint32_t* out_counts_host, float* out_dist_host, yams_scan_diag_t* diag);
YAMS_ACCEL_API void yams_scan_sharded_destroy(yams_scan_sharded* s);
YAMS_ACCEL_API uint32_t yams_scan_sharded_count(const yams_scan_sharded* s);
YAMS_ACCEL_API yams_accel_ctx* yams_scan_sharded_ctx(yams_scan_sharded* s, uint32_t shard);
YAMS_ACCEL_API const char* yams_scan_sharded_last_error(const yams_scan_sharded* s);
YAMS_ACCEL_API yams_status_t yams_scan_sharded_topk_host(
    yams_scan_sharded* s, const yams_scan_corpus_t* shards, const float* queries_host,
    uint32_t n_queries, const yams_scan_params_t* params, const uint32_t* rank_of_row,
    int64_t rank_row_base, float* out_scores_host, int64_t* out_rows_host,
    uint32_t* out_counts_host, float* out_dist_host, yams_scan_diag_t* diag);

/* Allocation-failure injection, for tests of the out-of-memory paths (ErrorCode::ResourceExhausted,
 * include/yams/core/types.h:49 of the reference).  After yams_accel_debug_fail_alloc_after(n) the next n allocations of
 * device / pinned / VMM-backed memory THIS LIBRARY makes for its own objects (workspaces, mirrors behind corpus_append,
 * lane buffers, staging rings, digest sets) succeed and every later one fails as hipErrorOutOfMemory does, until
 * yams_accel_debug_fail_alloc_after(-1).  Process-wide; never armed unless called (the library reads no environment).
 * yams_accel_alloc — the caller's own buffers — is exempt.  ..._alloc_faults: allocations failed by injection so far.
 * What the library promises under exhaustion: the failing call returns YAMS_ERR_RESOURCE_EXHAUSTED, the object it
 * was growing is left as it was (a corpus keeps its rows and answers searches), nothing is leaked (health JSON:
 * "mirror_bytes_mapped" / "mirror_bytes_parked"), and the same call succeeds once memory is there again.
 * MEASUREMENT BUILD ONLY (libyams_mi355x_accel_measure.so, -DYAMS_ACCEL_MEASURE): in the product library the three entry points
 * exist — one ABI for both builds — and do nothing: no code in a host process can arm allocation failures there, and the
 * allocation paths carry no check.  yams_accel_debug_alloc_injection_compiled() says which build this is (1 / 0). */
YAMS_ACCEL_API void yams_accel_debug_fail_alloc_after(int64_t n);
YAMS_ACCEL_API uint64_t yams_accel_debug_alloc_faults(void);
YAMS_ACCEL_API int yams_accel_debug_alloc_injection_compiled(void);

/* Fill a device matrix with the synthetic embedding recipe: Philox4x32-10
 * (seed, row, col/4) -> U[-1,1) -> fp32 L2-normalise.  Used by bench.py and tests so that a
 * corpus larger than host RAM can be generated in HBM and any slice regenerated on the CPU. */
YAMS_ACCEL_API yams_status_t yams_synth_rows_device(yams_accel_ctx* ctx, uint64_t seed,
                                                    uint64_t row0, uint64_t n_rows, uint32_t dim,
                                                    float* out_dev);
YAMS_ACCEL_API yams_status_t yams_synth_bytes_device(yams_accel_ctx* ctx, uint64_t seed,
                                                     uint64_t blob_id0, uint64_t n_blobs,
                                                     uint64_t blob_len, uint8_t* out_dev);

/* ------------------------------------------------------------------------------------------ */
/* The product-quantised engine: ADC scan over host-supplied codes + exact re-rank (round 6)  */
/* ------------------------------------------------------------------------------------------ */
/* Replaces the scoring, selection and re-rank of SqliteVecBackend::Impl::simeonPqSearchUnlocked
 * (src/vector/sqlite_vec_backend.cpp:3868-4056; VectorSearchEngine::SimeonPqAdc is the product's DEFAULT engine,
 * include/yams/vector/vector_types.h:80).  The host keeps what third_party/simeon owns — training the product quantiser,
 * encoding rows (SimeonPqIndexState::codes, :53, :3648-3660) and building the per-query table of inner products
 * (simeon::PQInnerProductQuery, :3901: lut[j][c] = <sub-vector j of the normalised query, centroid c of sub-quantiser j>) —
 * and hands over the codes once (a device mirror, appended like rows) and the tables per batch.  Per query the device
 *   1. scores every indexed row, or every index of `candidates` (:3910-3937, sorted ascending by the host), with
 *      approxScore = sum over j of lut[j][codes[index * m + j]] in fp32 (:3965-3977; the ORDER of the additions is
 *      simeon's: YAMS_PQ_SUM_* below — nothing about simeon is pinned, it is absent from the reference checkout; the
 *      host's own scoring function is probed instead, include/yams_accel/pq_calibration.hpp);
 *   2. keeps the best approxK = min(candidates, max(k, k * rerank_factor)) by (score desc, tie key asc) (:3952-3997);
 *   3. re-scores them with VectorDatabase::computeCosineSimilarity(raw query, row) in fp64, the reference's summation
 *      order (:4023-4034), drops similarity < threshold (:4036-4038);
 *   4. sorts by (similarity desc, chunk_id asc) and cuts to k (:4041-4051).
 * `exact_fallback` indexes (:3882-3893) are the host's call to yams_scan_topk_device.  PQ's own DocumentTopK selection
 * (approxK = the candidate count, then retainBestRecordPerDocument) stays on the host; the exact arm of document-level
 * selection is yams_scan_doc_topk_device. */
typedef struct yams_scan_pq_index_s {
    const uint8_t* codes;       /* device [n_codes][m], 4-byte aligned: code of indexed row i = bytes [i * m, (i + 1) * m)          */
    uint64_t n_codes;           /* indexed rows (SimeonPqIndexState::rowids.size()), < 2^32                                        */
    uint32_t m;                 /* sub-quantisers = bytes per code (simeon_pq_subquantizers, default 32), <= 128; 256 centroids each */
    uint32_t reserved;
    const uint32_t* tie_rank;   /* device [n_codes], nullable: rank of tie_break_keys[i] (= stableStringKey(chunk_id), :3337) among
                                   all indexed rows — ascending key, equal keys by index — the second key of the comparator
                                   :3985-3990.  Null: index order.                                                                 */
    const uint32_t* key_row;    /* device [n_codes], nullable: the corpus row (yams_scan_corpus_t::rows) of the code whose KEY INDEX
                                   is r, where the key index of code i is tie_rank[i] (or i without a tie_rank table): the
                                   rowids[idx] lookup of :4009.  Null: identity.                                                    */
} yams_scan_pq_index_t;

#define YAMS_PQ_SUM_SEQUENTIAL 0u /* one fp32 sum over j = 0 .. m - 1 (a scalar loop)                                             */
#define YAMS_PQ_SUM_X4 1u         /* 4 partial sums (element j -> lane j % 4), lanes added left to right (SSE-shaped)            */
#define YAMS_PQ_SUM_X8 2u         /* 8 partial sums (AVX-shaped)                                                                  */
#define YAMS_PQ_SUM_X16 3u        /* 16 partial sums (AVX-512-shaped)                                                             */
#define YAMS_PQ_SUM_MASK 3u
/* bits 2-3 (4 / 8 / 16 lanes only): how the L partial sums p[0 .. L - 1] become one                                             */
#define YAMS_PQ_SUM_COMBINE_LTR 0u                  /* s = 0; for l: s = s + p[l]                                                   */
#define YAMS_PQ_SUM_COMBINE_HALVES (1u << 2)        /* for (w = L/2; w >= 1; w /= 2) for l < w: p[l] = p[l] + p[l + w]; p[0]
                                                       (extract-high + add, then movehl / shuffle)                                  */
#define YAMS_PQ_SUM_COMBINE_PAIRS (2u << 2)         /* for (w = L; w > 1; w /= 2) for l < w/2: p[l] = p[2l] + p[2l + 1]; p[0] (hadd)  */
#define YAMS_PQ_SUM_COMBINE_HALVES4_PAIRS (3u << 2) /* HALVES while more than 4 lanes remain, then PAIRS on the last 4
                                                       (extract-high, then movehdup + movehl)                                       */
#define YAMS_PQ_SUM_COMBINE_MASK (3u << 2)
/* bit 4 (4 / 8 / 16 lanes only): only elements j < (m / L) * L go through the lanes; the m % L others are added to the COMBINED
 * sum one at a time in element order (a vector loop with a scalar remainder loop).  Without it they go into lanes j % L.        */
#define YAMS_PQ_SUM_TAIL_SCALAR (1u << 4)
#define YAMS_PQ_SUM_ORDER_MASK 0x1Fu
/* 1 + 3 * 4 * 2 = 25 definitions (some coincide: 4 lanes under PAIRS and HALVES4_PAIRS, the tail bit when m % L == 0, ...).
 * With YAMS_PQ_SUM_SEQUENTIAL every bit of 2-4 must be 0 (YAMS_ERR_INVALID_ARG, nothing written); bits above the mask are
 * ignored.  Which one is the host's is not for the host to guess: include/yams_accel/pq_calibration.hpp asks its own
 * scoring function and answers with one of these words, or with "none: refuse the engine". */

typedef struct yams_scan_pq_params_s {
    uint32_t k;
    float similarity_threshold; /* on the EXACT similarity of the re-rank (:4036-4038)                                           */
    uint32_t rerank_factor;     /* SimeonPqIndexState::rerank_factor (>= 1; 0 is read as 1); k * rerank_factor <= 2047            */
    uint32_t flags;             /* YAMS_PQ_SUM_* (lanes | combine | tail)                                                         */
} yams_scan_pq_params_t;

/* corpus: the fp32 rows the re-rank reads (+ tie_rank / rank_row: the chunk_id order of the final sort; row_base / stripes:
 * how a row becomes the id in out_rows).  queries: device [n_queries][dim] RAW queries (the re-rank's first argument);
 * luts: device [n_queries][m][256] fp32, 16-byte aligned; candidates: device, nullable — n_candidates ascending indices
 * into the PQ index (a restriction to documents, :3910-3930; an EMPTY list returns nothing, :3946-3948).
 * out_scores / out_rows: device [n_queries][k]; out_counts: device [n_queries].  A query whose norm^2 is <= 1e-20 or not
 * finite returns nothing (:3895-3898).  Synchronous.  diag (nullable): rows_visited = candidates per query summed,
 * exact_distance_evaluations = rows re-scored, path = 2, filter_tier = 5. */
YAMS_ACCEL_API yams_status_t yams_scan_pq_topk_device(yams_accel_ctx* ctx, const yams_scan_corpus_t* corpus,
                                                      const yams_scan_pq_index_t* pq, const float* queries, const float* luts,
                                                      uint32_t n_queries, const yams_scan_pq_params_t* params,
                                                      const uint32_t* candidates, uint64_t n_candidates, float* out_scores,
                                                      int64_t* out_rows, uint32_t* out_counts, yams_scan_diag_t* diag);

/* ------------------------------------------------------------------------------------------ */
/* Document-level top-k: the k best documents, each shown by its best row                      */
/* ------------------------------------------------------------------------------------------ */
/* CandidateFilterMode::DocumentTopK (include/yams/vector/vector_types.h:205-216): VectorDatabase sends it to
 * IDocumentCandidateVectorStore::searchDocumentCandidatesWithDiagnostics (vector_database.cpp:553-567), whose exact arm
 * is "every matching row of the candidate documents, then retainBestRecordPerDocument"
 * (sqlite_vec_backend.cpp:1508-1518, :86-125).  Here the per-document reduction happens on the device, next to the fp64
 * score that decides it: every allowed row is read once per group of queries, and k documents come back. */
#define YAMS_SCAN_NO_DOC 0xffffffffu
typedef struct yams_scan_docs_s {
    const uint32_t* row_doc;  /* device [n_rows]: document ordinal of each row; YAMS_SCAN_NO_DOC = the row has no
                                 document_hash: scored and counted, never returned (:91-93)                     */
    const uint32_t* doc_rank; /* device [n_docs], nullable: rank of the document's hash in byte-wise (memcmp)
                                 order, the cross-document tie-break; a permutation of 0 .. n_docs - 1;
                                 NULL = ordinal order                                                           */
    uint32_t n_docs, reserved;
} yams_scan_docs_t;

/* Per query: the best row of every document by (similarity desc, tie rank asc) (:96-105), then the best k documents by
 * (similarity desc, doc_rank asc) (:113-121).  The rows are scored exactly as the cosine fast path scores them
 * (:4253-4279: fp64, sequential, rows with norm^2 <= 1e-12 or a non-finite norm or score dropped, similarity < threshold
 * dropped) — bit for bit what yams_scan_topk_device returns for the same row.
 *   out_scores    device [n_queries][k] fp32, best first; unused slots hold -inf
 *   out_rows      device [n_queries][k] int64: row_base + row ordinal of the document's best row; unused -1
 *   out_docs      device [n_queries][k] uint32, nullable: document ordinal; unused YAMS_SCAN_NO_DOC
 *   out_counts    device [n_queries] uint32: documents returned
 *   out_matching  device [n_queries] uint64, nullable: rows >= threshold, before the reduction (the reference's
 *                 returnedRows of this path; diag->returned_rows is their sum)
 * As yams_scan_topk_device: query validation (a non-finite query or norm^2 < 1e-10 fails the whole batch with
 * YAMS_ERR_INVALID_ARG), k == 0 gives an empty result, k <= YAMS_SCAN_MAX_K, row_mask / tie_rank / rank_row / row_base.
 * Cosine only: YAMS_SCAN_L2, YAMS_SCAN_FLAG_RECORD_PATH and every flag but the filter-choice bits give
 * YAMS_ERR_UNSUPPORTED (DocumentTopK carries no metadata filters, :1571-1575), as does a striped shard.  The filter
 * shadows are ignored: every allowed row is scored in fp64, the reference's own cost model for this mode.
 * Diagnostics: used_exact_scan = 1, path = 1, rows_visited = exact_distance_evaluations = allowed rows per query.
 * A row_doc entry >= n_docs (other than YAMS_SCAN_NO_DOC) or a doc_rank that is not a permutation: YAMS_ERR_INVALID_ARG.
 * Any batch size: the per-document keys (16 bytes per query and document) are processed in slices of queries that
 * keep them within 256 MiB.  The call synchronises the context's stream before returning. */
YAMS_ACCEL_API yams_status_t yams_scan_doc_topk_device(
    yams_accel_ctx* ctx, const yams_scan_corpus_t* corpus, const yams_scan_docs_t* docs,
    const float* queries, uint32_t n_queries, const yams_scan_params_t* params,
    float* out_scores, int64_t* out_rows, uint32_t* out_docs, uint32_t* out_counts,
    uint64_t* out_matching /* nullable [n_queries]: rows >= threshold, before the reduction */,
    yams_scan_diag_t* diag);

/* ------------------------------------------------------------------------------------------ */
/* Entity-vector search: IEntityStore::searchEntities over a mirror of entity_vectors           */
/* ------------------------------------------------------------------------------------------ */
/* SqliteVecBackend::Impl::searchEntities (src/vector/sqlite_vec_backend.cpp:2801-2887; seam
 * include/yams/vector/entity_store.h:17-39; types vector_types.h:68, 140-177): the brute-force cosine search over the
 * entity_vectors table (one embedding per symbol / node of the knowledge graph), called once per query by the hybrid
 * search pipeline (src/search/search_vector_pipeline.cpp:439).  The corpus view is the mirror of the rows of
 * entity_vectors whose embedding has `dim` floats, in rowid order; the attribute columns below stand next to it and the
 * `WHERE embedding_type = ? AND node_type = ? AND document_hash = ?` predicate is evaluated on the device, per row and
 * query.  Tombstones and other host-side restrictions use the view's row_mask. */
#define YAMS_SCAN_ENTITY_UNSET 0xffffffffu  /* row_node_type / row_doc: no value; equals no filter value          */
#define YAMS_SCAN_ENTITY_TYPE_UNSET 0xffu   /* row_type: no value; equals no filter value                         */
typedef struct yams_scan_entities_s {
    const uint8_t* row_type;       /* device [n_rows], nullable: EntityEmbeddingType ordinal (vector_types.h:68)     */
    const uint32_t* row_node_type; /* device [n_rows], nullable: id the host interned for the node_type string       */
    const uint32_t* row_doc;       /* device [n_rows], nullable: id the host interned for the document_hash string   */
} yams_scan_entities_t;

#define YAMS_SCAN_ENTITY_FILTER_TYPE 1u      /* AND embedding_type = ? (:2821-2823) */
#define YAMS_SCAN_ENTITY_FILTER_NODE_TYPE 2u /* AND node_type = ?      (:2824-2826) */
#define YAMS_SCAN_ENTITY_FILTER_DOC 4u       /* AND document_hash = ?  (:2827-2829) */
typedef struct yams_scan_entity_filter_s { /* EntitySearchParams' three optional fields, one per query */
    uint32_t fields;         /* YAMS_SCAN_ENTITY_FILTER_* bits: which of the values below take part                 */
    uint32_t embedding_type; /* ids are opaque: a value no row carries (the UNSET values included) matches nothing  */
    uint32_t node_type;
    uint32_t doc;
} yams_scan_entity_filter_t;

/* Per query, the reference's contract (:2809-2884):
 *   rows      those the query's filter and the view's row_mask admit, in row order;
 *   score     float(computeCosineSimilarity(query, row)) (vector_database.cpp:1786-1810): dot, |q|^2, |row|^2 summed in
 *             fp64 element by element, sqrt of each norm, 0.0 if either norm == 0.0 (tested BEFORE the division: a zero
 *             query scores 0.0 against a NaN row, a zero row 0.0 against any query), else dot / (|q| * |row|).  No
 *             finiteness test and no small-norm drop;
 *   kept      iff score >= similarity_threshold (float compare: a NaN score or threshold keeps nothing);
 *   order     score descending, the first min(k, kept).
 * ZERO, NaN AND INFINITE QUERIES ARE SERVED, not refused: searchEntities validates nothing but emptiness (:2809-2811).
 * That is the difference from every other search entry of this header, which drop zero-norm / non-finite rows and
 * fail such queries.
 * The reference sorts with std::sort on the score alone (:2873-2874), which is not stable: the order inside a run of
 * equal scores (-0.0f == +0.0f), and which members of a run that straddles position k come back, the reference leaves
 * open; this is the rule served: (score descending with -0.0 == +0.0, then row ordinal ascending) — what a stable
 * sort of the table order gives, one of the reference's admissible outcomes.  Every returned score carries its own
 * bits (a -0.0f stays -0.0f).
 *   queries       device [n_queries][dim], raw
 *   filters       HOST [n_queries], nullable (= no query has a filter); copied by the call
 *   out_scores    device [n_queries][k] fp32, best first; unused slots hold -inf
 *   out_rows      device [n_queries][k] int64: row_base + row ordinal; unused -1
 *   out_counts    device [n_queries] uint32: rows returned
 *   out_matching  device [n_queries] uint64, nullable: rows kept by the threshold (before the cut to k)
 * k == 0: empty results (counts 0, nothing else written).  dim == 0 (the empty query, :2809-2811) or n_rows == 0: empty
 * results, padded.  k <= YAMS_SCAN_MAX_K.
 * The view's tie_rank / rank_row and filter shadows are IGNORED (the order has no secondary key but the row ordinal; every
 * admitted row is scored in fp64).  With a row_mask, row_mask_count MUST equal the number of set bits (it bounds the list of
 * admitted rows; a smaller value cuts that list at an arbitrary place).  A striped shard: YAMS_ERR_UNSUPPORTED.  An attribute id that no row carries is not
 * an error; a filter that carries an unknown field bit, or names a field whose column is NULL while there are rows to
 * describe, is YAMS_ERR_INVALID_ARG (over an empty table or an empty mask the result is empty whatever the filters name).
 * Diagnostics: used_exact_scan = 1, path = 1, rows_visited = exact_distance_evaluations = rows that passed predicate and
 * mask, returned_rows = rows kept by the threshold, both summed over the queries.
 * Any batch size: the keys (8 bytes per query and admitted row) are processed in slices of queries that keep them within
 * 256 MiB.  The call synchronises the context's stream before returning. */
YAMS_ACCEL_API yams_status_t yams_scan_entity_topk_device(
    yams_accel_ctx* ctx, const yams_scan_corpus_t* corpus, const yams_scan_entities_t* entities,
    const float* queries, const yams_scan_entity_filter_t* filters, uint32_t n_queries, uint32_t k,
    float similarity_threshold, float* out_scores, int64_t* out_rows, uint32_t* out_counts,
    uint64_t* out_matching, yams_scan_diag_t* diag);

/* ------------------------------------------------------------------------------------------ */
/* Spherical k-means of document embeddings: the topology engine "kmeans_v1"                    */
/* ------------------------------------------------------------------------------------------ */
/* KMeansTopologyEngine::buildArtifacts (src/topology/topology_alternate_engines.cpp:648-675) hands every document-level
 * embedding to runKMeans (:341-478), a deterministic spherical k-means; these entries are runKMeans over the usable rows
 * (the shell that filters them is include/yams_accel/topology_kmeans.hpp) and nearestCentroid (:321-336) alone.
 * The contract, restated from :288-478 and topology_build_utils.h:27-56:
 *   cosineDistance (:288-305)  dot, na, nb summed in fp64 element by element; 2.0 if na <= 0 || nb <= 0, else
 *             1 - std::clamp(dot / (sqrt(na) * sqrt(nb)), -1, 1) (std::clamp's comparisons: a NaN passes through).  na and nb
 *             are computed once per row / centroid by the same chain: the same bits.
 *   normalized (:307-319)  norm^2 in fp64; inv = float(1.0 / sqrt(norm)); x *= inv in fp32; a zero vector is left as it is.
 *   meanEmbedding (h:27-56)  an fp32 running sum 0.0f + m0 + m1 + ... over the members in ASCENDING ROW ORDER, /= float(count)
 *             (the IEEE divide), then normalized.
 *   k (:367-371)  0 = round(sqrt(n)); then clamped to [2, n].     max_iterations (:413)  0 = 10.
 *   initialisation (:373-401)  centroid 0 = normalized(row 0); until k centroids exist: over the rows not yet selected,
 *             minDist[u] = min(minDist[u], d(row u, last centroid)), then the first u with the strictly largest minDist is
 *             selected and normalized(row u) appended.  (While k <= n a row is always found: k_eff = k.)
 *   iteration (:414-466)  membership starts at 0; every row moves to its nearest centroid (strict <: the lowest index wins a
 *             tie, a NaN distance never wins, all NaN = 0) and `changed` records a move; every cluster with members gets
 *             normalized(mean of its members), one without keeps its centroid; then the repair below; the loop stops after
 *             the first iteration in which nothing changed.
 *   empty-cluster repair (:433-462)  empty clusters in cluster order: the first row with the strictly largest distance to
 *             its OWN, already updated centroid among the clusters holding more than one member moves over; its row,
 *             normalized, becomes the empty cluster's centroid and the donor's centroid is recomputed from its remaining
 *             members (order kept); later empty clusters see the updated state; `changed` is set.  Duplicate rows make this
 *             path run (a duplicate centroid collects no members).
 * Every finite input is served as the CPU computes it — zero rows, denormal rows (whose normalisation overflows fp32), rows at
 * +-FLT_MAX / 4 (whose fp32 mean overflows) included; a row with a non-finite element is YAMS_ERR_INVALID_ARG (the
 * reference's insert path admits finite values only).  Results equal the CPU loop bit for bit: no chain is split.
 * Limits: 2 <= n < 2^31, dim <= YAMS_CLUSTER_MAX_DIM, k (after the clamp) <= YAMS_CLUSTER_MAX_K: beyond, YAMS_ERR_UNSUPPORTED.
 * n == 0: YAMS_OK, *out_k = *out_iterations = 0, nothing written.  n == 1 (std::clamp(k, 2, 1) is undefined; the reference's
 * shell never gets there) or dim == 0: YAMS_ERR_INVALID_ARG.
 *   rows            device [n][dim] fp32, raw
 *   out_membership  device [n] uint32: the cluster of every row
 *   out_centroids   device [k_eff][dim] fp32, nullable; the caller sizes it for the clamped k (n rows is always enough)
 *   out_k           host, nullable: k_eff          out_iterations  host, nullable: iterations run (the last one included)
 * Work: N*K*D fp64 multiply-adds per iteration and for the initialisation, which is K dependent steps (no host round trip
 * between them); per iteration K + 1 words come back (member counts, changed).  The repair path is driven from the host (it
 * is rare; its distances are computed on the device).  The call synchronises the context's stream before returning. */
#define YAMS_CLUSTER_MAX_DIM 4096u
#define YAMS_CLUSTER_MAX_K 65536u
YAMS_ACCEL_API yams_status_t yams_cluster_kmeans_device(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, uint32_t k, uint32_t max_iterations,
    uint32_t* out_membership, float* out_centroids, uint32_t* out_k, uint32_t* out_iterations);
/* The same over host memory (rows, out_membership, out_centroids are host arrays). */
YAMS_ACCEL_API yams_status_t yams_cluster_kmeans_host(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, uint32_t k, uint32_t max_iterations,
    uint32_t* out_membership, float* out_centroids, uint32_t* out_k, uint32_t* out_iterations);
/* nearestCentroid (:321-336) of every row over GIVEN centroids (incremental routing): out_assign[u] = the lowest index among
 * the centroids at the smallest cosineDistance; a centroid whose centroid_empty flag is non-zero is skipped (:326-328: an
 * empty vector); a NaN distance never wins; a row no centroid wins (all skipped, all NaN, n_centroids == 0) gets 0.
 *   rows            device [n][dim]            centroids  device [n_centroids][dim], raw (no normalisation; non-finite values
 *                                                         are served: they give NaN distances)
 *   centroid_empty  device [n_centroids] uint8, nullable (= none)
 *   out_assign      device [n] uint32          out_distance  device [n] fp64, nullable: the winner's distance (DBL_MAX, the
 *                                                         loop's initial bestDist, when no centroid won)
 * n == 0: YAMS_OK.  dim == 0: YAMS_ERR_INVALID_ARG.  Non-finite ROWS: YAMS_ERR_INVALID_ARG.  The limits above.
 * The call synchronises the context's stream before returning. */
YAMS_ACCEL_API yams_status_t yams_cluster_assign_device(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t n_centroids,
    const uint8_t* centroid_empty, uint32_t* out_assign, double* out_distance);

/* ------------------------------------------------------------------------------------------ */
/* Cluster artifacts: centroids, routing representatives, the boundary spill's residuals      */
/* ------------------------------------------------------------------------------------------ */
/* After clustering every topology engine of the reference runs the same tail over the n x dim matrix
 * (ConnectedComponentTopologyEngine, src/topology/topology_baseline.cpp:202-204,338; Louvain / KMeans through
 * buildBatchFromAssignment, src/topology/topology_alternate_engines.cpp:218-220,263): detail::meanEmbedding
 * (src/topology/topology_build_utils.h:27-56), selectDiverseRoutingRepresentatives and applyOrthogonalBoundarySpill
 * (src/topology/topology_representatives.cpp:33-91, :93-287).  These entries are the array arithmetic of that tail; the shell
 * that keeps the hash maps, the admission tests, the sorts and the member-list edits on the host, and probes which residual
 * form the host's build has, is include/yams_accel/topology_artifacts.hpp.  The contract, restated:
 *   centroid (h:27-56)  per dimension an fp32 running sum 0.0f + m0 + m1 + ... over the members IN THE ORDER OF THE MEMBER LIST
 *             (the reference sorts members by document hash, alternate_engines.cpp:128-130: the order is an input, not the
 *             k-means entry's ascending rows), then /= float(count), the IEEE divide.  No normalisation.  A cluster without
 *             members has no centroid: out_counts = 0 and its row of out_centroids is zeros.
 *   cosineDistance (cpp:13-29)  dot, lhsNorm, rhsNorm: three fp64 chains in element order (the product of two floats is exact
 *             in fp64: fused or not, the same bits); 2.0 if either norm <= 0.0, else
 *             1.0 - std::clamp(dot / (sqrt(l) * sqrt(r)), -1.0, 1.0) (std::clamp's comparisons: a NaN passes through).  A
 *             row's norm is the same chain whoever asks: computed once per row.
 *   selection (cpp:58-90)  candidates in the caller's order (the caller admits and sorts them); extraLimit = min(n_extra,
 *             candidates); for selection s every unused candidate in list order gets d = distance(candidate, s == 0 ? centroid :
 *             last selected) and minDist = std::min(minDist, d) (b < a ? b : a: a NaN d leaves it; minDist starts at DBL_MAX);
 *             the first candidate with minDist > bestDistance STRICTLY wins (bestDistance starts at -1.0) and is used from
 *             then on.  The centroid may be non-finite (an fp32 mean of +-FLT_MAX / 4 rows overflows): served as IEEE gives it.
 *   residuals (cpp:119-141, :189-198, :235-252)  residual = double(e[d]) - double(c[d]); normSq += residual * residual;
 *             residualDot += primaryResidual[d] * residual, with primaryResidual the same subtraction against the primary
 *             centroid.  These products are NOT exact in fp64, so the bits depend on whether the host's compiler contracted
 *             `x += a * b` into an fma (aarch64 with the default -ffp-contract does; x86-64 without -mfma does not):
 *             YAMS_RESIDUAL_SEPARATE = a rounded multiply, then a rounded add; YAMS_RESIDUAL_FUSED = one fma per `+=`.
 *             The shell probes which one the host's build is.
 * Results equal the CPU loop bit for bit: no chain is split, no atomics.
 * Lists are CSR: offsets [lists + 1] uint64 starting at 0 and never decreasing, entries uint32; fewer than 2^32 entries.
 * Limits: n < 2^31, dim <= YAMS_CLUSTER_MAX_DIM, n_clusters <= YAMS_CLUSTER_MAX_K, n_extra <=
 * YAMS_CLUSTER_MAX_REPRESENTATIVES, entries < 2^32: beyond, YAMS_ERR_UNSUPPORTED.  dim == 0, a null array that is needed,
 * offsets that do not start at 0 or decrease, an entry out of range, an unknown form: YAMS_ERR_INVALID_ARG, and nothing is
 * written.  n_clusters == 0 (centroids, representatives) or n == 0 (residuals): YAMS_OK, nothing written.
 * Every call synchronises the context's stream before returning.  The _host twins take host arrays throughout. */
#define YAMS_CLUSTER_MAX_REPRESENTATIVES 64u
#define YAMS_RESIDUAL_SEPARATE 0u
#define YAMS_RESIDUAL_FUSED 1u
#define YAMS_CLUSTER_NONE 0xffffffffu
/* meanEmbedding of every cluster.
 *   rows             device [n][dim] fp32 (any values: served as IEEE gives them)
 *   cluster_offsets  device [n_clusters + 1]        members  device: row indices < n, in the order of the sums
 *   out_centroids    device [n_clusters][dim]       out_counts  device [n_clusters] uint32
 * One chain per (cluster, dimension), one lane each: a wide cluster is parallel along dim, a skewed one is a long tail. */
YAMS_ACCEL_API yams_status_t yams_cluster_centroids_device(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint64_t* cluster_offsets, const uint32_t* members,
    uint32_t n_clusters, float* out_centroids, uint32_t* out_counts);
YAMS_ACCEL_API yams_status_t yams_cluster_centroids_host(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint64_t* cluster_offsets, const uint32_t* members,
    uint32_t n_clusters, float* out_centroids, uint32_t* out_counts);
/* The selection loop of selectDiverseRoutingRepresentatives for every cluster at once.
 *   candidates      device: row indices < n per cluster, in the order the caller gives (admitted, sorted by hash)
 *   centroids       device [n_clusters][dim], raw       centroid_empty  device [n_clusters] uint8, nullable: a cluster whose
 *                                                       flag is set selects nothing (cpp:37)
 *   n_extra         routingRepresentativeCount - 1
 *   out_selected    device [n_clusters][n_extra] uint32: POSITIONS in the cluster's candidate list, in selection order; unused
 *                   slots hold YAMS_CLUSTER_NONE           out_counts  device [n_clusters]: the number selected
 * A row (any row of the matrix) with a non-finite element: YAMS_ERR_INVALID_ARG (the admission test never sends one).
 * Work: the selections are the dependent outer loop; each is one launch over ALL candidates of all clusters plus one
 * reduction per cluster, all enqueued at once (no host round trip between selections). */
YAMS_ACCEL_API yams_status_t yams_cluster_representatives_device(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint64_t* cluster_offsets, const uint32_t* candidates,
    const float* centroids, const uint8_t* centroid_empty, uint32_t n_clusters, uint32_t n_extra, uint32_t* out_selected,
    uint32_t* out_counts);
YAMS_ACCEL_API yams_status_t yams_cluster_representatives_host(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint64_t* cluster_offsets, const uint32_t* candidates,
    const float* centroids, const uint8_t* centroid_empty, uint32_t n_clusters, uint32_t n_extra, uint32_t* out_selected,
    uint32_t* out_counts);
/* The chains of applyOrthogonalBoundarySpill for (document, candidate cluster) pairs.
 *   primary         device [n] uint32, nullable (= none anywhere): every document's primary cluster, YAMS_CLUSTER_NONE = none
 *   cand_offsets, cand   device CSR over the documents: the candidate clusters of every document, in any order, repeats and
 *                   the primary allowed; BOTH NULL = every cluster in index order (pair (u, c) at u * n_clusters + c)
 *   form            YAMS_RESIDUAL_SEPARATE or YAMS_RESIDUAL_FUSED
 *   out_primary_norm_sq  device [n] fp64: primaryNormSquared (0.0 for a document without a primary); needed with primary
 *   out_cand_norm_sq     device [pairs] fp64: candidateNormSquared (the radius pass's radiusSquared is the same chain)
 *   out_residual_dot     device [pairs] fp64: residualDot; needed with primary, undefined for a document without one
 * Every input is served as IEEE gives it (the reference tests isfinite on the results).  The _host twin serves the documents in
 * slices whose outputs occupy at most 256 MiB of device memory. */
YAMS_ACCEL_API yams_status_t yams_cluster_residuals_device(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t n_clusters,
    const uint32_t* primary, const uint64_t* cand_offsets, const uint32_t* cand, uint32_t form, double* out_primary_norm_sq,
    double* out_cand_norm_sq, double* out_residual_dot);
YAMS_ACCEL_API yams_status_t yams_cluster_residuals_host(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t n_clusters,
    const uint32_t* primary, const uint64_t* cand_offsets, const uint32_t* cand, uint32_t form, double* out_primary_norm_sq,
    double* out_cand_norm_sq, double* out_residual_dot);

/* ------------------------------------------------------------------------------------------ */
/* Cluster routing: the dense signal of SparseGuidedClusterRouter::route                        */
/* ------------------------------------------------------------------------------------------ */
/* The one consumer of the cluster artifacts on the query path is SparseGuidedClusterRouter::route
 * (src/topology/topology_baseline.cpp:771-981; its index, buildRouteIndex, :700-769).  Its array arithmetic is the loop
 * :873-920: per candidate cluster the query's cosine to the centroid and to each routing representative, mapped to [0, 1],
 * maximum kept.  These entries are that loop over a RESIDENT table of cluster vectors (the reference caches its index per
 * snapshot; so does the device).  The seed hash maps, the sparse mass, the ANN shortlist, the blend
 * alpha * sparseNorm + (1 - alpha) * dense (a float expression the host's compiler may contract), the scoring modes, the
 * sort and the cut stay on the host.  The contract, restated:
 *   dotProduct (:669-678)  one fp64 chain over i = 0 .. dim-1, acc += double(a[i]) * double(b[i]), then float(acc).  The
 *             products are exact in fp64, so fma equals `+=` bit for bit.
 *   vectorNorm (:680-689)  the same kind of chain over v * v, then float(sqrt(acc)).
 *   per vector  cos = dot_f32 / (qn_f32 * vn_f32) in float: one rounded multiply, one correctly rounded divide;
 *             dense = std::clamp((cos + 1.0F) * 0.5F, 0.0F, 1.0F), clamp being (v < lo) ? lo : (hi < v) ? hi : v: a NaN
 *             stays a NaN.  f32 denormals are kept.
 *   centroid (:879-889)  evaluated only if qn > 0 && cn > 0 (false for a NaN norm); it ASSIGNS dense and sets observed.
 *             Without it dense starts at 0.0F, unobserved.
 *   representatives (:902-919)  positions 0 .. limit-1 of the reference's routingRepresentatives list, limit = the whole list
 *             when maxRoutingRepresentatives == 0, else min(size, max - 1).  The limit counts POSITIONS IN THE REFERENCE'S
 *             LIST, skipped ones included: every row carries its position.  A representative is skipped only if
 *             qn <= 0 || rn <= 0 (or its size differs: such a vector is not in the table at all), so a NaN norm is NOT
 *             skipped: it yields a NaN, which std::max(cur, NaN) = (cur < NaN) ? NaN : cur drops, while observed still
 *             becomes true and the evaluation is still counted.  A NaN the centroid assigned survives every later
 *             representative.  No -0.0f can arise after the map.
 *   per call  every evaluation performed counts once (representativeDistanceEvaluations and
 *             exactRepresentativeDistanceEvaluations both grow by out_evals[q]).  A cluster outside routeCandidates
 *             (:844-871) is not scored: 0.0F, unobserved, not counted.  alpha >= 1 scores nothing: the shell does not call.
 * Every output equals the reference's loop bit for bit (a NaN is some NaN).
 * Limits: 1 <= dim <= YAMS_ROUTE_MAX_DIM, n_clusters <= YAMS_ROUTE_MAX_CLUSTERS, at most YAMS_ROUTE_MAX_REPRESENTATIVES
 * representative rows per cluster, n_queries <= YAMS_ROUTE_MAX_QUERIES per call.  Outside them, or with a null array that is
 * needed, offsets that do not start at 0, decrease or do not end at n_vectors, a centroid flag on an empty segment, or a
 * representative position of 0xffff: YAMS_ERR_INVALID_ARG, and no output is written. */
#define YAMS_ROUTE_MAX_DIM 4096u
#define YAMS_ROUTE_MAX_CLUSTERS 65536u
#define YAMS_ROUTE_MAX_REPRESENTATIVES 64u
#define YAMS_ROUTE_MAX_QUERIES 1024u
typedef struct yams_route_index yams_route_index;
typedef struct yams_route_index_info_t {
    uint64_t n_vectors;
    uint32_t n_clusters;
    uint32_t dim;
    uint64_t bytes;          /* device memory the index holds */
} yams_route_index_info_t;
typedef struct yams_route_diag_t {
    uint64_t pairs;          /* (query, row) pairs the score kernels covered */
    uint32_t slices;         /* launches of the score kernel (a call is served in slices of queries) */
    uint32_t form;           /* the last slice's kernel: 0 = one lane per row (up to 8 queries), 1 = the fp64 tile */
} yams_route_diag_t;
/* Builds the resident index: copies the table to the device and computes every row's norm.
 *   vectors          [n_vectors][dim] fp32, cluster after cluster; inside a cluster the centroid first (when it has one), then
 *                    the representatives the host admits (those of the index dimension), in any order
 *   cluster_offsets  [n_clusters + 1] uint32: the rows of cluster c are [off[c], off[c + 1])
 *   has_centroid     [n_clusters] uint8: nonzero = the first row of the segment is the centroid
 *   position         [n_vectors] uint16: a representative row's place in the reference's list (ignored for a centroid row)
 *   out_norms        [n_vectors] fp32, nullable: float(sqrt(chain)) per row — centroidNorms / routingRepresentativeNorms
 * _device: every array is device memory.  _host: every array is host memory.  The index belongs to `ctx` and is used on its
 * stream; destroy it before the context. */
YAMS_ACCEL_API yams_status_t yams_route_index_create_device(
    yams_accel_ctx* ctx, const float* vectors, uint64_t n_vectors, uint32_t dim, const uint32_t* cluster_offsets,
    const uint8_t* has_centroid, const uint16_t* position, uint32_t n_clusters, yams_route_index** out_index, float* out_norms);
YAMS_ACCEL_API yams_status_t yams_route_index_create_host(
    yams_accel_ctx* ctx, const float* vectors, uint64_t n_vectors, uint32_t dim, const uint32_t* cluster_offsets,
    const uint8_t* has_centroid, const uint16_t* position, uint32_t n_clusters, yams_route_index** out_index, float* out_norms);
YAMS_ACCEL_API void yams_route_index_destroy(yams_route_index* index);
YAMS_ACCEL_API yams_status_t yams_route_index_info(const yams_route_index* index, yams_route_index_info_t* out_info);
/* The dense signal of n_queries queries against the index.
 *   queries       [n_queries][dim] fp32 (any values)
 *   rep_limit     maxRoutingRepresentatives: 0 = every position, else positions < rep_limit - 1
 *   candidates    nullable (= every cluster): bitset [n_queries][ceil(n_clusters / 32)] uint32, bit c % 32 of word c / 32
 *   out_dense     [n_queries][n_clusters] fp32      out_observed  [n_queries][n_clusters] uint8 (0 / 1)
 *   out_evals     [n_queries] uint32: evaluations performed       diag  nullable (host memory in both forms)
 * n_queries == 0: YAMS_OK, nothing written.  _host serves the queries in slices whose outputs occupy at most 256 MiB of device
 * memory.  Synchronises the context's stream before returning. */
YAMS_ACCEL_API yams_status_t yams_route_dense_device(
    yams_route_index* index, const float* queries, uint32_t n_queries, uint32_t rep_limit, const uint32_t* candidates,
    float* out_dense, uint8_t* out_observed, uint32_t* out_evals, yams_route_diag_t* diag);
YAMS_ACCEL_API yams_status_t yams_route_dense_host(
    yams_route_index* index, const float* queries, uint32_t n_queries, uint32_t rep_limit, const uint32_t* candidates,
    float* out_dense, uint8_t* out_observed, uint32_t* out_evals, yams_route_diag_t* diag);

/* ------------------------------------------------------------------------------------------ */
/* Topological quality: H0 persistence of a point cloud (computePersistenceH0)                  */
/* ------------------------------------------------------------------------------------------ */
/* After every rebuild TopologyManager (src/daemon/components/TopologyManager.cpp:660-707) hands the mean embeddings of the
 * clusters with at least two members — what yams_cluster_centroids_device returns — to yams::search::computePersistenceH0
 * (src/search/topological_quality.cpp:75-128): m (m - 1) / 2 pairwise distances, a stable sort, a percentile, Kruskal.  This
 * entry is that function; the shell around it is include/yams_accel/topological_quality.hpp.  deterministicSubsample
 * (:150-167) stays the host's: std::shuffle's sequence belongs to its standard library.  The contract, restated:
 *   points     m rows of `dim` floats: rows[select[0]], rows[select[1]], ... in the order given (repeats allowed: duplicate
 *              points are legal input), or the rows 0 .. n-1 without `select`.  m < 2: value 0.0.  E = m (m - 1) / 2.
 *   distance (:51-61)  for i < j: acc = 0.0; per k in element order d = double(a[k]) - double(b[k]); acc += d * d;
 *              dist = sqrt(acc), correctly rounded.  d carries up to 53 bits, so d * d is NOT exact and the bits of `acc += d * d`
 *              depend on whether the host's compiler contracted it into an fma: YAMS_RESIDUAL_SEPARATE = a rounded multiply,
 *              then a rounded add; YAMS_RESIDUAL_FUSED = one fma.  The shell probes which one the host's build is.
 *              (-d)^2 == d^2 bit for bit: the matrix is symmetric; acc starts at +0.0 and adds non-negatives: never -0.0.
 *   norm (:63-71, :102)  the order statistic of the E distances at idx = size_t(std::clamp(0.95 * double(E - 1), 0.0,
 *              double(E - 1))), computed on the host with exactly that expression.  norm <= 0: value 0.0.
 *   merges (:97-126)  Kruskal over the edges ascending, at most m - 2 merges, total += dist / norm per merge (the divide and
 *              the sum run on the host, in ascending order).  The sorted weights of ANY minimum spanning tree equal
 *              Kruskal's (for every t the number of tree edges <= t is m minus the components of the graph of edges <= t), so
 *              the reference's stable sort does not have to be reproduced; the heaviest tree edge is the one left out.
 *              m == 2: no merge, value 0.0 (norm and the one distance are still reported).
 * Every output equals the reference's computation bit for bit in the form asked for.
 * Limits, decided before anything is allocated: m > YAMS_QUALITY_MAX_POINTS (an m x m fp64 matrix of 2 GiB), dim >
 * YAMS_CLUSTER_MAX_DIM, n >= 2^31: YAMS_ERR_UNSUPPORTED.  dim == 0, a null array that is needed (out; rows when m > 0), an
 * unknown form, a select entry >= n, a non-finite element of a selected row (inf - inf would put NaNs into a sort the
 * reference leaves undefined; judged at every m >= 1): YAMS_ERR_INVALID_ARG.  The m x m matrix comes from the context's
 * workspace (or is out_distances itself in the _device form); when it cannot be had: YAMS_ERR_RESOURCE_EXHAUSTED.  After any
 * status but YAMS_OK nothing has been written to any output.
 *   rows               [n][dim] fp32
 *   select, n_select   nullable: n_select uint32 row indices < n; NULL = all n rows (n_select is ignored).  This is how a caller
 *                      drops the clusters with fewer than two members from a centroid matrix already on the device.
 *   form               YAMS_RESIDUAL_SEPARATE or YAMS_RESIDUAL_FUSED
 *   out                host memory in both forms
 *   out_distances      nullable [m][m] fp64: the matrix, diagonal +0.0
 *   out_merge_weights  nullable [m - 1] fp64: the tree's edge weights ascending (the first m - 2 are the merges)
 *   out_stage_ms       nullable, host memory in both forms: [3] = pair distances, order statistic, spanning tree (device time)
 * _device: rows, select, out_distances, out_merge_weights are device memory.  _host: host memory; only the selected rows
 * travel.  Synchronises the context's stream before returning. */
#define YAMS_QUALITY_MAX_POINTS 16384u
typedef struct yams_persistence_h0_t {
    double value;            /* computePersistenceH0's return value */
    double norm;             /* the 95th-percentile distance (0.0 when m < 2) */
    uint64_t norm_index;     /* its index among the sorted distances */
    uint64_t n_edges;        /* m (m - 1) / 2 */
    uint32_t n_points;       /* m */
    uint32_t n_merges;       /* merges summed into value: m - 2, or 0 when m < 2 or norm <= 0 */
} yams_persistence_h0_t;
YAMS_ACCEL_API yams_status_t yams_quality_persistence_h0_device(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select, uint32_t form,
    yams_persistence_h0_t* out, double* out_distances, double* out_merge_weights, float* out_stage_ms);
YAMS_ACCEL_API yams_status_t yams_quality_persistence_h0_host(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select, uint32_t form,
    yams_persistence_h0_t* out, double* out_distances, double* out_merge_weights, float* out_stage_ms);

/* ------------------------------------------------------------------------------------------ */
/* Topology input features: chunk aggregation, variance weights, the composed feature vector   */
/* ------------------------------------------------------------------------------------------ */
/* Every stage of the topology rebuild starts from the n x dim matrix of per-document feature vectors that
 * TopologyInputExtractor::extract (src/topology/topology_input_extractor.cpp:517-745) composes on one host core.  These entries
 * are its array arithmetic; the shell that keeps the record admissions, the sample cap, the selection of the kept dimensions
 * (the host's own std::partial_sort), the conditions of :353-354 and :169-171, and probes which variance form the host's
 * build has, is include/yams_accel/topology_features.hpp.  The contract, restated:
 *   aggregate (:397-430)  per (document, dimension) ONE fp32 chain in one lane over the document's record list IN THE ORDER
 *             GIVEN: the first record is ASSIGNED (:411: its bits are kept, a lone -0.0f stays -0.0f, a NaN keeps its payload;
 *             the centroid entry starts from 0.0f + and would return +0.0f), every later record is added (:419), and for
 *             count > 1 the sum is divided by float(count), the IEEE divide (:424-428).  count == 0: a row of zeros, count 0.
 *             The short-circuit on a DOCUMENT-level record (:398-402), the skip of empty records (:407) and of records whose
 *             size differs from the first contributing one (:415) are the shell's: the list holds the contributing records.
 *   variance (:123-152)  per dimension: mean = the fp64 chain mean += double(e) over the sample rows in sample order, then
 *             /= double(m); then d = double(e) - mean, var += d * d in the same order, then /= double(m).  d carries up to 53
 *             bits, so d * d is NOT exact and the bits of `var += d * d` depend on whether the host's compiler contracted it
 *             into an fma: YAMS_RESIDUAL_SEPARATE = a rounded multiply, then a rounded add; YAMS_RESIDUAL_FUSED = one fma.
 *             The shell probes which one the host's build is.  A CHAIN IS NEVER SPLIT: the parallelism is across dimensions
 *             only (one lane per dimension), so the call is a LATENCY CHAIN of 2 * m dependent fp64 steps, whatever dim is.
 *             The selection of the top targetDim variances (:156-163) stays on the host: the order of equal variances at the
 *             cut is std::partial_sort's.
 *   compose (:344-388)  per row, in the reference's order:
 *             matryoshka view (:172-186), when `weights` is given: kept = the indices with weights[i] > 0.0f, ascending (a
 *             NaN weight is not kept; the count need not equal any target); coarse[j] = dense[kept[j]] * weights[kept[j]], an
 *             fp32 multiply; then the normalisation.  Without `weights` the normalisation applies to dense itself.
 *             normalisation (:98-110): sumSq = one fp64 chain of double(x) * double(x) in element order (exact products:
 *             form-free); sumSq <= 0.0 leaves the vector as it is (a NaN sumSq does not take that branch); otherwise
 *             norm = float(sqrt(sumSq)) and every element is x / norm in fp32.  A norm that rounds to 0.0f or to inf is
 *             served as IEEE gives it (inf or NaN elements; zeros).
 *             sketch (:192-203): count[sig[i] % sketch_dim] per bucket, taken as float(count) — the reference's `+= 1.0F`
 *             chain while sig_len < 2^24; the limit is YAMS_FEATURES_MAX_SIG_LEN — then normalised the same way.  (The
 *             counts are integers summing to sig_len, so every partial sum of their squares is an integer <= 2^32: the chain
 *             is exact in any order.)
 *             concatenation (:362-387): entityOn = entity && K && entity_on[i]; minhashOn = sig && sig_len && sketch_on[i] &&
 *             sketch_dim > 0.  Both off: the row is the dense part alone, with NO multiply.  Otherwise aE = entityOn ?
 *             alpha_e : 0.0f, aM likewise, aD = std::max(0.0f, (1.0f - aE) - aM) in fp32 = (0.0f < t) ? t : 0.0f (a NaN gives
 *             0.0f), and the row is dense * aD, then entity * aE if on, then sketch * aM if on.  f32 denormals are kept.
 * Results equal the CPU loop bit for bit in the form asked for (a NaN is the reference's NaN where no arithmetic touches it,
 * some NaN otherwise).  Every input value is served as IEEE gives it (NaN, inf, +-0.0).
 * Lists are CSR: offsets [lists + 1] uint64 starting at 0 and never decreasing, entries uint32.
 * Limits: dim, K, sketch_dim <= YAMS_FEATURES_MAX_DIM, sig_len <= YAMS_FEATURES_MAX_SIG_LEN, n (n_records, n_docs) < 2^31,
 * entries < 2^32: beyond, YAMS_ERR_UNSUPPORTED.  dim == 0, a null array that is needed, offsets that do not start at 0 or
 * decrease, an index out of range, an unknown form, out_stride smaller than the longest possible row, an output overlapping an
 * input: YAMS_ERR_INVALID_ARG, found before anything is written.  Every call synchronises the context's stream before
 * returning.  The _host twins take host arrays throughout. */
#define YAMS_FEATURES_MAX_DIM 4096u
#define YAMS_FEATURES_MAX_SIG_LEN 65536u
/* aggregateEmbedding of every document at once.
 *   rows         [n_records][dim] fp32: the chunk embeddings (any values)
 *   doc_offsets  [n_docs + 1] uint64       records  uint32 row indices < n_records, per document in the order of the sums
 *   out          [n_docs][dim] fp32        out_counts  [n_docs] uint32: the contributing records
 * n_docs == 0: YAMS_OK, nothing written.  One chain per (document, dimension), one lane each. */
YAMS_ACCEL_API yams_status_t yams_features_aggregate_device(
    yams_accel_ctx* ctx, const float* rows, uint64_t n_records, uint32_t dim, const uint64_t* doc_offsets, const uint32_t* records,
    uint64_t n_docs, float* out, uint32_t* out_counts);
YAMS_ACCEL_API yams_status_t yams_features_aggregate_host(
    yams_accel_ctx* ctx, const float* rows, uint64_t n_records, uint32_t dim, const uint64_t* doc_offsets, const uint32_t* records,
    uint64_t n_docs, float* out, uint32_t* out_counts);
/* The two passes of computeVarianceWeights.
 *   rows              [n][dim] fp32
 *   select, n_select  nullable: m = n_select sample rows (indices < n) in the order of the sums, repeats allowed; NULL = the
 *                     rows 0 .. n-1 (m = n, n_select ignored)
 *   form              YAMS_RESIDUAL_SEPARATE or YAMS_RESIDUAL_FUSED
 *   out_mean, out_var [dim] fp64 each
 * m == 0: YAMS_OK, nothing written (the reference returns before it divides, :134-136).  The _host twin sends only the sample
 * rows. */
YAMS_ACCEL_API yams_status_t yams_features_variance_device(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select, uint32_t form,
    double* out_mean, double* out_var);
YAMS_ACCEL_API yams_status_t yams_features_variance_host(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select, uint32_t form,
    double* out_mean, double* out_var);
/* composeFeatureVector of every row at once.
 *   dense       [n][dim] fp32: the dense view
 *   weights     [dim] fp32, HOST memory in both twins, nullable: the matryoshka weights of the shell's host-side selection;
 *               NULL = matryoshka off
 *   entity      [n][K] fp32, nullable: entity signatures, already normalised by the host, taken as given
 *   entity_on   [n] uint8: the per-row switch of the entity part (needed when entity && K)
 *   sig         [n][sig_len] uint32, nullable: MinHash signatures
 *   sketch_on   [n] uint8: the per-row switch of the sketch part (needed when sig && sig_len && sketch_dim)
 *   out         [n][out_stride] fp32; out_dims [n] uint32: the row's length; everything behind it in the row is zero-filled.
 *               The longest possible row is kept (or dim) + (entity && K ? K : 0) + (sig && sig_len && sketch_dim ?
 *               sketch_dim : 0).
 * n == 0: YAMS_OK, nothing written.  Each row's sumSq is one chain in one lane; the scale-and-store pass is parallel across
 * elements. */
YAMS_ACCEL_API yams_status_t yams_features_compose_device(
    yams_accel_ctx* ctx, const float* dense, uint64_t n, uint32_t dim, const float* weights, const float* entity, uint32_t k,
    const uint8_t* entity_on, const uint32_t* sig, uint32_t sig_len, const uint8_t* sketch_on, uint32_t sketch_dim, float alpha_e,
    float alpha_m, float* out, uint32_t out_stride, uint32_t* out_dims);
YAMS_ACCEL_API yams_status_t yams_features_compose_host(
    yams_accel_ctx* ctx, const float* dense, uint64_t n, uint32_t dim, const float* weights, const float* entity, uint32_t k,
    const uint8_t* entity_on, const uint32_t* sig, uint32_t sig_len, const uint8_t* sketch_on, uint32_t sketch_dim, float alpha_e,
    float alpha_m, float* out, uint32_t out_stride, uint32_t* out_dims);

/* ------------------------------------------------------------------------------------------ */
/* Late-interaction rerank: ColBERT MaxSim over a window of documents, and token pooling        */
/* ------------------------------------------------------------------------------------------ */
/* Behind every reranked search the reference scores each candidate document against the query token by token:
 * OnnxColbertSession::Impl::computeMaxSim (plugins/onnx/onnx_colbert_session.cpp:247-259, dot at :286-293), once per document
 * from score_documents (plugins/onnx/model_provider.cpp:1883-1888), on one host core.  The same class turns a token matrix into
 * one embedding: maxPoolEmbeddings (:214-230) and normalizeEmbedding (:232-245).  These entries are those loops; the shell that
 * flattens the vectors of vectors, takes dim = min of the two sides, sends ragged embedding sets back to the host and probes
 * which form the host's build has is include/yams_accel/colbert_rerank.hpp.  The contract, restated:
 *   maxsim   sim(q, d) = ONE fp32 chain from +0.0f over i = 0 .. dim-1 in order: YAMS_RESIDUAL_SEPARATE = sum + (a[i] * b[i]),
 *            a rounded multiply then a rounded add; YAMS_RESIDUAL_FUSED = fmaf(a[i], b[i], sum).  Which one a host's
 *            `sum += a[i] * b[i]` is, is a property of its build.
 *            maxSim starts at -inf and is replaced only if sim > maxSim: a NaN sim never wins, a row of NaNs or an empty
 *            document leaves -inf, and among equal values (zeros of both signs are equal) the first in document order stays.
 *            score starts at +0.0f; score = score + maxSim in query-token order, ONE chain per document, never split.  An empty
 *            query gives +0.0f.  Infinities flow as the chain carries them (+inf then -inf: NaN).  Subnormals are kept.
 *   maxpool  per (document, dimension): pooled = -inf, replaced only when pooled < token[i] (std::max: a NaN never enters); a
 *            non-finite result becomes 0.0f; an empty document gives zeros.  Then norm = sqrt of ONE fp64 chain of
 *            double(v) * double(v) in element order (exact products: form-free); norm > 1e-8: v = float(double(v) / norm),
 *            otherwise a row of zeros.
 * Results equal the CPU loop bit for bit in the form asked for; a NaN score is some NaN (x86 and the device give the default
 * NaN different signs).  Documents are CSR over one row pool: doc_offsets [n_docs + 1] uint64 from 0, never decreasing.
 * Limits: dim <= YAMS_RERANK_MAX_DIM, tq <= YAMS_RERANK_MAX_QUERY_TOKENS, n_docs <= YAMS_RERANK_MAX_DOCS, n_docs * tq <=
 * YAMS_RERANK_MAX_ROWMAX, a document <= YAMS_RERANK_MAX_DOC_TOKENS rows, the pool <= YAMS_RERANK_MAX_ROWS rows: beyond,
 * YAMS_ERR_UNSUPPORTED.  dim == 0, a null array that is needed, offsets that do not start at 0 or decrease, an unknown form, an
 * output overlapping an input: YAMS_ERR_INVALID_ARG.  Order, in both twins: the limits that need no array, then the nulls and the
 * form, then the OFFSETS (their defects, a document too long), and only then what the offsets' total sizes — the row limit, null
 * rows, the overlaps: a call with two defects reports the earlier one.  Every refusal is found before anything is written.  Every
 * call synchronises the context's stream before returning.  The _host twins take host arrays throughout. */
#define YAMS_RERANK_MAX_DIM 1024u
#define YAMS_RERANK_MAX_DOC_TOKENS (1u << 20)
#define YAMS_RERANK_MAX_QUERY_TOKENS (1u << 16)
#define YAMS_RERANK_MAX_ROWS (1ull << 28)
#define YAMS_RERANK_MAX_DOCS (1ull << 20)
#define YAMS_RERANK_MAX_ROWMAX (1ull << 27)
#define YAMS_RERANK_PATH_VALU 0u /* register tiles of chains on the vector ALU */
#define YAMS_RERANK_PATH_MFMA 1u /* v_mfma_f32_32x32x2_f32: the fused form only */
#define YAMS_RERANK_NONE 0xffffffffu /* out_rowarg: no token won, the row maximum is the initial -inf */
typedef struct yams_rerank_diag {
    uint32_t path;         /* YAMS_RERANK_PATH_* that served the chains */
    uint32_t form;         /* the form asked for */
    uint64_t rows;         /* document token rows seen (the last offset) */
    uint64_t docs;         /* documents seen */
    uint32_t query_tokens; /* query tokens seen */
    uint32_t reserved;
} yams_rerank_diag_t;
/* computeMaxSim(query, document) of every document of the window at once.
 *   query        [tq][dim] fp32       rows  [doc_offsets[n_docs]][dim] fp32: the documents' token rows
 *   out_scores   [n_docs] fp32
 *   out_rowmax   nullable, [n_docs][tq] fp32: maxSim of every (document, query token)
 *   out_rowarg   nullable, [n_docs][tq] uint32, written only along with out_rowmax: the token (index inside its document) whose
 *                sim stayed, YAMS_RERANK_NONE where none did
 *   diag         nullable, written on YAMS_OK
 * n_docs == 0: YAMS_OK, nothing written. */
YAMS_ACCEL_API yams_status_t yams_rerank_maxsim_device(
    yams_accel_ctx* ctx, const float* query, uint32_t tq, uint32_t dim, const float* rows, const uint64_t* doc_offsets,
    uint64_t n_docs, uint32_t form, float* out_scores, float* out_rowmax, uint32_t* out_rowarg, yams_rerank_diag_t* diag);
YAMS_ACCEL_API yams_status_t yams_rerank_maxsim_host(
    yams_accel_ctx* ctx, const float* query, uint32_t tq, uint32_t dim, const float* rows, const uint64_t* doc_offsets,
    uint64_t n_docs, uint32_t form, float* out_scores, float* out_rowmax, uint32_t* out_rowarg, yams_rerank_diag_t* diag);
/* normalizeEmbedding(maxPoolEmbeddings(document, dim)) of every document at once.  out [n_docs][dim] fp32.
 * n_docs == 0: YAMS_OK, nothing written. */
YAMS_ACCEL_API yams_status_t yams_rerank_maxpool_device(
    yams_accel_ctx* ctx, const float* rows, uint32_t dim, const uint64_t* doc_offsets, uint64_t n_docs, float* out);
YAMS_ACCEL_API yams_status_t yams_rerank_maxpool_host(
    yams_accel_ctx* ctx, const float* rows, uint32_t dim, const uint64_t* doc_offsets, uint64_t n_docs, float* out);

/* ------------------------------------------------------------------------------------------ */
/* The embedding model's pooling head: CLS, max or mean over the tokens of each text            */
/* ------------------------------------------------------------------------------------------ */
/* Every embedding the reference produces passes through the pooling head of its ONNX plugin: OnnxModelSession takes the
 * encoder's output [B, S, D] (fp32 hidden states) and the attention masks and, on one host core, pools the tokens of each text
 * and L2-normalises the result (plugins/onnx/onnx_model_pool.cpp:1808-1854 the batch path; :1729-1774 and :1448-1491 the same
 * loops; :1935-1953, :1501-1515 and :1888-1900 the rank-2 output, which is normalised only).  These entries are those loops;
 * the shell that flattens the masks and keeps the host's own loop for what is refused is include/yams_accel/embedding_pool.hpp.
 * The contract, restated.  Per text b, with T = min(seq, mask_len) tokens considered:
 *   start      emb[dim] starts at +0.0f.
 *   CLS        emb[d] = hidden[b][0][d], whatever the mask says (the mask is never read; the diag's counts are 0).
 *   MAX        for each token i < T with mask[b][i] > 0, in token order: emb[d] = (emb[d] < x) ? x : emb[d] (std::max: a NaN
 *              never enters; the floor is the initial +0.0f).  Any positive mask value is active.
 *   MEAN       total = 0.0f; for each i < T with w = float(mask[b][i]) > 0: total += w; emb[d] += x * w — ONE fp32 chain per
 *              (b, d) in token order, never split or reassociated; then, if total > 0, emb[d] = emb[d] / total, a correctly
 *              rounded fp32 division.  Served for masks of 0 and 1 (what the reference's generateAttentionMask produces): the
 *              product is then exact and the fused and the separate host build agree.  A considered value above 1 is refused.
 *   normalise  (YAMS_EMBED_NORMALIZE) norm = sqrt of ONE fp64 chain of double(v) * double(v) in element order (exact products:
 *              form-free); norm > 1e-8: v = float(double(v) / norm), otherwise a row of zeros — a NaN norm fails the comparison.
 * A masked row is never read: a NaN or an infinity there does not reach the output.  Subnormals are kept.  Results equal the CPU
 * loop bit for bit; a NaN is some NaN.
 * Limits: dim <= YAMS_EMBED_MAX_DIM, seq <= YAMS_EMBED_MAX_SEQ, batch * seq <= YAMS_EMBED_MAX_ROWS (normalise: batch <=
 * YAMS_EMBED_MAX_ROWS), MEAN with a considered mask value above 1: beyond, YAMS_ERR_UNSUPPORTED.  dim == 0, seq == 0, a null
 * array that is needed, an unknown mode or flag bit, an output overlapping an input: YAMS_ERR_INVALID_ARG.  Every refusal is
 * found before anything is written.  Every call synchronises the context's stream before returning.  The _host twins take host
 * arrays throughout. */
#define YAMS_EMBED_MAX_DIM 8192u
#define YAMS_EMBED_MAX_SEQ (1u << 16)
#define YAMS_EMBED_MAX_ROWS (1ull << 22)
#define YAMS_EMBED_POOL_CLS 0u
#define YAMS_EMBED_POOL_MAX 1u
#define YAMS_EMBED_POOL_MEAN 2u
#define YAMS_EMBED_NORMALIZE 1u /* flags: L2-normalise the pooled rows */
typedef struct yams_embed_diag {
    uint32_t mode;              /* the mode asked for */
    uint32_t flags;             /* the flags asked for */
    uint64_t batch;             /* texts seen */
    uint32_t seq;               /* tokens per text */
    uint32_t dim;
    uint64_t tokens_considered; /* batch * min(seq, mask_len); 0 for CLS or without a mask */
    uint64_t active_tokens;     /* considered mask values above 0; 0 for CLS */
    uint32_t slab_dims;         /* dimensions one workgroup owned: chosen from batch and dim so that small batches cover the device */
    uint32_t reserved;
} yams_embed_diag_t;
/* The pooled (and, when asked, normalised) row of every text.
 *   hidden   [batch][seq][dim] fp32
 *   mask     [batch][mask_len] int32; nullable for CLS or when mask_len == 0 (MAX and MEAN then give zeros)
 *   out      [batch][dim] fp32
 *   diag     nullable, written on YAMS_OK
 * batch == 0: YAMS_OK, nothing written. */
YAMS_ACCEL_API yams_status_t yams_embed_pool_device(
    yams_accel_ctx* ctx, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask, uint32_t mask_len,
    uint32_t mode, uint32_t flags, float* out, yams_embed_diag_t* diag);
YAMS_ACCEL_API yams_status_t yams_embed_pool_host(
    yams_accel_ctx* ctx, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask, uint32_t mask_len,
    uint32_t mode, uint32_t flags, float* out, yams_embed_diag_t* diag);
/* The rank-2 output: out[b][:] = rows[b][:] L2-normalised.  rows, out [batch][dim] fp32.  batch == 0: YAMS_OK, nothing written. */
YAMS_ACCEL_API yams_status_t yams_embed_normalize_device(yams_accel_ctx* ctx, const float* rows, uint64_t batch, uint32_t dim, float* out);
YAMS_ACCEL_API yams_status_t yams_embed_normalize_host(yams_accel_ctx* ctx, const float* rows, uint64_t batch, uint32_t dim, float* out);

/* ------------------------------------------------------------------------------------------ */
/* The semantic-neighbour graph: exact top-K self-join of the document-level embeddings         */
/* ------------------------------------------------------------------------------------------ */
/* EmbeddingService::updateSemanticNeighborGraphUnlocked (src/daemon/components/EmbeddingService.cpp) scores, for every
 * source document, every other document-level embedding and writes the best semanticTopK (default 8, :385) as
 * `semantic_neighbor` edges: N^2 * D scalar fp64 multiply-adds on one core (:612-648 the streaming branch, :856-1076 the
 * whole-corpus branch).  This entry is that loop; the shell around it is include/yams_accel/semantic_graph.hpp.
 * The contract, restated from EmbeddingService.cpp:
 *   inverse norm (:405-415)  norm = an fp64 chain of x * x in element order; inv = norm <= 0 ? 0.0f : float(1.0 / sqrt(norm)).
 *             A row with inv <= 0 is not part of the corpus (:876-878, :527): never a candidate, no neighbours as a source.
 *   similarity (:417-431)  dot = an fp64 chain of double(a[i]) * double(b[i]) in element order;
 *             sim = float((dot * double(inv_source)) * double(inv_neighbour)), in that operand order.
 *   admission (:626-632, :991-997)  adaptive mode (no explicit threshold): sim <= 0.0f is dropped, both zeros go; explicit
 *             mode: sim < threshold is dropped (at threshold 0.0f both -0.0f and +0.0f stay).
 *   self (:619, :985)  the source never lists itself: the row index differs.  Another row with identical bits is listed.
 *   order (:464-470, :949-954)  similarity descending by the float compare (the two zeros are ONE score; the returned score
 *             keeps its sign bit), then document hash ascending: tie_rank[row] = the rank of the row's hash, a permutation
 *             of [0, n); without one, row order.
 *   result  the min-replacement loop (:637-646, :1001-1010) keeps exactly the best K under that strict total order; they are
 *             returned sorted (:760, :1017).  The effective threshold (:761-762, :1018-1019) is the explicit one or the
 *             last kept similarity: every kept row passes it, so the result is the sorted list of at most K rows.
 *   diagnostics  pairs_scored = similarityPairCount, pairs_admitted = candidateNeighborCount (summed over the sources).
 * What the reference leaves undefined is refused with YAMS_ERR_INVALID_ARG and nothing written: a non-finite element (NaN
 * similarities in a comparator that does not order them; inserts are validated finite, src/vector/vector_database.cpp:
 * 1771-1784) and a row whose float inverse norm is +inf (every element a denormal: 0 * inf).  A finite, denormal inverse
 * norm (a row of +-FLT_MAX / 4: inv = 4.2e-39) is served.  Results equal the CPU loop bit for bit: no chain is split.
 * Limits: n < 2^31, dim <= YAMS_GRAPH_MAX_DIM, k <= YAMS_GRAPH_MAX_K: beyond, YAMS_ERR_UNSUPPORTED.  k == 0, n < 2 or
 * n_sources == 0: YAMS_OK, an empty result (the early return at :890; nothing written, *out_diag zeroed).  dim == 0, null
 * rows or null outputs: YAMS_ERR_INVALID_ARG.
 *   rows          device [n][dim] fp32, raw (any float alignment)
 *   tie_rank      device [n] uint32, nullable.  Not a permutation of [0, n): YAMS_ERR_INVALID_ARG (found on the device).
 *   source_rows   device [n_sources] uint32, nullable = every row in row order (n_sources is then taken as n); indices may
 *                 repeat and come in any order; an index >= n: YAMS_ERR_INVALID_ARG (found on the device).
 *   flags         YAMS_GRAPH_FLAG_EXPLICIT_THRESHOLD: `threshold` is the explicit one (any finite value; the adapter
 *                 clamps to [0, 1] as :398 does); otherwise adaptive mode and `threshold` is ignored.  A non-finite
 *                 threshold in explicit mode, or an unknown flag: YAMS_ERR_INVALID_ARG.
 *   out_rows      device [n_sources][k] uint32, best first; unused slots 0xffffffff
 *   out_sims      device [n_sources][k] fp32; unused slots -inf
 *   out_counts    device [n_sources] uint32
 *   out_inv_norm  device [n] fp32, nullable: the inverse norms (what the host caches in SemanticCorpusEntry)
 *   out_diag      host, nullable
 * Work: n_sources * n * dim fp64 multiply-adds in tiles of 128 sources x 64 candidates; when the source tiles alone would
 * leave CUs idle the candidates are dealt to `stripes` workgroups per source tile and a merge kernel joins their lists.
 * No n^2-sized buffer: the workspace is O(n) + n_sources * stripes * k keys.  One 4-byte read-back (the refusal flags)
 * sits between the inverse-norm pass and the pairs.  The call synchronises the context's stream before returning. */
#define YAMS_GRAPH_MAX_DIM 4096u
#define YAMS_GRAPH_MAX_K 64u
#define YAMS_GRAPH_FLAG_EXPLICIT_THRESHOLD 1u
typedef struct yams_graph_diag {
    uint32_t stripes;        /* candidate stripes per source tile (1 = no merge needed) */
    uint32_t source_tiles;   /* tiles of 128 sources */
    uint64_t pairs_scored;   /* similarityPairCount */
    uint64_t pairs_admitted; /* candidateNeighborCount */
} yams_graph_diag_t;
YAMS_ACCEL_API yams_status_t yams_graph_semantic_neighbors_device(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint32_t* tie_rank,
    const uint32_t* source_rows, uint64_t n_sources, uint32_t k, uint32_t flags, float threshold,
    uint32_t* out_rows, float* out_sims, uint32_t* out_counts, float* out_inv_norm, yams_graph_diag_t* out_diag);
/* The same over host memory: rows, tie_rank, source_rows and the four output arrays are host arrays. */
YAMS_ACCEL_API yams_status_t yams_graph_semantic_neighbors_host(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint32_t* tie_rank,
    const uint32_t* source_rows, uint64_t n_sources, uint32_t k, uint32_t flags, float threshold,
    uint32_t* out_rows, float* out_sims, uint32_t* out_counts, float* out_inv_norm, yams_graph_diag_t* out_diag);

/* ------------------------------------------------------------------------------------------ */
/* SGC smoothing of the document embeddings over the neighbour graph                          */
/* ------------------------------------------------------------------------------------------ */
/* applySGCSmoothing (src/topology/topology_sgc.cpp:23-179 of the reference, header include/yams/topology/topology_sgc.h,
 * Lean contract formal/topology/Yams/Topology/SGC.lean) runs between the semantic-neighbour graph and the clustering:
 * `hops` rounds of X <- D^-1/2 (A + I) D^-1/2 X over every document embedding ("54k docs x 1024 dim", :127-129).  This
 * entry is its degree pass and its hop loop (:114-161); the shell in front of them (early returns :25-50, admission
 * :60-84, symmetrisation :86-112, the feature matrix :130-137, the write-back :163-168) is
 * include/yams_accel/topology_sgc.hpp.
 * THE ORDER OF A ROW'S LIST IS AN INPUT.  The reference accumulates each output element in fp32, one neighbour at a time,
 * in the order in which its symmetrised lists were filled — the iteration order of a std::unordered_map (:106-111), a
 * property of the host's standard library.  Another order gives other bits, so the host builds the lists and this entry
 * keeps their order: every output element is ONE chain in one lane; no atomics, no split chains, no reduction over edges.
 * The contract, restated from topology_sgc.cpp, over the list (row_offsets, cols, weights):
 *   degree (:114-125)  deg[i] = 1.0 + the fp64 chain of double(w) over row i's edges in list order;
 *             inv[i] = deg > 0 ? 1.0 / sqrt(deg) : 0.0 — a correctly rounded square root, then a correctly rounded divide
 *             (not a reciprocal square root).
 *   one hop (:140-161)  for every row i and dimension d: acc = float((inv[i] * inv[i]) * double(x[i][d])); then for each edge
 *             (to, w) of row i in list order: scale = (double(w) * inv[i]) * inv[to]; an edge with scale == 0.0 is SKIPPED,
 *             not added (adding +0.0f would turn a -0.0f accumulator into +0.0f); otherwise
 *             acc = acc +f32 float(scale * double(x[to][d])): an fp64 product, a cast that rounds to nearest even, an fp32 add
 *             with denormals kept.  Hop h + 1 reads the output of hop h.
 * The list need not be symmetric; self-loops and repeated columns are computed as the formula says.  An fp32 overflow inside
 * the hops is served as IEEE gives it (inf, and NaN from inf - inf): only non-finite INPUT is refused.
 * Refused with YAMS_ERR_INVALID_ARG, found on the device before anything is written: row_offsets[0] != 0, an offset that
 * decreases, a column >= n, a weight that is negative or not finite, a non-finite element of rows.
 * n == 0: YAMS_OK, nothing written.  hops == 0: out = rows, bit for bit (nothing else is looked at).  dim == 0, null rows,
 * out or row_offsets, out overlapping rows: YAMS_ERR_INVALID_ARG.  n >= 2^31, nnz (= row_offsets[n]) >= 2^32,
 * dim > YAMS_SGC_MAX_DIM: YAMS_ERR_UNSUPPORTED.
 *   rows         device [n][dim] fp32 (any float alignment; 16-byte aligned bases and dim % 4 == 0 get vector loads)
 *   row_offsets  device [n + 1] uint64;  cols device [nnz] uint32;  weights device [nnz] fp32 — the order IS the sum order
 *   out          device [n][dim] fp32; must not overlap rows
 *   out_diag     host, nullable
 * Work: a lane owns four consecutive dimensions of one row and walks the row's edges in order with the loads of four edges
 * in flight; a row of YAMS_SGC_HUB_DEGREE edges or more is dealt one dimension per lane instead, so four times as many waves
 * share its walk.  Workspace: n doubles, nnz doubles (the scales, computed once per edge), n uint32, and for hops >= 2 one
 * n x dim fp32 buffer; the result lands in `out` whatever the parity of hops.  One 32-byte read-back (the refusal flags, nnz)
 * sits between the checks and the hops.  The call synchronises the context's stream before returning. */
#define YAMS_SGC_MAX_DIM 4096u
#define YAMS_SGC_HUB_DEGREE 512u
typedef struct yams_sgc_diag {
    uint64_t nnz;                      /* row_offsets[n] */
    uint64_t edges_skipped_zero_scale; /* edges whose scale is 0.0 (each is skipped in every hop) */
    uint32_t max_degree;               /* the longest list */
    uint32_t hops;
    uint32_t hub_rows;                 /* rows of YAMS_SGC_HUB_DEGREE edges or more */
    uint32_t reserved;
} yams_sgc_diag_t;
YAMS_ACCEL_API yams_status_t yams_graph_sgc_smooth_device(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint64_t* row_offsets,
    const uint32_t* cols, const float* weights, uint32_t hops, float* out, yams_sgc_diag_t* out_diag);
/* The same over host memory: rows, row_offsets, cols, weights and out are host arrays. */
YAMS_ACCEL_API yams_status_t yams_graph_sgc_smooth_host(
    yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint64_t* row_offsets,
    const uint32_t* cols, const float* weights, uint32_t hops, float* out, yams_sgc_diag_t* out_diag);

/* ------------------------------------------------------------------------------------------ */
/* SHA-256                                                                                   */
/* ------------------------------------------------------------------------------------------ */
/* Digest n_msgs byte ranges of one device buffer: message i = data[offsets[i] .. +lengths[i]).
 * offsets/lengths are DEVICE arrays; digests is device [n_msgs][32] (raw bytes, big-endian words
 * as FIPS 180-4 prints them).  Asynchronous on the context's stream. */
YAMS_ACCEL_API yams_status_t yams_sha256_batch_device(yams_accel_ctx* ctx, const uint8_t* data,
                                                      const uint64_t* offsets,
                                                      const uint64_t* lengths, uint64_t n_msgs,
                                                      uint8_t* digests);
/* Batched integrity check (ChunkValidator::validateChunks / validateManifest,
 * src/integrity/chunk_validator.cpp:36-120,160-212,230-262): re-hash n_chunks byte ranges of one
 * device buffer and compare with the expected raw 32-byte digests (device, any alignment).
 * out_valid[i] = 1 iff SHA-256(data[offsets[i] .. +lengths[i])) == expected_digests[i];
 * *out_n_invalid = number of mismatches.  Synchronises the context's stream. */
YAMS_ACCEL_API yams_status_t yams_verify_chunks_device(yams_accel_ctx* ctx, const uint8_t* data,
                                                       const uint64_t* offsets,
                                                       const uint64_t* lengths, uint64_t n_chunks,
                                                       const uint8_t* expected_digests,
                                                       uint8_t* out_valid, uint64_t* out_n_invalid);
/* One-shot over host memory: SHA256Hasher::hash(span), sha256_hasher.cpp:167-195.
 * out_hex receives 64 lower-case hex characters + NUL (bytesToHex, :19-30). */
YAMS_ACCEL_API yams_status_t yams_sha256_host(yams_accel_ctx* ctx, const uint8_t* data_host,
                                              size_t n, char out_hex[65]);
/* Many host buffers at once (one message per lane on the device). */
YAMS_ACCEL_API yams_status_t yams_sha256_many_host(yams_accel_ctx* ctx,
                                                   const uint8_t* const* msgs_host,
                                                   const size_t* lens, size_t n_msgs,
                                                   char* out_hex /* [n_msgs][65] */);

/* ------------------------------------------------------------------------------------------ */
/* Content-defined chunking                                                                     */
/* ------------------------------------------------------------------------------------------ */
typedef enum yams_cdc_mode_e {
    YAMS_CDC_RABIN = 0,     /* RabinChunker: first tested byte is start+min, sizes in [min+1,max] */
    YAMS_CDC_STREAMING = 1  /* StreamingChunker (product default): first tested byte is
                               start+min-1, sizes in [min,max]                                   */
} yams_cdc_mode_t;

/* ChunkingConfig, include/yams/chunking/chunker.h:44-51 (target size does not enter the
 * boundary logic and is omitted).  polynomial == 0 selects the default (rabin_chunker.cpp:29-37). */
typedef struct yams_cdc_config_s {
    uint64_t window_size; /* 1..48 (RabinWindow is a 48-byte ring, chunker.h:151-155)            */
    uint64_t min_size;
    uint64_t max_size;
    uint64_t polynomial;
    uint64_t mask;
    uint32_t mode;        /* yams_cdc_mode_t */
    uint32_t flags;       /* YAMS_CDC_FLAG_*; 0 = defaults */
} yams_cdc_config_t;
/* Boundary detection has two kernel forms with identical results: a narrow one for window 48 and
 * masks below 2^31 (the product defaults) and a generic one (any window 1..48, any 64-bit mask).
 * This flag selects the generic form even where the narrow one applies (parity tests use it). */
#define YAMS_CDC_FLAG_GENERIC_KERNEL 1u

YAMS_ACCEL_API void yams_cdc_default_config(yams_cdc_config_t* cfg, uint32_t mode);

/* Result of chunking (and optionally hashing) a set of blobs; device arrays owned by the
 * context's workspace, valid until the next ingest/cdc call on the same context. */
typedef struct yams_ingest_result_s {
    uint64_t n_chunks;            /* total over all blobs                                        */
    const uint64_t* chunk_offset; /* device [n_chunks]: offset within its blob                   */
    const uint64_t* chunk_size;   /* device [n_chunks]                                           */
    const uint32_t* chunk_blob;   /* device [n_chunks]: blob index                               */
    const uint64_t* blob_first;   /* device [n_blobs + 1]: first chunk of each blob (prefix)     */
    const uint8_t* chunk_digest;  /* device [n_chunks][32] or NULL                               */
    const uint8_t* blob_digest;   /* device [n_blobs][32] or NULL                                */
} yams_ingest_result_t;

/* Chunk boundaries only.  data: device bytes; blob_offsets/blob_lengths: HOST arrays locating
 * each blob inside `data`. */
YAMS_ACCEL_API yams_status_t yams_cdc_chunk_device(yams_accel_ctx* ctx, const uint8_t* data,
                                                   const uint64_t* blob_offsets_host,
                                                   const uint64_t* blob_lengths_host,
                                                   uint64_t n_blobs, const yams_cdc_config_t* cfg,
                                                   yams_ingest_result_t* out);
/* The ingest hot path: chunk boundaries + per-chunk SHA-256 + whole-blob SHA-256
 * (content_store_impl.cpp:199-231).  flags: bit0 = chunk digests, bit1 = blob digests. */
#define YAMS_INGEST_CHUNK_DIGESTS 1u
#define YAMS_INGEST_BLOB_DIGESTS 2u
/* With YAMS_INGEST_BLOB_DIGESTS: do NOT compute the whole-blob digest of blobs whose chain would outlast the rest
 * of the call.  One SHA-256 chain is sequential — ~35 MB/s on a device lane, > 1 GB/s on a host core with SHA
 * extensions — so ONE 64 MiB blob in a batch holds the call for 1.9 s while everything else finishes in tens of
 * milliseconds.  A blob is deferred iff its length exceeds the threshold below (a pure function of the call's total
 * bytes: the caller evaluates the same predicate, starts its own hasher — ContentStore::store's SHA256Hasher,
 * content_store_impl.cpp:199-231 — on those blobs BEFORE the call and joins after it); the digest entry of a
 * deferred blob is 32 zero bytes.  Chunk boundaries and per-chunk digests of deferred blobs are computed as usual.
 * Thresholds: chain time L / 35 MB/s against the rest of the call at its measured rate — device-resident input
 * ~340 GB/s (ratio 2^12, rounded towards keeping work on the device), host-streamed input ~25 GB/s (ratio 2^9);
 * never below the lone-chain limit of content_hash_v1 (1 MiB). */
#define YAMS_INGEST_DEFER_LONG_BLOB_DIGESTS 4u
static inline uint64_t yams_ingest_defer_threshold_device(uint64_t total_bytes) {
    const uint64_t t = total_bytes >> 12;
    return t > (1ull << 20) ? t : (1ull << 20);
}
static inline uint64_t yams_ingest_defer_threshold_host(uint64_t total_bytes) {
    const uint64_t t = total_bytes >> 9;
    return t > (1ull << 20) ? t : (1ull << 20);
}
YAMS_ACCEL_API yams_status_t yams_ingest_device(yams_accel_ctx* ctx, const uint8_t* data,
                                                const uint64_t* blob_offsets_host,
                                                const uint64_t* blob_lengths_host,
                                                uint64_t n_blobs, const yams_cdc_config_t* cfg,
                                                uint32_t flags, yams_ingest_result_t* out);

/* The same path for blobs in HOST memory (what ContentStore::store has after reading a file,
 * content_store_impl.cpp:199-231): blobs cross PCIe in batches of ~batch_bytes (0 = chosen from the call: about
 * 2048 of its longest blob, 1 to 8 GiB, at least four batches — the digest chains of a batch take (longest blob) /
 * 35 MB/s and three batches' chains are in flight; a blob is never split; and never more than a tenth of the device
 * memory that is free when the call starts, so that four slot buffers + tables take at most half of it) through two to
 * four device buffers, batch i + 1 uploading while batch i is chunked and hashed.  Device footprint: during the call up
 * to 4 x batch_bytes + ~25 % of tables; AFTER the call the context keeps no buffer above 1.25 GiB (larger ones are
 * freed on return: they belong to the call, not to the context).
 * How a call is cut into batches (part of the contract: tests/_ingest_model.py restates it and holds the "batches" and
 * "slots" of device_info's "last_host_ingest" to it): batches hold consecutive blobs in call order; a blob is never split;
 * inside its batch every blob starts on a 16-byte boundary, so a blob counts with its length rounded up to a multiple of 16
 * (an empty blob counts 0); a batch always takes at least one blob, however long; a batch closes in front of the first
 * blob whose rounded length would take its sum past batch_bytes.  Without YAMS_INGEST_BLOB_DIGESTS two slot buffers serve
 * the batches in turn, with it four; never more buffers than there are batches.
 * Pinned (page-locked) blob memory uploads at link speed, pageable memory through the runtime's
 * staging.  Results go to caller arrays: out_blob_first[n_blobs + 1] (prefix of chunk counts),
 * out_chunk_offset / out_chunk_size [chunk_cap], out_chunk_digest [chunk_cap][32] (nullable),
 * out_blob_digest [n_blobs][32] (required with YAMS_INGEST_BLOB_DIGESTS).  If the chunks do not fit
 * chunk_cap the status is YAMS_ERR_INVALID_ARG and *out_n_chunks holds the required size (blob digests
 * and out_blob_first are complete even then). */
YAMS_ACCEL_API yams_status_t yams_ingest_host(yams_accel_ctx* ctx, const uint8_t* const* blobs_host,
                                              const uint64_t* blob_lengths, uint64_t n_blobs,
                                              const yams_cdc_config_t* cfg, uint32_t flags,
                                              uint64_t batch_bytes, uint64_t* out_blob_first,
                                              uint64_t* out_chunk_offset, uint64_t* out_chunk_size,
                                              uint8_t* out_chunk_digest, uint64_t chunk_cap,
                                              uint8_t* out_blob_digest, uint64_t* out_n_chunks);

/* IChunker::chunkDataLazy over host memory (chunker.h:84-86): fills caller arrays; hex may be
 * NULL.  Returns the chunk count in *out_count (cap = capacity of the arrays; if the count
 * exceeds cap the status is YAMS_ERR_INVALID_ARG and *out_count holds the required size). */
YAMS_ACCEL_API yams_status_t yams_cdc_chunk_host(yams_accel_ctx* ctx, const uint8_t* data_host,
                                                 size_t n, const yams_cdc_config_t* cfg,
                                                 uint64_t* offsets, uint64_t* sizes,
                                                 char* hex /* [cap][65] */, size_t cap,
                                                 size_t* out_count);

/* One WINDOW of a stream (StreamingChunker::processStream / processFileStream, streaming_chunker.h:54-121: the
 * bounded-memory callback form).  The first context_len bytes of `data_host` are history only — they feed the
 * rolling hash (its state is a function of the last 56 bytes: 8 inside the 64-bit shift, 48..55 through the byte
 * that leaves the ring; >= 64 bytes of true history reproduce it exactly), the first chunk starts at offset
 * context_len; offsets are relative to data_host.  The LAST chunk returned ends at the end of the buffer whether or
 * not a boundary falls there: a caller that has more data carries that chunk (and 64 bytes in front of it) into the
 * next window.  Streaming mode only (RabinChunker restarts its hash at every chunk): YAMS_ERR_INVALID_ARG otherwise.
 * context_len = 0 is yams_cdc_chunk_host. */
YAMS_ACCEL_API yams_status_t yams_cdc_chunk_window_host(yams_accel_ctx* ctx, const uint8_t* data_host,
                                                        size_t n, size_t context_len, const yams_cdc_config_t* cfg,
                                                        uint64_t* offsets, uint64_t* sizes,
                                                        char* hex /* [cap][65] */, size_t cap,
                                                        size_t* out_count);

/* ------------------------------------------------------------------------------------------------
 * Chunk dedup lookup: a device-resident set of SHA-256 digests.
 *
 * Replaces the per-chunk `storage_->exists(chunk.hash)` round trips of ContentStore::store
 * (src/api/content_store_impl.cpp:246-287).  The reference walks the chunk list in order: a chunk
 * is stored iff its hash is neither in the store nor carried by an EARLIER chunk of the same walk;
 * yams_dedup_insert_* answers exactly that per chunk (is_new[i]; first occurrence = lowest index)
 * and adds the new digests to the set, so one call per ingest batch replaces n exists() calls.
 * Digests are raw 32-byte values (the `chunk_digest` array of yams_ingest_result_t), 8-byte
 * aligned.  The set grows by rehashing; calls synchronise the context's stream.
 * ---------------------------------------------------------------------------------------------- */
typedef struct yams_dedup_set yams_dedup_set;
YAMS_ACCEL_API yams_status_t yams_dedup_set_create(yams_accel_ctx* ctx, uint64_t expected_entries,
                                                   yams_dedup_set** out_set);
YAMS_ACCEL_API void yams_dedup_set_destroy(yams_dedup_set* set);
YAMS_ACCEL_API yams_status_t yams_dedup_set_size(const yams_dedup_set* set, uint64_t* out_entries);
/* chunk_sizes (device, nullable): when given, out_bytes_new / out_bytes_deduped receive the
 * bytesStored / bytesDeduped sums of content_store_impl.cpp:255,274. */
YAMS_ACCEL_API yams_status_t yams_dedup_insert_device(yams_dedup_set* set, const uint8_t* digests,
                                                      uint64_t n, const uint64_t* chunk_sizes,
                                                      uint8_t* out_is_new, uint64_t* out_n_new,
                                                      uint64_t* out_bytes_new,
                                                      uint64_t* out_bytes_deduped);
YAMS_ACCEL_API yams_status_t yams_dedup_probe_device(yams_dedup_set* set, const uint8_t* digests,
                                                     uint64_t n, uint8_t* out_exists);
YAMS_ACCEL_API yams_status_t yams_dedup_insert_host(yams_dedup_set* set, const uint8_t* digests_host,
                                                    uint64_t n, uint8_t* out_is_new_host,
                                                    uint64_t* out_n_new);
YAMS_ACCEL_API yams_status_t yams_dedup_probe_host(yams_dedup_set* set, const uint8_t* digests_host,
                                                   uint64_t n, uint8_t* out_exists_host);

/* ------------------------------------------------------------------------------------------------
 * Batched CRC-32: CompressedStorageEngine's header.uncompressedCRC32
 * (src/storage/compressed_storage_engine.cpp:49-59, 524) and the read side's check of it (:594-627,
 * src/storage/storage_engine.cpp:102-120, src/compression/compression_utils.cpp:31-52,
 * src/compression/integrity_validator.cpp:36-65).  The standard CRC-32: reflected polynomial 0xEDB88320,
 * initial value ~0, final xor ~0, check value 0xCBF43926; the CRC of an empty message is 0.
 *
 * CRC is linear over GF(2), so a message is cut into segments of YAMS_CRC32_SEGMENT_BYTES that are computed
 * independently and folded: one long message spreads over the device like many short ones.  Messages start at any
 * byte offset and have any length up to 2^40; only the 16-byte-aligned granules that hold message bytes are read.
 * Every call returns with its results complete (it reads one word back to size its workspace of
 * O(total bytes / segment + n) bytes).  n == 0: YAMS_OK, nothing written; NULL ctx or tables: YAMS_ERR_INVALID_ARG;
 * 2^31 messages or more: YAMS_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------------- */
#define YAMS_CRC32_SEGMENT_BYTES 4096u
/* Pure, needs no device: the CRC-32 of A || B from crc(A), crc(B) and |B| (updateCRC32,
 * compression_utils.cpp:42-52, by linearity). */
YAMS_ACCEL_API uint32_t yams_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* Message i = data[offsets[i] .. offsets[i] + lengths[i]); offsets / lengths: DEVICE arrays; out_crc32: DEVICE u32[n_msgs],
 * in input order.  Messages may overlap. */
YAMS_ACCEL_API yams_status_t yams_crc32_batch_device(yams_accel_ctx* ctx, const uint8_t* data,
                                                     const uint64_t* offsets, const uint64_t* lengths,
                                                     uint64_t n_msgs, uint32_t* out_crc32);
/* The chunks of an ingest result (chunk_blob / chunk_offset / chunk_size of yams_ingest_device or yams_cdc_chunk_device
 * over the same `data` and blob_offsets_host) while the bytes are still resident.  select: device u8[n_chunks] or NULL —
 * e.g. out_is_new of yams_dedup_insert_device: only new chunks are stored; an unselected chunk's bytes are not read and
 * its entry is 0.  out_crc32: DEVICE u32[n_chunks].  The result's arrays are only read. */
YAMS_ACCEL_API yams_status_t yams_crc32_chunks_device(yams_accel_ctx* ctx, const uint8_t* data,
                                                      const uint64_t* blob_offsets_host, uint64_t n_blobs,
                                                      const yams_ingest_result_t* chunks, const uint8_t* select,
                                                      uint32_t* out_crc32);
/* The read side (storage_engine.cpp:102-120, compressed_storage_engine.cpp:594-627): out_valid[i] =
 * (crc(message i) == expected_crc32[i]); expected_crc32 / out_valid: DEVICE arrays; *out_n_invalid (host, nullable)
 * counts the mismatches. */
YAMS_ACCEL_API yams_status_t yams_crc32_verify_device(yams_accel_ctx* ctx, const uint8_t* data,
                                                      const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                                                      const uint32_t* expected_crc32, uint8_t* out_valid,
                                                      uint64_t* out_n_invalid);
/* Messages in HOST memory: one upload, one batch, one download.  A NULL message needs length 0. */
YAMS_ACCEL_API yams_status_t yams_crc32_many_host(yams_accel_ctx* ctx, const uint8_t* const* msgs_host,
                                                  const size_t* lens, size_t n_msgs, uint32_t* out_crc32_host);
/* yams_ingest_host plus the CRC-32 of every chunk: out_chunk_crc32 [chunk_cap] (required unless chunk_cap is 0), filled
 * like out_chunk_offset.  The same implementation with one more pass and one more copy per batch, on the one upload;
 * every other output is what yams_ingest_host gives for the same arguments. */
YAMS_ACCEL_API yams_status_t yams_ingest_host_crc32(yams_accel_ctx* ctx, const uint8_t* const* blobs_host,
                                                    const uint64_t* blob_lengths, uint64_t n_blobs,
                                                    const yams_cdc_config_t* cfg, uint32_t flags,
                                                    uint64_t batch_bytes, uint64_t* out_blob_first,
                                                    uint64_t* out_chunk_offset, uint64_t* out_chunk_size,
                                                    uint8_t* out_chunk_digest, uint64_t chunk_cap,
                                                    uint8_t* out_blob_digest, uint64_t* out_n_chunks,
                                                    uint32_t* out_chunk_crc32);

/* ------------------------------------------------------------------------------------------ */
/* Plugin vtables (obtained through yams_plugin_get_interface)                                  */
/* ------------------------------------------------------------------------------------------ */
#define YAMS_IFACE_VECTOR_SCAN_V1 "vector_scan_v1"
#define YAMS_IFACE_VECTOR_SCAN_V1_VERSION 2u /* 2 appends pq_index_set / search_pq; a host that asks for version 1 gets the same table */
#define YAMS_IFACE_CONTENT_HASH_V1 "content_hash_v1"
#define YAMS_IFACE_CONTENT_HASH_V1_VERSION 1u
#define YAMS_IFACE_CHUNKER_V1 "chunker_v1"
#define YAMS_IFACE_CHUNKER_V1_VERSION 3u /* 2: chunk_many / free_chunk_batch appended; 3: chunk_window appended (hosts
                                           that asked for an older version see the same leading fields) */

/* The YAMS plugin entry points (include/yams/plugins/abi.h:18-34 in the reference; the declarations
 * are identical, so this header and the reference's can be included together). */
#ifndef YAMS_PLUGIN_ABI_VERSION
#define YAMS_PLUGIN_ABI_VERSION 1
#define YAMS_PLUGIN_OK 0
#define YAMS_PLUGIN_ERR_INCOMPATIBLE -1
#define YAMS_PLUGIN_ERR_NOT_FOUND -2
#define YAMS_PLUGIN_ERR_INIT_FAILED -3
#define YAMS_PLUGIN_ERR_INVALID -4
#endif
YAMS_ACCEL_API int yams_plugin_get_abi_version(void);
YAMS_ACCEL_API const char* yams_plugin_get_name(void);
YAMS_ACCEL_API const char* yams_plugin_get_version(void);
YAMS_ACCEL_API const char* yams_plugin_get_manifest_json(void);
/* config_json: {"device": n} | {"devices": [..]} (a corpus is dealt to all of them in stripes and
 * searched behind one call), "search_slots": n (concurrent searches, default 2),
 * "shadows": "both" | "bf16" | "i8" | "none". */
YAMS_ACCEL_API int yams_plugin_init(const char* config_json, const void* host_context);
YAMS_ACCEL_API void yams_plugin_shutdown(void);
YAMS_ACCEL_API int yams_plugin_get_interface(const char* iface_id, uint32_t version, void** out_iface);
YAMS_ACCEL_API int yams_plugin_get_health_json(char** out_json);

typedef struct yams_scan_hit_s {
    int64_t row;      /* row ordinal in the mirror (host maps it to its VectorRecord)            */
    float similarity; /* relevance_score */
    float distance;   /* L2 distance for YAMS_SCAN_L2, else 1 - similarity
                         (utils::similarityToDistance, vector_database.cpp:1867-1875)           */
} yams_scan_hit_t;

typedef struct yams_vector_scan_v1 {
    uint32_t abi_version; /* YAMS_IFACE_VECTOR_SCAN_V1_VERSION */
    void* self;
    /* Device mirror lifecycle.  `rows` is host memory [n_rows][dim]; tie_ranks nullable. */
    yams_status_t (*corpus_create)(void* self, uint32_t dim, uint64_t* out_corpus_id);
    yams_status_t (*corpus_append)(void* self, uint64_t corpus_id, const float* rows,
                                   uint64_t n_rows);
    yams_status_t (*corpus_set_tie_ranks)(void* self, uint64_t corpus_id,
                                          const uint32_t* tie_ranks, uint64_t n_rows);
    yams_status_t (*corpus_clear)(void* self, uint64_t corpus_id);
    yams_status_t (*corpus_destroy)(void* self, uint64_t corpus_id);
    yams_status_t (*corpus_size)(void* self, uint64_t corpus_id, uint64_t* out_rows,
                                 uint32_t* out_dim);
    /* Batched search: one contiguous row-major result buffer [n_queries][k] (padded; counts say
     * how many entries of each row are valid), released with free_hits. */
    yams_status_t (*search_batch)(void* self, uint64_t corpus_id, const float* queries,
                                  uint32_t n_queries, uint32_t dim, uint32_t k,
                                  float similarity_threshold, uint32_t metric,
                                  yams_scan_hit_t** out_hits, uint32_t** out_counts,
                                  yams_scan_diag_t* out_diag /* nullable */);
    void (*free_hits)(void* self, yams_scan_hit_t* hits, uint32_t* counts);
    yams_status_t (*get_runtime_info_json)(void* self, char** out_json);
    void (*free_string)(void* self, char* s);
    /* Filtered search (document_hash / candidate_hashes, vector_store.h:44-49): `row_mask` is a
     * HOST bitmap over the mirror's rows (bit r & 31 of word r >> 5), NULL = all rows. */
    yams_status_t (*search_batch_masked)(void* self, uint64_t corpus_id, const float* queries,
                                         uint32_t n_queries, uint32_t dim, uint32_t k,
                                         float similarity_threshold, uint32_t metric,
                                         const uint32_t* row_mask, yams_scan_hit_t** out_hits,
                                         uint32_t** out_counts, yams_scan_diag_t* out_diag);
    /* Same, with YAMS_SCAN_FLAG_* bits (e.g. YAMS_SCAN_FLAG_RECORD_PATH for searches that carry
     * metadata_filters, whose predicate the host has already folded into `row_mask`). */
    yams_status_t (*search_batch_ex)(void* self, uint64_t corpus_id, const float* queries,
                                     uint32_t n_queries, uint32_t dim, uint32_t k,
                                     float similarity_threshold, uint32_t metric, uint32_t flags,
                                     const uint32_t* row_mask, yams_scan_hit_t** out_hits,
                                     uint32_t** out_counts, yams_scan_diag_t* out_diag);
    /* ---- version 2: the product-quantised engine (VectorSearchEngine::SimeonPqAdc; simeonPqSearchUnlocked,
     * src/vector/sqlite_vec_backend.cpp:3868-4056) over the same mirror; see yams_scan_pq_topk_device.
     * pq_index_set: the host's SimeonPqIndexState (:48-62) for this corpus, all HOST arrays: codes [n_codes][m],
     * tie_keys [n_codes] (tie_break_keys = stableStringKey(chunk_id)), row_of_index [n_codes] (nullable = identity: which
     * mirror row code i belongs to — rowids[i] mapped to the mirror's ordinal).  Replaces a previous index; n_codes == 0
     * drops it.  corpus_append does NOT touch it (a PQ index that names rows the mirror has lost skips them, :4010-4012).
     * corpus_clear RELEASES it with the other per-row tables (documents, entity attributes): its row_of_index names rows
     * that are gone, and rows appended afterwards are different rows — search_pq on a cleared corpus returns nothing until
     * pq_index_set is called again.  Corpora dealt to several devices: YAMS_ERR_UNSUPPORTED. */
    yams_status_t (*pq_index_set)(void* self, uint64_t corpus_id, const uint8_t* codes, uint64_t n_codes, uint32_t m,
                                  const uint64_t* tie_keys, const uint32_t* row_of_index);
    /* queries: host [n_queries][dim] RAW queries; luts: host [n_queries][m][256] (what simeon::PQInnerProductQuery holds for
     * the NORMALISED query, :3895-3901); candidates (nullable): n_candidates ascending indices into the PQ index (:3910-3937);
     * flags: YAMS_PQ_SUM_*.  Hits as search_batch (distance = 1 - similarity); the final order uses the corpus's tie ranks
     * (corpus_set_tie_ranks: chunk_id order, :4041-4051). */
    yams_status_t (*search_pq)(void* self, uint64_t corpus_id, const float* queries, const float* luts, uint32_t n_queries,
                               uint32_t dim, uint32_t k, float similarity_threshold, uint32_t rerank_factor, uint32_t flags,
                               const uint32_t* candidates, uint64_t n_candidates, yams_scan_hit_t** out_hits,
                               uint32_t** out_counts, yams_scan_diag_t* out_diag);
} yams_vector_scan_v1;

/* Document-level selection over a vector_scan_v1 corpus (yams_scan_doc_topk_device).  A separate interface, version 1,
 * so that vector_scan_v1 keeps its version: it is served by yams_plugin_get_interface but NOT listed in the manifest
 * (the reference's loader does not consult the manifest in getInterface, abi_plugin_loader.cpp:657-681; adding it there
 * is a separate change).  The corpus ids are vector_scan_v1's. */
#define YAMS_IFACE_VECTOR_DOC_SCAN_V1 "vector_doc_scan_v1"
#define YAMS_IFACE_VECTOR_DOC_SCAN_V1_VERSION 1u
typedef struct yams_vector_doc_scan_v1 {
    uint32_t abi_version; /* YAMS_IFACE_VECTOR_DOC_SCAN_V1_VERSION */
    void* self;
    /* The row -> document map of a corpus (host arrays): row_doc [n_rows] (n_rows == the corpus's rows;
     * YAMS_SCAN_NO_DOC = no document), doc_rank [n_docs] nullable (see yams_scan_docs_t).  Replaces the previous map;
     * rows appended later are YAMS_SCAN_NO_DOC until it is called again; corpus_clear drops it. */
    yams_status_t (*corpus_set_documents)(void* self, uint64_t corpus_id, const uint32_t* row_doc, uint64_t n_rows,
                                          const uint32_t* doc_rank, uint32_t n_docs);
    /* k documents per query, row_mask (host, nullable) as search_batch_masked: hits [n_queries][k] with
     * distance = 1 - similarity, counts [n_queries], out_matching (host [n_queries], nullable) = rows >= threshold
     * before the reduction.  Release with free_doc_hits.  A corpus dealt to several devices: YAMS_ERR_UNSUPPORTED. */
    yams_status_t (*search_docs)(void* self, uint64_t corpus_id, const float* queries, uint32_t n_queries, uint32_t dim,
                                 uint32_t k, float similarity_threshold, const uint32_t* row_mask, yams_scan_hit_t** out_hits,
                                 uint32_t** out_counts, uint64_t* out_matching, yams_scan_diag_t* out_diag);
    void (*free_doc_hits)(void* self, yams_scan_hit_t* hits, uint32_t* counts);
} yams_vector_doc_scan_v1;

/* IEntityStore::searchEntities over a vector_scan_v1 corpus (yams_scan_entity_topk_device): an entity table is its own
 * corpus id, one per embedding dimension.  A separate interface, version 1, served by yams_plugin_get_interface and NOT
 * listed in the manifest, for the reason given at vector_doc_scan_v1.  Host memory in, host memory out. */
#define YAMS_IFACE_VECTOR_ENTITY_SCAN_V1 "vector_entity_scan_v1"
#define YAMS_IFACE_VECTOR_ENTITY_SCAN_V1_VERSION 1u
typedef struct yams_vector_entity_scan_v1 {
    uint32_t abi_version; /* YAMS_IFACE_VECTOR_ENTITY_SCAN_V1_VERSION */
    void* self;
    /* The attribute columns of rows [first_row, first_row + n_rows) of the corpus (host arrays, each nullable = leave that
     * column of the range as it is): EntityEmbeddingType ordinals, interned node_type ids, interned document_hash ids.
     * Rows never set carry YAMS_SCAN_ENTITY_TYPE_UNSET / YAMS_SCAN_ENTITY_UNSET, which no filter matches; corpus_clear
     * drops the columns.  A corpus dealt to several devices: YAMS_ERR_UNSUPPORTED. */
    yams_status_t (*corpus_set_attributes)(void* self, uint64_t corpus_id, uint64_t first_row, uint64_t n_rows,
                                           const uint8_t* types, const uint32_t* node_types, const uint32_t* docs);
    /* searchEntities for n_queries queries: filters [n_queries] nullable, row_mask (host, nullable) as
     * search_batch_masked (the adapter's tombstones).  hits [n_queries][k] with distance = 1 - similarity, counts
     * [n_queries], out_matching (host [n_queries], nullable) = rows kept by the threshold.  Release with free_entity_hits. */
    yams_status_t (*search_entities)(void* self, uint64_t corpus_id, const float* queries,
                                     const yams_scan_entity_filter_t* filters, uint32_t n_queries, uint32_t dim, uint32_t k,
                                     float similarity_threshold, const uint32_t* row_mask, yams_scan_hit_t** out_hits,
                                     uint32_t** out_counts, uint64_t* out_matching, yams_scan_diag_t* out_diag);
    void (*free_entity_hits)(void* self, yams_scan_hit_t* hits, uint32_t* counts);
} yams_vector_entity_scan_v1;

/* The topology build's k-means (yams_cluster_kmeans_device / yams_cluster_assign_device) for a host that holds the
 * embeddings in its own memory.  A separate interface, version 1, served by yams_plugin_get_interface and NOT listed in
 * the manifest, for the reason given at vector_doc_scan_v1.  Host memory in, host memory out. */
#define YAMS_IFACE_TOPOLOGY_CLUSTER_V1 "topology_cluster_v1"
#define YAMS_IFACE_TOPOLOGY_CLUSTER_V1_VERSION 1u
typedef struct yams_topology_cluster_v1 {
    uint32_t abi_version; /* YAMS_IFACE_TOPOLOGY_CLUSTER_V1_VERSION */
    void* self;
    /* runKMeans over rows [n][dim] (every row usable): *out_membership [n] and *out_centroids [*out_k][dim] are allocated
     * by the plugin (release with free_clusters); out_centroids, out_k, out_iterations are nullable.  Statuses and limits
     * of yams_cluster_kmeans_device; n == 0 gives null arrays. */
    yams_status_t (*kmeans)(void* self, const float* rows, uint64_t n, uint32_t dim, uint32_t k, uint32_t max_iterations,
                            uint32_t** out_membership, float** out_centroids, uint32_t* out_k, uint32_t* out_iterations);
    /* nearestCentroid of rows [n][dim] over centroids [n_centroids][dim]; centroid_empty [n_centroids] nullable;
     * *out_assign [n] and *out_distance [n] (nullable: not wanted) are allocated by the plugin (free_assignment). */
    yams_status_t (*assign)(void* self, const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t n_centroids,
                            const uint8_t* centroid_empty, uint32_t** out_assign, double** out_distance);
    void (*free_clusters)(void* self, uint32_t* membership, float* centroids);
    void (*free_assignment)(void* self, uint32_t* assign, double* distance);
} yams_topology_cluster_v1;

/* The semantic-neighbour graph (yams_graph_semantic_neighbors_host) for a host that holds the document-level embeddings
 * in its own memory.  A separate interface, version 1, served by yams_plugin_get_interface and NOT listed in the
 * manifest, for the reason given at vector_doc_scan_v1.  Host memory in, host memory out. */
#define YAMS_IFACE_SEMANTIC_GRAPH_V1 "semantic_graph_v1"
#define YAMS_IFACE_SEMANTIC_GRAPH_V1_VERSION 1u
typedef struct yams_semantic_graph_v1 {
    uint32_t abi_version; /* YAMS_IFACE_SEMANTIC_GRAPH_V1_VERSION */
    void* self;
    /* The best k neighbours of every source over rows [n][dim]; tie_rank [n] and source_rows [n_sources] nullable as in
     * yams_graph_semantic_neighbors_device.  *out_rows [S][k], *out_sims [S][k], *out_counts [S] (S = the number of
     * sources) and *out_inv_norm [n] (nullable: not wanted) are allocated by the plugin (release with free_neighbors);
     * out_diag nullable.  Statuses and limits of the flat entry; an empty result (k == 0, n < 2, no sources) gives null
     * arrays. */
    yams_status_t (*neighbors)(void* self, const float* rows, uint64_t n, uint32_t dim, const uint32_t* tie_rank,
                               const uint32_t* source_rows, uint64_t n_sources, uint32_t k, uint32_t flags, float threshold,
                               uint32_t** out_rows, float** out_sims, uint32_t** out_counts, float** out_inv_norm,
                               yams_graph_diag_t* out_diag);
    void (*free_neighbors)(void* self, uint32_t* rows, float* sims, uint32_t* counts, float* inv_norm);
} yams_semantic_graph_v1;

/* SGC smoothing (yams_graph_sgc_smooth_host) for a host that holds the document embeddings and the neighbour lists in
 * its own memory.  A separate interface, version 1, served by yams_plugin_get_interface and NOT listed in the manifest,
 * for the reason given at vector_doc_scan_v1.  Host memory in, host memory out. */
#define YAMS_IFACE_TOPOLOGY_SMOOTH_V1 "topology_smooth_v1"
#define YAMS_IFACE_TOPOLOGY_SMOOTH_V1_VERSION 1u
typedef struct yams_topology_smooth_v1 {
    uint32_t abi_version; /* YAMS_IFACE_TOPOLOGY_SMOOTH_V1_VERSION */
    void* self;
    /* `hops` rounds of smoothing of rows [n][dim] over the list (row_offsets [n + 1], cols, weights: the order of a row's
     * edges is the order of its sums) into out [n][dim], the caller's array; out_diag nullable.  Statuses and limits of the
     * flat entry. */
    yams_status_t (*smooth)(void* self, const float* rows, uint64_t n, uint32_t dim, const uint64_t* row_offsets, const uint32_t* cols,
                            const float* weights, uint32_t hops, float* out, yams_sgc_diag_t* out_diag);
} yams_topology_smooth_v1;

/* The cluster artifacts (yams_cluster_centroids_host / _representatives_host / _residuals_host) for a host that holds the
 * embeddings in its own memory.  A separate interface, version 1, served by yams_plugin_get_interface and NOT listed in the
 * manifest, for the reason given at vector_doc_scan_v1.  Host memory in, host memory out; the outputs are allocated by the
 * plugin and released with the paired free_*.  Statuses and limits of the flat entries; an empty result gives null arrays. */
#define YAMS_IFACE_TOPOLOGY_ARTIFACTS_V1 "topology_artifacts_v1"
#define YAMS_IFACE_TOPOLOGY_ARTIFACTS_V1_VERSION 1u
typedef struct yams_topology_artifacts_v1 {
    uint32_t abi_version; /* YAMS_IFACE_TOPOLOGY_ARTIFACTS_V1_VERSION */
    void* self;
    /* *out_centroids [n_clusters][dim], *out_counts [n_clusters] */
    yams_status_t (*centroids)(void* self, const float* rows, uint64_t n, uint32_t dim, const uint64_t* cluster_offsets,
                               const uint32_t* members, uint32_t n_clusters, float** out_centroids, uint32_t** out_counts);
    /* *out_selected [n_clusters][n_extra] (null when n_extra == 0), *out_counts [n_clusters] */
    yams_status_t (*representatives)(void* self, const float* rows, uint64_t n, uint32_t dim, const uint64_t* cluster_offsets,
                                     const uint32_t* candidates, const float* centroids, const uint8_t* centroid_empty,
                                     uint32_t n_clusters, uint32_t n_extra, uint32_t** out_selected, uint32_t** out_counts);
    /* *out_cand_norm_sq [pairs]; with a primary also *out_primary_norm_sq [n] and *out_residual_dot [pairs] (without one both
     * pointers may be null and come back null).  pairs = cand_offsets[n], or n * n_clusters without lists. */
    yams_status_t (*residuals)(void* self, const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t n_clusters,
                               const uint32_t* primary, const uint64_t* cand_offsets, const uint32_t* cand, uint32_t form,
                               double** out_primary_norm_sq, double** out_cand_norm_sq, double** out_residual_dot);
    void (*free_centroids)(void* self, float* centroids, uint32_t* counts);
    void (*free_representatives)(void* self, uint32_t* selected, uint32_t* counts);
    void (*free_residuals)(void* self, double* primary_norm_sq, double* cand_norm_sq, double* residual_dot);
} yams_topology_artifacts_v1;

/* The cluster router's dense signal (yams_route_index_create_host / yams_route_dense_host) for a host that holds the cluster
 * vectors in its own memory.  A separate interface, version 1, served by yams_plugin_get_interface and NOT listed in the
 * manifest, for the reason given at vector_doc_scan_v1.  Host memory in, host memory out: every output is the caller's array.
 * An index lives on the device under an id until index_destroy (or the plugin's shutdown); calls on one index take turns,
 * calls on different indexes overlap.  Statuses and limits of the flat entries; an unknown id: YAMS_ERR_NOT_FOUND. */
#define YAMS_IFACE_TOPOLOGY_ROUTE_V1 "topology_route_v1"
#define YAMS_IFACE_TOPOLOGY_ROUTE_V1_VERSION 1u
typedef struct yams_topology_route_v1 {
    uint32_t abi_version; /* YAMS_IFACE_TOPOLOGY_ROUTE_V1_VERSION */
    void* self;
    /* out_norms: the caller's [n_vectors], nullable */
    yams_status_t (*index_create)(void* self, const float* vectors, uint64_t n_vectors, uint32_t dim, const uint32_t* cluster_offsets,
                                  const uint8_t* has_centroid, const uint16_t* position, uint32_t n_clusters, uint64_t* out_id,
                                  float* out_norms);
    yams_status_t (*index_info)(void* self, uint64_t id, yams_route_index_info_t* out_info);
    /* out_dense / out_observed: the caller's [n_queries][n_clusters]; out_evals: [n_queries]; out_diag nullable */
    yams_status_t (*dense)(void* self, uint64_t id, const float* queries, uint32_t n_queries, uint32_t rep_limit,
                           const uint32_t* candidates, float* out_dense, uint8_t* out_observed, uint32_t* out_evals,
                           yams_route_diag_t* out_diag);
    yams_status_t (*index_destroy)(void* self, uint64_t id);
} yams_topology_route_v1;

/* computePersistenceH0 (yams_quality_persistence_h0_host) for a host that holds the point cloud in its own memory.  A separate
 * interface, version 1, served by yams_plugin_get_interface and NOT listed in the manifest, for the reason given at
 * vector_doc_scan_v1.  Host memory in, host memory out; the two arrays are allocated by the plugin when asked for (a non-null
 * pointer to receive them) and released with free_persistence_h0.  Statuses and limits of the flat entry; m < 2 gives a null
 * *out_merge_weights. */
#define YAMS_IFACE_TOPOLOGY_QUALITY_V1 "topology_quality_v1"
#define YAMS_IFACE_TOPOLOGY_QUALITY_V1_VERSION 1u
typedef struct yams_topology_quality_v1 {
    uint32_t abi_version; /* YAMS_IFACE_TOPOLOGY_QUALITY_V1_VERSION */
    void* self;
    /* out_distances / out_merge_weights: nullable; *out_distances [m][m], *out_merge_weights [m - 1] */
    yams_status_t (*persistence_h0)(void* self, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select,
                                    uint32_t form, yams_persistence_h0_t* out, double** out_distances, double** out_merge_weights);
    void (*free_persistence_h0)(void* self, double* distances, double* merge_weights);
} yams_topology_quality_v1;

/* The topology build's input features (yams_features_aggregate_host / _variance_host / _compose_host) for a host that holds the
 * embeddings in its own memory.  A separate interface, version 1, served by yams_plugin_get_interface and NOT listed in the
 * manifest, for the reason given at vector_doc_scan_v1.  Host memory in, host memory out: every output is the caller's array.
 * Statuses and limits of the flat entries. */
#define YAMS_IFACE_TOPOLOGY_FEATURES_V1 "topology_features_v1"
#define YAMS_IFACE_TOPOLOGY_FEATURES_V1_VERSION 1u
typedef struct yams_topology_features_v1 {
    uint32_t abi_version; /* YAMS_IFACE_TOPOLOGY_FEATURES_V1_VERSION */
    void* self;
    /* out: the caller's [n_docs][dim]; out_counts: [n_docs] */
    yams_status_t (*aggregate)(void* self, const float* rows, uint64_t n_records, uint32_t dim, const uint64_t* doc_offsets,
                               const uint32_t* records, uint64_t n_docs, float* out, uint32_t* out_counts);
    /* out_mean / out_var: the caller's [dim] */
    yams_status_t (*variance)(void* self, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select,
                              uint32_t form, double* out_mean, double* out_var);
    /* out: the caller's [n][out_stride]; out_dims: [n] */
    yams_status_t (*compose)(void* self, const float* dense, uint64_t n, uint32_t dim, const float* weights, const float* entity,
                             uint32_t k, const uint8_t* entity_on, const uint32_t* sig, uint32_t sig_len, const uint8_t* sketch_on,
                             uint32_t sketch_dim, float alpha_e, float alpha_m, float* out, uint32_t out_stride, uint32_t* out_dims);
} yams_topology_features_v1;

/* The late-interaction rerank (yams_rerank_maxsim_host / yams_rerank_maxpool_host) for a host that holds the token embeddings in
 * its own memory.  A separate interface, version 1, served by yams_plugin_get_interface and NOT listed in the manifest, for the
 * reason given at vector_doc_scan_v1.  Host memory in, host memory out: every output is the caller's array.  Statuses and
 * limits of the flat entries. */
#define YAMS_IFACE_LATE_INTERACTION_RERANK_V1 "late_interaction_rerank_v1"
#define YAMS_IFACE_LATE_INTERACTION_RERANK_V1_VERSION 1u
typedef struct yams_late_interaction_rerank_v1 {
    uint32_t abi_version; /* YAMS_IFACE_LATE_INTERACTION_RERANK_V1_VERSION */
    void* self;
    /* out_scores: the caller's [n_docs]; out_rowmax / out_rowarg: nullable, the caller's [n_docs][tq]; diag: nullable */
    yams_status_t (*maxsim)(void* self, const float* query, uint32_t tq, uint32_t dim, const float* rows, const uint64_t* doc_offsets,
                            uint64_t n_docs, uint32_t form, float* out_scores, float* out_rowmax, uint32_t* out_rowarg,
                            yams_rerank_diag_t* diag);
    /* out: the caller's [n_docs][dim] */
    yams_status_t (*maxpool)(void* self, const float* rows, uint32_t dim, const uint64_t* doc_offsets, uint64_t n_docs, float* out);
} yams_late_interaction_rerank_v1;

/* The embedding model's pooling head (yams_embed_pool_* / yams_embed_normalize_*).  A separate interface, version 1, served by
 * yams_plugin_get_interface and NOT listed in the manifest, for the reason given at vector_doc_scan_v1.  pool and normalize take
 * host memory in and give host memory out: every output is the caller's array.  pool_device and normalize_device take the
 * hidden states (the rows) at a DEVICE address of the plugin's device (an encoder whose output is bound to device memory) and
 * everything else in host memory: only the masks and the batch * dim result cross the bus.  Statuses and limits of the flat
 * entries. */
#define YAMS_IFACE_EMBEDDING_POOL_V1 "embedding_pool_v1"
#define YAMS_IFACE_EMBEDDING_POOL_V1_VERSION 1u
typedef struct yams_embedding_pool_v1 {
    uint32_t abi_version; /* YAMS_IFACE_EMBEDDING_POOL_V1_VERSION */
    void* self;
    /* out: the caller's [batch][dim]; mask: nullable for CLS or mask_len == 0; diag: nullable */
    yams_status_t (*pool)(void* self, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask,
                          uint32_t mask_len, uint32_t mode, uint32_t flags, float* out, yams_embed_diag_t* diag);
    /* out: the caller's [batch][dim] */
    yams_status_t (*normalize)(void* self, const float* rows, uint64_t batch, uint32_t dim, float* out);
    /* hidden / rows: device addresses; mask, out, diag: the caller's host arrays */
    yams_status_t (*pool_device)(void* self, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask,
                                 uint32_t mask_len, uint32_t mode, uint32_t flags, float* out, yams_embed_diag_t* diag);
    yams_status_t (*normalize_device)(void* self, const float* rows, uint64_t batch, uint32_t dim, float* out);
} yams_embedding_pool_v1;

/* WHAT THE DEVICE IS WORSE AT IS REFUSED, NOT SERVED SLOWLY.  SHA-256 of one message is one sequential chain: a
 * GPU lane advances it at ~35 MB/s, a host core with SHA-NI at > 1 GB/s.  The device wins only with many
 * chains in flight.  So:
 *   - hash() of more than YAMS_HASH_LONE_CHAIN_MAX bytes returns YAMS_ERR_UNSUPPORTED;
 *   - hash_many() / verify_many() return YAMS_ERR_UNSUPPORTED when the call cannot finish before ONE host core
 *     would: longest message > max(YAMS_HASH_LONE_CHAIN_MAX, total bytes / YAMS_HASH_CHAIN_RATIO);
 * and the host hashes those with its own SHA256Hasher — the reference's convention for optional features
 * (abi_model_provider_adapter.cpp:121-122,159-170; UNSUPPORTED -> ErrorCode::NotImplemented, :528-552).
 * AccelSHA256Hasher (include/yams_accel/hasher.hpp) takes the host's hasher for exactly that.  The stream_*
 * functions are a compatibility door for hosts without one: correct, never fast. */
#define YAMS_HASH_LONE_CHAIN_MAX (1u << 20)
#define YAMS_HASH_CHAIN_RATIO 37u /* ~ 1.3 GB/s per host core / 35 MB/s per device chain */
typedef struct yams_content_hash_v1 {
    uint32_t abi_version; /* YAMS_IFACE_CONTENT_HASH_V1_VERSION */
    void* self;
    /* IContentHasher::hash one-shot: 64 hex chars + NUL into out_hex.  More than YAMS_HASH_LONE_CHAIN_MAX bytes:
     * YAMS_ERR_UNSUPPORTED (see above). */
    yams_status_t (*hash)(void* self, const uint8_t* data, size_t n, char out_hex[65]);
    /* Many messages per call (what makes a GPU worthwhile). */
    yams_status_t (*hash_many)(void* self, const uint8_t* const* msgs, const size_t* lens,
                               size_t n_msgs, char* out_hex /* [n_msgs][65] */);
    /* Streaming init/update/finalize (sha256_hasher.cpp:81-109): state lives in an opaque handle;
     * finalize re-initialises the handle like the reference (:103-106). */
    yams_status_t (*stream_create)(void* self, void** out_stream);
    yams_status_t (*stream_init)(void* self, void* stream);
    yams_status_t (*stream_update)(void* self, void* stream, const uint8_t* data, size_t n);
    yams_status_t (*stream_finalize)(void* self, void* stream, char out_hex[65]);
    void (*stream_destroy)(void* self, void* stream);
    /* Batched integrity check (ChunkValidator::validateChunks, src/integrity/chunk_validator.cpp:
     * 160-212): out_valid[i] = 1 iff SHA-256(msgs[i]) == expected_hex[i] (64 hex chars, either case;
     * a malformed expectation is simply a mismatch). */
    yams_status_t (*verify_many)(void* self, const uint8_t* const* msgs, const size_t* lens,
                                 const char* expected_hex /* [n_msgs][65] */, size_t n_msgs,
                                 uint8_t* out_valid);
    /* Device-resident set of known chunk hashes (the batched `storage_->exists` of
     * ContentStore::store, src/api/content_store_impl.cpp:246-287).  dedup_insert answers, per hash
     * and in order, "is this one new?" (neither in the set nor earlier in the same call) and adds
     * the new ones; dedup_contains only looks. */
    yams_status_t (*dedup_create)(void* self, uint64_t expected_entries, uint64_t* out_set_id);
    yams_status_t (*dedup_insert)(void* self, uint64_t set_id, const char* hashes_hex /* [n][65] */,
                                  size_t n, uint8_t* out_is_new);
    yams_status_t (*dedup_contains)(void* self, uint64_t set_id, const char* hashes_hex, size_t n,
                                    uint8_t* out_exists);
    yams_status_t (*dedup_size)(void* self, uint64_t set_id, uint64_t* out_entries);
    yams_status_t (*dedup_destroy)(void* self, uint64_t set_id);
} yams_content_hash_v1;

/* The compressed store's checksum (yams_crc32_many_host) for a host that holds the bytes in its own memory:
 * calculateCRC32 / updateCRC32 of include/yams/compression/compression_utils.h:16, 24 and the batched forms a device
 * needs to be worthwhile.  A separate interface, version 1, served by yams_plugin_get_interface and NOT listed in the
 * manifest, for the reason given at vector_doc_scan_v1.  Without a device every call returns YAMS_ERR_UNSUPPORTED.
 * crc32_many through this door is a second PCIe crossing of bytes chunk_many already saw; the flat ABI offers the
 * fused form (yams_crc32_chunks_device after yams_ingest_device). */
#define YAMS_IFACE_CONTENT_CHECKSUM_V1 "content_checksum_v1"
#define YAMS_IFACE_CONTENT_CHECKSUM_V1_VERSION 1u
typedef struct yams_content_checksum_v1 {
    uint32_t abi_version; /* YAMS_IFACE_CONTENT_CHECKSUM_V1_VERSION */
    void* self;
    yams_status_t (*crc32)(void* self, const uint8_t* data, size_t n, uint32_t* out);
    yams_status_t (*crc32_many)(void* self, const uint8_t* const* msgs, const size_t* lens, size_t n_msgs,
                                uint32_t* out /* [n_msgs] */);
    /* out_valid[i] = 1 iff CRC-32(msgs[i]) == expected[i] */
    yams_status_t (*verify_many)(void* self, const uint8_t* const* msgs, const size_t* lens,
                                 const uint32_t* expected /* [n_msgs] */, size_t n_msgs, uint8_t* out_valid);
} yams_content_checksum_v1;

typedef struct yams_chunk_ref_s { /* ChunkRef, chunker.h:32-41 (hash as hex) */
    uint64_t offset;
    uint64_t size;
    char hash_hex[65];
    char pad[7];
} yams_chunk_ref_t;

/* Result of chunk_many: the chunk tables of all buffers back to back. */
typedef struct yams_chunk_batch_s {
    size_t n_buffers;
    size_t n_chunks;
    size_t* first_chunk;       /* [n_buffers + 1]: buffer b owns chunks[first_chunk[b] .. first_chunk[b + 1])     */
    yams_chunk_ref_t* chunks;  /* [n_chunks]: offset within its buffer, size, SHA-256 of the chunk (hex)          */
    char* buffer_hash_hex;     /* [n_buffers][65]: SHA-256 of each whole buffer (the file hash of
                                  ContentStore::store, content_store_impl.cpp:199-231), or NULL if not asked for  */
} yams_chunk_batch_t;
#define YAMS_CHUNK_MANY_BUFFER_HASHES 1u
/* With YAMS_CHUNK_MANY_BUFFER_HASHES: buffers longer than yams_ingest_defer_threshold_host(sum of lens) come back with
 * an EMPTY buffer_hash_hex entry (first byte 0) — their whole-buffer chain would outlast the rest of the call; the
 * adapter's host hasher computes them while the device works (AccelChunker::chunkMany).  See
 * YAMS_INGEST_DEFER_LONG_BLOB_DIGESTS. */
#define YAMS_CHUNK_MANY_DEFER_LONG_BUFFER_HASHES 2u

typedef struct yams_chunker_v1 {
    uint32_t abi_version; /* YAMS_IFACE_CHUNKER_V1_VERSION */
    void* self;
    yams_status_t (*get_default_config)(void* self, uint32_t mode, yams_cdc_config_t* out_cfg);
    /* IChunker::chunkDataLazy: offsets, sizes and per-chunk SHA-256. */
    yams_status_t (*chunk_data)(void* self, const uint8_t* data, size_t n,
                                const yams_cdc_config_t* cfg, yams_chunk_ref_t** out_chunks,
                                size_t* out_count);
    void (*free_chunks)(void* self, yams_chunk_ref_t* chunks, size_t count);
    /* ---- version 2 (NULL in older builds: "not implemented", abi_model_provider_adapter.cpp:121-122) --------
     * MANY buffers per call — the shape that lets the device run at its ingest rate (yams_ingest_host: uploads
     * of batch i + 1 under the kernels of batch i; ~500 GB/s device-resident, PCIe-bound from host memory)
     * instead of one launch sequence per file: boundaries + per-chunk SHA-256 of every buffer and, with
     * YAMS_CHUNK_MANY_BUFFER_HASHES, the whole-buffer digests — everything ContentStore::store needs for a
     * batch of files (content_store_impl.cpp:199-231) in one call.  Release with free_chunk_batch. */
    yams_status_t (*chunk_many)(void* self, const uint8_t* const* buffers, const size_t* lens, size_t n_buffers,
                                const yams_cdc_config_t* cfg, uint32_t flags, yams_chunk_batch_t** out_batch);
    void (*free_chunk_batch)(void* self, yams_chunk_batch_t* batch);
    /* ---- version 3 -----------------------------------------------------------------------------------------
     * One window of a stream (yams_cdc_chunk_window_host): the first context_len bytes are history, chunks start
     * behind them; what AccelChunker::processStream calls once per window.  Release with free_chunks. */
    yams_status_t (*chunk_window)(void* self, const uint8_t* data, size_t n, size_t context_len,
                                  const yams_cdc_config_t* cfg, yams_chunk_ref_t** out_chunks, size_t* out_count);
} yams_chunker_v1;

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* YAMS_MI355X_ACCEL_H */
