// doc_api.cpp — yams_scan_doc_topk_device: document-level selection (CandidateFilterMode::DocumentTopK) behind the C ABI.
//
// Mirrors the exact arm of SqliteVecBackend's document search (src/vector/sqlite_vec_backend.cpp:1508-1518): every
// matching row of the allowed set (the fp64 cosine of :4253-4279), then retainBestRecordPerDocument (:86-125) — with the
// per-document reduction on the device, next to the score that decides it:
//   prep (validate, fp64 norms) -> per slice of queries: doc_score_kernel (score, count, atomicMax per document)
//   -> selection keys (score, doc_rank) -> block top-k -> emit (score, row, document, count).
#include <algorithm>
#include <cstring>
#include <vector>

#include "accel_ctx.h"
#include "doc_launch.h"
#include "scan_launch.h"

using namespace yams_accel;

namespace {
// bytes of per-document keys (doc_key + selection keys) one slice of queries may hold: 600 queries x 1 M documents run
// as slices of 16 queries
constexpr uint64_t kDocKeyBudget = 256ull << 20;
// an allow-mask that lets fewer than one row in 8 through is gathered first (launch_compact_mask), a denser one is
// read in place
constexpr uint64_t kSparseDivisor = 8;
// the flags a DocumentTopK call may carry: filter-choice bits only (the call scores every allowed row in fp64 anyway)
constexpr uint32_t kDocFlagsAllowed = YAMS_SCAN_FLAG_FORCE_EXACT | YAMS_SCAN_FLAG_F32_FILTER | YAMS_SCAN_FLAG_SPLIT_FILTER |
                                      YAMS_SCAN_FLAG_WIDE_TILE | YAMS_SCAN_FLAG_NO_I8_FILTER | YAMS_SCAN_FLAG_RESIDENT_QUERIES;
} // namespace

extern "C" yams_status_t yams_scan_doc_topk_device(yams_accel_ctx* ctx, const yams_scan_corpus_t* corpus,
                                                   const yams_scan_docs_t* docs, const float* queries, uint32_t n_queries,
                                                   const yams_scan_params_t* params, float* out_scores, int64_t* out_rows,
                                                   uint32_t* out_docs, uint32_t* out_counts, uint64_t* out_matching,
                                                   yams_scan_diag_t* diag) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (!corpus || !docs || !params) return fail(ctx, YAMS_ERR_INVALID_ARG, "null corpus / documents / params");
    if (diag) std::memset(diag, 0, sizeof(*diag));
    if (params->metric != YAMS_SCAN_COSINE) return fail(ctx, YAMS_ERR_UNSUPPORTED, "document-level selection is cosine only");
    if (params->flags & ~kDocFlagsAllowed)
        return fail(ctx, YAMS_ERR_UNSUPPORTED, "document-level selection takes no record-path, threshold or L2 flags");
    if (n_queries == 0) return YAMS_OK;
    if (!queries || !out_counts) return fail(ctx, YAMS_ERR_INVALID_ARG, "null queries/out_counts");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t nq = n_queries, dim = corpus->dim, k = params->k;
    if (dim == 0 || k == 0) { // empty query / k == 0: an empty result before the query is validated (:4123-4126)
        YA_HIP(ctx, hipMemsetAsync(out_counts, 0, static_cast<size_t>(nq) * 4, st));
        if (out_matching) YA_HIP(ctx, hipMemsetAsync(out_matching, 0, static_cast<size_t>(nq) * 8, st));
        YA_HIP(ctx, hipStreamSynchronize(st));
        return YAMS_OK;
    }
    if (!out_scores || !out_rows) return fail(ctx, YAMS_ERR_INVALID_ARG, "null outputs");
    if (k > YAMS_SCAN_MAX_K) return fail(ctx, YAMS_ERR_UNSUPPORTED, "k exceeds YAMS_SCAN_MAX_K");
    if (dim > YAMS_SCAN_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_SCAN_MAX_DIM (8192)");
    if (corpus->n_rows >= (1ull << 32)) return fail(ctx, YAMS_ERR_UNSUPPORTED, "shard must hold < 2^32 rows");
    if (corpus->stripe_rows) return fail(ctx, YAMS_ERR_UNSUPPORTED, "document-level selection over a striped shard");
    if (corpus->n_rows > 0 && (!corpus->rows || !docs->row_doc)) return fail(ctx, YAMS_ERR_INVALID_ARG, "null corpus rows / row_doc");
    if ((corpus->tie_rank == nullptr) != (corpus->rank_row == nullptr))
        return fail(ctx, YAMS_ERR_INVALID_ARG, "tie_rank and rank_row must be given together");
    if (corpus->row_mask && corpus->row_mask_count > corpus->n_rows)
        return fail(ctx, YAMS_ERR_INVALID_ARG, "row_mask_count exceeds n_rows");
    if (docs->n_docs == YAMS_SCAN_NO_DOC) return fail(ctx, YAMS_ERR_INVALID_ARG, "n_docs must be below YAMS_SCAN_NO_DOC");
    const uint32_t n_docs = docs->n_docs;
    const uint64_t n_eff = corpus->row_mask ? corpus->row_mask_count : corpus->n_rows;

    // ---- the queries: validation and fp64 norms (prep_queries_kernel, as the exact scan does)
    float* d_qprep; double* d_qnorm; uint32_t* d_qflags; uint32_t* d_bad; unsigned long long* d_match;
    YA_TRY(ws_get(ctx, "doc_qprep", static_cast<size_t>(nq) * dim * 4, (void**)&d_qprep));
    YA_TRY(ws_get(ctx, "doc_qnorm", static_cast<size_t>(nq) * 8, (void**)&d_qnorm));
    YA_TRY(ws_get(ctx, "doc_qflags", static_cast<size_t>(nq) * 4, (void**)&d_qflags));
    YA_TRY(ws_get(ctx, "doc_match", static_cast<size_t>(nq) * 8, (void**)&d_match));
    YA_TRY(ws_get(ctx, "doc_bad", 16, (void**)&d_bad));
    YA_HIP(ctx, hipMemsetAsync(d_match, 0, static_cast<size_t>(nq) * 8, st));
    YA_HIP(ctx, hipMemsetAsync(d_bad, 0, 16, st));
    YA_HIP(ctx, launch_prep_queries(st, queries, nq, dim, YAMS_SCAN_COSINE, d_qprep, d_qnorm, nullptr, d_qflags));

    // ---- the rows: a sparse allow-mask is gathered into a list of ordinals (any order: keys carry the tie rank)
    const uint32_t* rows_sel = nullptr;
    unsigned long long* d_nsel = nullptr;
    uint64_t n_items = corpus->n_rows;
    if (corpus->row_mask && n_eff * kSparseDivisor < corpus->n_rows) {
        uint32_t* sel;
        YA_TRY(ws_get(ctx, "doc_rows_sel", static_cast<size_t>(std::max<uint64_t>(corpus->n_rows, 1)) * 4, (void**)&sel));
        YA_TRY(ws_get(ctx, "doc_nsel", 8, (void**)&d_nsel));
        YA_HIP(ctx, launch_compact_mask(st, corpus->row_mask, corpus->n_rows, sel, d_nsel));
        rows_sel = sel;
        n_items = n_eff;
    }
    // ---- the document order: inverse of doc_rank (validated: a permutation of 0 .. n_docs - 1)
    uint32_t* d_rank_inv = nullptr;
    if (docs->doc_rank && n_docs) {
        YA_TRY(ws_get(ctx, "doc_rank_inv", static_cast<size_t>(n_docs) * 4, (void**)&d_rank_inv));
        YA_HIP(ctx, launch_doc_rank_inverse(st, docs->doc_rank, n_docs, d_rank_inv, d_bad));
    }

    // ---- slices of queries whose per-document keys fit the budget
    const uint64_t per_slot = std::max<uint64_t>(n_docs, 1) * 16;
    const uint32_t slice = static_cast<uint32_t>(std::min<uint64_t>(nq, std::max<uint64_t>(1, kDocKeyBudget / per_slot)));
    unsigned long long* d_key = nullptr; unsigned long long* d_sel = nullptr; uint64_t* d_work = nullptr;
    if (n_docs) {
        const uint64_t chunks = (static_cast<uint64_t>(n_docs) + kSelectCap - 1) / kSelectCap;
        YA_TRY(ws_get(ctx, "doc_key", static_cast<size_t>(slice) * n_docs * 8, (void**)&d_key));
        YA_TRY(ws_get(ctx, "doc_sel", static_cast<size_t>(slice) * n_docs * 8, (void**)&d_sel));
        YA_TRY(ws_get(ctx, "doc_work", static_cast<size_t>(2) * slice * chunks * k * 8, (void**)&d_work));
    }
    const uint32_t* rank_row = corpus->tie_rank ? corpus->rank_row : nullptr;
    for (uint32_t q0 = 0; q0 < nq; q0 += slice) {
        const uint32_t ns = std::min(slice, nq - q0);
        const uint64_t* res = nullptr; uint64_t res_stride = 0;
        if (n_docs) YA_HIP(ctx, hipMemsetAsync(d_key, 0, static_cast<size_t>(ns) * n_docs * 8, st));
        {
            TimedRegion tr(ctx, "doc_score");
            YA_HIP(ctx, launch_doc_score(st, corpus->rows, corpus->n_rows, dim, queries, d_qnorm, q0, ns, corpus->tie_rank,
                                         corpus->row_mask, rows_sel, d_nsel, n_items, docs->row_doc, n_docs,
                                         params->similarity_threshold, d_key, d_match, d_bad));
            tr.end();
        }
        if (n_docs) {
            TimedRegion tr(ctx, "doc_select");
            YA_HIP(ctx, launch_doc_sel_keys(st, d_key, docs->doc_rank, n_docs, ns, d_sel));
            YA_HIP(ctx, launch_topk_keys(st, reinterpret_cast<const uint64_t*>(d_sel), n_docs, n_docs, ns, k, d_work, &res,
                                         &res_stride));
            tr.end();
        }
        YA_HIP(ctx, launch_doc_emit(st, reinterpret_cast<const unsigned long long*>(res), res_stride, d_key, n_docs, corpus->rows,
                                    dim, queries, d_qnorm, d_rank_inv, rank_row, corpus->row_base, q0, ns, k, out_scores, out_rows, out_docs, out_counts));
    }
    if (out_matching) YA_HIP(ctx, hipMemcpyAsync(out_matching, d_match, static_cast<size_t>(nq) * 8, hipMemcpyDeviceToDevice, st));

    // ---- one look back: query flags, layout errors, matching rows (diagnostics)
    uint32_t* h_pin;
    YA_TRY(pinned_get(ctx, static_cast<size_t>(nq) * 12 + 64, (void**)&h_pin));
    uint64_t* h_match = reinterpret_cast<uint64_t*>(h_pin);
    uint32_t* h_flags = h_pin + 2 * static_cast<size_t>(nq);
    uint32_t* h_bad = h_flags + nq;
    YA_HIP(ctx, hipMemcpyAsync(h_flags, d_qflags, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost, st));
    YA_HIP(ctx, hipMemcpyAsync(h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    if (diag) YA_HIP(ctx, hipMemcpyAsync(h_match, d_match, static_cast<size_t>(nq) * 8, hipMemcpyDeviceToHost, st));
    YA_HIP(ctx, hipStreamSynchronize(st));
    for (uint32_t i = 0; i < nq; ++i) // a non-finite query or norm^2 < 1e-10 fails the batch (:4127-4130, :1635-1647)
        if (h_flags[i] != 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "Exact vector search requires a finite, non-zero query embedding");
    if (*h_bad & 1u) return fail(ctx, YAMS_ERR_INVALID_ARG, "row_doc holds a document ordinal >= n_docs");
    if (*h_bad & 2u) return fail(ctx, YAMS_ERR_INVALID_ARG, "doc_rank is not a permutation of 0 .. n_docs - 1");
    if (diag) {
        uint64_t matching = 0;
        for (uint32_t i = 0; i < nq; ++i) matching += h_match[i];
        diag->used_exact_scan = 1; diag->rows_visited_observed = 1;
        diag->rows_visited = static_cast<uint64_t>(nq) * n_eff;
        diag->exact_distance_evaluations = static_cast<uint64_t>(nq) * n_eff;
        diag->rescored_rows = static_cast<uint64_t>(nq) * n_eff;
        diag->returned_rows = matching; // the reference's returnedRows of this path: set before the reduction
        diag->path = 1; diag->filter_tier = 0;
    }
    return YAMS_OK;
}
