// entity_api.cpp — yams_scan_entity_topk_device: IEntityStore::searchEntities behind the C ABI.
//
// Mirrors SqliteVecBackend::Impl::searchEntities (src/vector/sqlite_vec_backend.cpp:2801-2887): the rows the three optional
// column equalities admit, scored with VectorDatabase::computeCosineSimilarity (vector_database.cpp:1786-1810), kept at
// similarity >= threshold, the best k by similarity.  No query validation: zero / NaN / inf queries go through the arithmetic.
//   query norms -> [compaction of the admitted ordinals, when a mask or the filters restrict] -> per slice of queries:
//   entity_score_kernel (score, count, one key per row) -> block top-k -> emit (score bits, row, count).
#include <algorithm>
#include <cstring>
#include <vector>

#include "accel_ctx.h"
#include "entity_launch.h"
#include "scan_launch.h"

using namespace yams_accel;

namespace {
// bytes of keys one slice of queries may hold (the budget of doc_api.cpp): 64 queries x 1 M rows run as two slices of 32
constexpr uint64_t kEntityKeyBudget = 256ull << 20;
constexpr uint32_t kEntityFilterBits = YAMS_SCAN_ENTITY_FILTER_TYPE | YAMS_SCAN_ENTITY_FILTER_NODE_TYPE | YAMS_SCAN_ENTITY_FILTER_DOC;
} // namespace

extern "C" yams_status_t yams_scan_entity_topk_device(yams_accel_ctx* ctx, const yams_scan_corpus_t* corpus,
                                                      const yams_scan_entities_t* entities, const float* queries,
                                                      const yams_scan_entity_filter_t* filters, uint32_t n_queries, uint32_t k,
                                                      float similarity_threshold, float* out_scores, int64_t* out_rows,
                                                      uint32_t* out_counts, uint64_t* out_matching, yams_scan_diag_t* diag) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (!corpus) return fail(ctx, YAMS_ERR_INVALID_ARG, "null corpus");
    if (diag) std::memset(diag, 0, sizeof(*diag));
    if (n_queries == 0) return YAMS_OK;
    if (!out_counts) return fail(ctx, YAMS_ERR_INVALID_ARG, "null out_counts");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t nq = n_queries, dim = corpus->dim;
    if (k > YAMS_SCAN_MAX_K) return fail(ctx, YAMS_ERR_UNSUPPORTED, "k exceeds YAMS_SCAN_MAX_K");
    if (corpus->n_rows >= (1ull << 32)) return fail(ctx, YAMS_ERR_UNSUPPORTED, "shard must hold < 2^32 rows");
    if (corpus->stripe_rows) return fail(ctx, YAMS_ERR_UNSUPPORTED, "entity search over a striped shard");
    if (corpus->row_mask && corpus->row_mask_count > corpus->n_rows)
        return fail(ctx, YAMS_ERR_INVALID_ARG, "row_mask_count exceeds n_rows");
    const yams_scan_entities_t cols = entities ? *entities : yams_scan_entities_t{nullptr, nullptr, nullptr};
    // ---- the filters (host): which columns they name, whether they restrict the rows at all, the distinct ones
    // (an empty table, an empty mask or the empty query has no rows for a column to describe: empty results, whatever the
    // filters name — the reference returns an empty vector there)
    uint64_t n_items = (corpus->row_mask ? corpus->row_mask_count : corpus->n_rows);   // (a bound until the gather has run)
    const bool empty = dim == 0 || n_items == 0;
    bool any_pred = false, all_restrict = filters != nullptr;
    std::vector<yams_scan_entity_filter_t> uniq;
    for (uint32_t i = 0; filters && i < nq; ++i) {
        const yams_scan_entity_filter_t& f = filters[i];
        if (f.fields & ~kEntityFilterBits) return fail(ctx, YAMS_ERR_INVALID_ARG, "unknown entity filter field");
        if (empty) continue;
        if (((f.fields & YAMS_SCAN_ENTITY_FILTER_TYPE) && !cols.row_type) ||
            ((f.fields & YAMS_SCAN_ENTITY_FILTER_NODE_TYPE) && !cols.row_node_type) ||
            ((f.fields & YAMS_SCAN_ENTITY_FILTER_DOC) && !cols.row_doc))
            return fail(ctx, YAMS_ERR_INVALID_ARG, "an entity filter names a field whose column is null");
        if (f.fields == 0) { all_restrict = false; continue; }
        any_pred = true;
        if (std::none_of(uniq.begin(), uniq.end(), [&](const yams_scan_entity_filter_t& u) { return std::memcmp(&u, &f, sizeof f) == 0; }))
            uniq.push_back(f);
    }
    if (k == 0) {
        YA_HIP(ctx, hipMemsetAsync(out_counts, 0, static_cast<size_t>(nq) * 4, st));
        if (out_matching) YA_HIP(ctx, hipMemsetAsync(out_matching, 0, static_cast<size_t>(nq) * 8, st));
        YA_HIP(ctx, hipStreamSynchronize(st));
        return YAMS_OK;
    }
    if (!out_scores || !out_rows) return fail(ctx, YAMS_ERR_INVALID_ARG, "null outputs");
    // rows_sel form: a mask or filters that every query carries restrict the rows; else every row is an item
    const bool compact = corpus->row_mask != nullptr || all_restrict;
    auto empty_result = [&]() -> yams_status_t { // padded, empty results
        if (out_matching) YA_HIP(ctx, hipMemsetAsync(out_matching, 0, static_cast<size_t>(nq) * 8, st));
        YA_HIP(ctx, launch_entity_emit(st, nullptr, 0, nullptr, 0, nullptr, nullptr, corpus->row_base, 0, nq, k, out_scores, out_rows, out_counts));
        YA_HIP(ctx, hipStreamSynchronize(st));
        if (diag) { diag->used_exact_scan = 1; diag->rows_visited_observed = 1; diag->path = 1; }
        return YAMS_OK;
    };
    if (empty) return empty_result(); // the empty query (:2809-2811), an empty table or an empty mask
    if (!queries || !corpus->rows) return fail(ctx, YAMS_ERR_INVALID_ARG, "null queries / corpus rows");

    // ---- one pinned staging area for the call: the filters on their way in, the counters on their way out
    const size_t n_uniq = all_restrict ? uniq.size() : 0;   // (a query without a filter admits every row: no restriction)
    const size_t filt_bytes = any_pred ? (static_cast<size_t>(nq) + n_uniq) * sizeof(yams_scan_entity_filter_t) : 0;
    uint8_t* h_pin;
    const size_t pin_body = (std::max(filt_bytes, static_cast<size_t>(nq) * 16) + 15) & ~static_cast<size_t>(15);
    YA_TRY(pinned_get(ctx, pin_body + 64, (void**)&h_pin));
    yams_scan_entity_filter_t* d_filt = nullptr;
    if (any_pred) {
        YA_TRY(ws_get(ctx, "ent_filters", filt_bytes, (void**)&d_filt));
        std::memcpy(h_pin, filters, static_cast<size_t>(nq) * sizeof(yams_scan_entity_filter_t));
        if (n_uniq) std::memcpy(h_pin + static_cast<size_t>(nq) * sizeof(yams_scan_entity_filter_t), uniq.data(), n_uniq * sizeof(yams_scan_entity_filter_t));
        YA_HIP(ctx, hipMemcpyAsync(d_filt, h_pin, filt_bytes, hipMemcpyHostToDevice, st));
    }
    double* d_qnorm; unsigned long long* d_cnt;
    YA_TRY(ws_get(ctx, "ent_qnorm", static_cast<size_t>(nq) * 8, (void**)&d_qnorm));
    YA_TRY(ws_get(ctx, "ent_counts", static_cast<size_t>(nq) * 16, (void**)&d_cnt));
    unsigned long long* d_visited = d_cnt; unsigned long long* d_match = d_cnt + nq;
    YA_HIP(ctx, hipMemsetAsync(d_cnt, 0, static_cast<size_t>(nq) * 16, st));
    YA_HIP(ctx, launch_entity_qnorm(st, queries, nq, dim, d_qnorm));

    const uint32_t* rows_sel = nullptr;
    unsigned long long* d_nsel = nullptr;
    if (compact) {
        uint32_t* sel;
        YA_TRY(ws_get(ctx, "ent_rows_sel", static_cast<size_t>(corpus->n_rows) * 4, (void**)&sel));
        YA_TRY(ws_get(ctx, "ent_nsel", 8, (void**)&d_nsel));
        YA_HIP(ctx, launch_compact_rows(st, corpus->row_mask, corpus->n_rows, n_uniq ? d_filt + nq : nullptr,
                                        static_cast<uint32_t>(n_uniq), cols, sel, d_nsel));
        rows_sel = sel;
        // the admitted count comes back (8 bytes): keys, selection and the score grid are sized by it, not by the row count
        uint64_t* h_nsel = reinterpret_cast<uint64_t*>(h_pin + pin_body);
        YA_HIP(ctx, hipMemcpyAsync(h_nsel, d_nsel, 8, hipMemcpyDeviceToHost, st));
        YA_HIP(ctx, hipStreamSynchronize(st));
        n_items = std::min<uint64_t>(n_items, *h_nsel);
        if (n_items == 0) return empty_result();
    }

    // ---- slices of queries whose keys fit the budget (whole groups of 8 queries where a slice holds that many)
    uint32_t slice = static_cast<uint32_t>(std::min<uint64_t>(nq, std::max<uint64_t>(1, kEntityKeyBudget / (n_items * 8))));
    if (slice > 8) slice -= slice % 8;
    const uint64_t chunks = (n_items + kSelectCap - 1) / kSelectCap;
    unsigned long long* d_keys; uint64_t* d_work;
    YA_TRY(ws_get(ctx, "ent_keys", static_cast<size_t>(slice) * n_items * 8, (void**)&d_keys));
    YA_TRY(ws_get(ctx, "ent_work", static_cast<size_t>(2) * slice * chunks * k * 8, (void**)&d_work));
    for (uint32_t q0 = 0; q0 < nq; q0 += slice) {
        const uint32_t ns = std::min(slice, nq - q0);
        const uint64_t* res = nullptr; uint64_t res_stride = 0;
        {
            TimedRegion tr(ctx, "entity_score");
            YA_HIP(ctx, launch_entity_score(st, corpus->rows, corpus->n_rows, dim, queries, d_qnorm, d_filt, q0, ns, cols, rows_sel,
                                            d_nsel, n_items, similarity_threshold, d_keys, d_visited, d_match));
            tr.end();
        }
        {
            TimedRegion tr(ctx, "entity_select");
            YA_HIP(ctx, launch_topk_keys(st, reinterpret_cast<const uint64_t*>(d_keys), n_items, static_cast<uint32_t>(n_items), ns, k,
                                         d_work, &res, &res_stride));
            tr.end();
        }
        YA_HIP(ctx, launch_entity_emit(st, reinterpret_cast<const unsigned long long*>(res), res_stride, corpus->rows, dim, queries,
                                       d_qnorm, corpus->row_base, q0, ns, k, out_scores, out_rows, out_counts));
    }
    if (out_matching) YA_HIP(ctx, hipMemcpyAsync(out_matching, d_match, static_cast<size_t>(nq) * 8, hipMemcpyDeviceToDevice, st));
    if (diag) YA_HIP(ctx, hipMemcpyAsync(h_pin, d_cnt, static_cast<size_t>(nq) * 16, hipMemcpyDeviceToHost, st));
    YA_HIP(ctx, hipStreamSynchronize(st));
    if (diag) {
        const uint64_t* h = reinterpret_cast<const uint64_t*>(h_pin);
        uint64_t visited = 0, matching = 0;
        for (uint32_t i = 0; i < nq; ++i) { visited += h[i]; matching += h[nq + i]; }
        diag->used_exact_scan = 1; diag->rows_visited_observed = 1;
        diag->rows_visited = visited; diag->exact_distance_evaluations = visited; diag->rescored_rows = visited;
        diag->returned_rows = matching;
        diag->path = 1; diag->filter_tier = 0;
    }
    return YAMS_OK;
}
