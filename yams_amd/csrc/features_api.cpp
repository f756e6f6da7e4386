// features_api.cpp — yams_features_aggregate / _variance / _compose (_device and _host): the array arithmetic of
// TopologyInputExtractor::extract (aggregateEmbedding, computeVarianceWeights' two passes, composeFeatureVector) behind the C
// ABI.  Every entry: the limits (no device needed) -> argument checks -> the list totals read back -> ONE read-back of the check
// flags -> the work.  Nothing is written to an output before every refusal is known.
#include <cstring>
#include <vector>

#include "accel_ctx.h"
#include "arg_checks.h"
#include "artifact_launch.h"
#include "features_launch.h"
#include "host_stage.h"

using namespace yams_accel;

namespace {

static_assert(YAMS_FEATURES_MAX_DIM == kFeatMaxDim && YAMS_FEATURES_MAX_SIG_LEN == kFeatMaxSigLen, "the header's limits are the launchers'");
constexpr uint64_t kMaxRows = 1ull << 31;
constexpr uint64_t kMaxEntries = 1ull << 32;

// The list checks on the device: offsets from 0, never decreasing, ending at `total`; entries < limit.  Synchronises.
yams_status_t check_lists(yams_accel_ctx* ctx, const uint64_t* d_off, uint64_t lists, uint64_t total, const uint32_t* d_idx, uint32_t limit,
                          const char* what) {
    hipStream_t st = ctx->stream;
    uint32_t* d_flags; uint32_t flags;
    YA_TRY(flags_get(ctx, 4, &d_flags));
    YA_HIP(ctx, launch_artifact_check(st, d_off, d_off ? lists : 0, total, d_idx, limit, d_flags));
    YA_TRY(read_words(ctx, d_flags, 1, &flags));
    if (flags & 1u) return fail(ctx, YAMS_ERR_INVALID_ARG, std::string(what) + ": the offsets do not start at 0 or decrease");
    if (flags & 2u) return fail(ctx, YAMS_ERR_INVALID_ARG, std::string(what) + ": an index is out of range");
    return YAMS_OK;
}

// ---- aggregate: what needs no device ---------------------------------------------------------------------------------------
yams_status_t check_aggregate(yams_accel_ctx* ctx, uint64_t n_records, uint32_t dim, const uint64_t* doc_offsets, uint64_t n_docs,
                              const float* out, const uint32_t* out_counts) {
    if (n_records >= kMaxRows || n_docs >= kMaxRows) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n_records and n_docs must be < 2^31");
    if (dim > YAMS_FEATURES_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_FEATURES_MAX_DIM");
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (n_docs && (!doc_offsets || !out || !out_counts)) return fail(ctx, YAMS_ERR_INVALID_ARG, "null doc_offsets or output");
    return YAMS_OK;
}
// once the lists' total is known
yams_status_t check_aggregate_total(yams_accel_ctx* ctx, const float* rows, uint64_t n_records, uint32_t dim, const uint32_t* records,
                                    uint64_t total, uint64_t n_docs, const float* out, const uint32_t* out_counts) {
    if (total >= kMaxEntries) return fail(ctx, YAMS_ERR_UNSUPPORTED, "the lists must hold fewer than 2^32 entries");
    if (total && (!records || !rows)) return fail(ctx, YAMS_ERR_INVALID_ARG, "null rows or records");
    const size_t rb = static_cast<size_t>(n_records) * dim * 4;
    if (overlaps(out, static_cast<size_t>(n_docs) * dim * 4, rows, rb) || overlaps(out_counts, static_cast<size_t>(n_docs) * 4, rows, rb))
        return fail(ctx, YAMS_ERR_INVALID_ARG, "an output overlaps rows");
    return YAMS_OK;
}

// ---- variance ----------------------------------------------------------------------------------------------------------------
yams_status_t check_variance(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, uint64_t m, uint32_t form,
                             const double* out_mean, const double* out_var) {
    if (n >= kMaxRows) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n must be < 2^31");
    if (m >= kMaxEntries) return fail(ctx, YAMS_ERR_UNSUPPORTED, "select must hold fewer than 2^32 entries");
    if (dim > YAMS_FEATURES_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_FEATURES_MAX_DIM");
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (form != YAMS_RESIDUAL_SEPARATE && form != YAMS_RESIDUAL_FUSED) return fail(ctx, YAMS_ERR_INVALID_ARG, "unknown form");
    if (m == 0) return YAMS_OK;
    if (!rows || !out_mean || !out_var) return fail(ctx, YAMS_ERR_INVALID_ARG, "null rows or output");
    const size_t rb = static_cast<size_t>(n) * dim * 4, ob = static_cast<size_t>(dim) * 8;
    if (overlaps(out_mean, ob, rows, rb) || overlaps(out_var, ob, rows, rb) || overlaps(out_mean, ob, out_var, ob))
        return fail(ctx, YAMS_ERR_INVALID_ARG, "an output overlaps rows or the other output");
    return YAMS_OK;
}

// ---- compose -----------------------------------------------------------------------------------------------------------------
struct ComposeShape { std::vector<uint32_t> kept; std::vector<float> kept_w; uint32_t kc; bool entity, sketch; uint32_t longest; };

yams_status_t check_compose(yams_accel_ctx* ctx, const float* dense, uint64_t n, uint32_t dim, const float* weights, const float* entity,
                            uint32_t k, const uint8_t* entity_on, const uint32_t* sig, uint32_t sig_len, const uint8_t* sketch_on,
                            uint32_t sketch_dim, const float* out, uint32_t out_stride, const uint32_t* out_dims, ComposeShape* sh) {
    if (n >= kMaxRows) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n must be < 2^31");
    if (dim > YAMS_FEATURES_MAX_DIM || k > YAMS_FEATURES_MAX_DIM || sketch_dim > YAMS_FEATURES_MAX_DIM)
        return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim, K or sketch_dim exceeds YAMS_FEATURES_MAX_DIM");
    if (sig_len > YAMS_FEATURES_MAX_SIG_LEN) return fail(ctx, YAMS_ERR_UNSUPPORTED, "sig_len exceeds YAMS_FEATURES_MAX_SIG_LEN");
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    sh->entity = entity && k;
    sh->sketch = sig && sig_len && sketch_dim;
    sh->kept.clear();
    sh->kept_w.clear();
    if (weights)      // :175-179 — the indices of the weights > 0.0F, ascending (a NaN is not kept)
        for (uint32_t i = 0; i < dim; ++i)
            if (weights[i] > 0.0f) { sh->kept.push_back(i); sh->kept_w.push_back(weights[i]); }
    sh->kc = weights ? static_cast<uint32_t>(sh->kept.size()) : dim;
    sh->longest = sh->kc + (sh->entity ? k : 0u) + (sh->sketch ? sketch_dim : 0u);
    if (n == 0) return YAMS_OK;
    if (!dense || !out_dims || (out_stride && !out)) return fail(ctx, YAMS_ERR_INVALID_ARG, "null dense or output");
    if ((sh->entity && !entity_on) || (sh->sketch && !sketch_on)) return fail(ctx, YAMS_ERR_INVALID_ARG, "a part needs its per-row switch");
    if (out_stride < sh->longest) return fail(ctx, YAMS_ERR_INVALID_ARG, "out_stride is smaller than the longest possible row");
    const size_t ob = static_cast<size_t>(n) * out_stride * 4, db = static_cast<size_t>(n) * 4;
    const struct { const void* p; size_t bytes; } in[] = {{dense, static_cast<size_t>(n) * dim * 4},
                                                          {sh->entity ? entity : nullptr, static_cast<size_t>(n) * k * 4},
                                                          {sh->entity ? entity_on : nullptr, static_cast<size_t>(n)},
                                                          {sh->sketch ? sig : nullptr, static_cast<size_t>(n) * sig_len * 4},
                                                          {sh->sketch ? sketch_on : nullptr, static_cast<size_t>(n)}};
    for (const auto& a : in)
        if (overlaps(out, ob, a.p, a.bytes) || overlaps(out_dims, db, a.p, a.bytes)) return fail(ctx, YAMS_ERR_INVALID_ARG, "an output overlaps an input");
    if (overlaps(out, ob, out_dims, db)) return fail(ctx, YAMS_ERR_INVALID_ARG, "out overlaps out_dims");
    return YAMS_OK;
}

} // namespace

// ---- aggregate ---------------------------------------------------------------------------------------------------------------
extern "C" yams_status_t yams_features_aggregate_device(yams_accel_ctx* ctx, const float* rows, uint64_t n_records, uint32_t dim,
                                                        const uint64_t* doc_offsets, const uint32_t* records, uint64_t n_docs, float* out,
                                                        uint32_t* out_counts) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_aggregate(ctx, n_records, dim, doc_offsets, n_docs, out, out_counts));
    if (n_docs == 0) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    uint64_t total;
    YA_TRY(read_words(ctx, doc_offsets + n_docs, 2, &total));
    YA_TRY(check_aggregate_total(ctx, rows, n_records, dim, records, total, n_docs, out, out_counts));
    YA_TRY(check_lists(ctx, doc_offsets, n_docs, total, records, static_cast<uint32_t>(n_records), "records"));
    {
        TimedRegion tr(ctx, "features_aggregate");
        YA_HIP(ctx, launch_features_aggregate(st, rows, dim, doc_offsets, records, static_cast<uint32_t>(n_docs), out, out_counts));
        tr.end();
    }
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

extern "C" yams_status_t yams_features_aggregate_host(yams_accel_ctx* ctx, const float* rows, uint64_t n_records, uint32_t dim,
                                                      const uint64_t* doc_offsets, const uint32_t* records, uint64_t n_docs, float* out,
                                                      uint32_t* out_counts) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_aggregate(ctx, n_records, dim, doc_offsets, n_docs, out, out_counts));
    if (n_docs == 0) return YAMS_OK;
    // judged here, before an upload is sized by them
    if (!offsets_ascend(doc_offsets, n_docs)) return fail(ctx, YAMS_ERR_INVALID_ARG, "records: the offsets do not start at 0 or decrease");
    const uint64_t total = doc_offsets[n_docs];
    YA_TRY(check_aggregate_total(ctx, rows, n_records, dim, records, total, n_docs, out, out_counts));
    HostStage hs(ctx);
    const size_t nd = static_cast<size_t>(n_docs);
    const float* d_rows = hs.up("feat_host_rows", rows, static_cast<size_t>(n_records) * dim);
    const uint64_t* d_off = hs.up("feat_host_offsets", doc_offsets, nd + 1);
    const uint32_t* d_rec = hs.up("feat_host_list", records, static_cast<size_t>(total));
    float* d_out = hs.room<float>("feat_host_out", nd * dim);
    uint32_t* d_cnt = hs.room<uint32_t>("feat_host_counts", nd);
    YA_TRY(hs.status());
    YA_TRY(yams_features_aggregate_device(ctx, d_rows, n_records, dim, d_off, d_rec, n_docs, d_out, d_cnt));
    hs.down(out, d_out, nd * dim);
    hs.down(out_counts, d_cnt, nd);
    return hs.finish();
}

// ---- variance ----------------------------------------------------------------------------------------------------------------
extern "C" yams_status_t yams_features_variance_device(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                       const uint32_t* select, uint64_t n_select, uint32_t form, double* out_mean,
                                                       double* out_var) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    const uint64_t m = select ? n_select : n;
    YA_TRY(check_variance(ctx, rows, n, dim, m, form, out_mean, out_var));
    if (m == 0) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    if (select) YA_TRY(check_lists(ctx, nullptr, 0, m, select, static_cast<uint32_t>(n), "select"));
    {
        TimedRegion tr(ctx, "features_variance");
        YA_HIP(ctx, launch_features_variance(st, rows, dim, select, static_cast<uint32_t>(m), form == YAMS_RESIDUAL_FUSED, out_mean, out_var));
        tr.end();
    }
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

extern "C" yams_status_t yams_features_variance_host(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                     const uint32_t* select, uint64_t n_select, uint32_t form, double* out_mean,
                                                     double* out_var) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    const uint64_t m = select ? n_select : n;
    YA_TRY(check_variance(ctx, rows, n, dim, m, form, out_mean, out_var));
    if (m == 0) return YAMS_OK;
    if (select && !indices_below(select, m, n)) return fail(ctx, YAMS_ERR_INVALID_ARG, "select: an index is out of range");
    // only the sample rows travel, packed in the order of the sums
    std::vector<float> packed;
    if (select) {
        packed.resize(static_cast<size_t>(m) * dim);
        gather_rows(rows, dim, select, m, packed.data());
    }
    HostStage hs(ctx);
    const float* d_rows = hs.up("feat_host_rows", select ? packed.data() : rows, static_cast<size_t>(m) * dim);
    double* d_out = hs.room<double>("feat_host_moments", static_cast<size_t>(dim) * 2);
    YA_TRY(hs.finish());      // `packed` goes away
    YA_TRY(yams_features_variance_device(ctx, d_rows, m, dim, nullptr, 0, form, d_out, d_out + dim));
    hs.down(out_mean, d_out, dim);
    hs.down(out_var, d_out + dim, dim);
    return hs.finish();
}

// ---- compose -----------------------------------------------------------------------------------------------------------------
namespace {

// The work over device arrays; sh is check_compose's.  Synchronises.
yams_status_t run_compose(yams_accel_ctx* ctx, const ComposeShape& sh, FeatComposeArgs a) {
    hipStream_t st = ctx->stream;
    a.kc = sh.kc;
    a.kept = nullptr;
    a.kept_w = nullptr;
    if (!sh.entity) a.entity = nullptr;
    if (!sh.sketch) a.sig = nullptr;
    double* d_nsq = nullptr;
    if (sh.kc) YA_TRY(ws_get(ctx, "feat_nsq", static_cast<size_t>(a.n) * 8, (void**)&d_nsq));
    if (!sh.kept.empty()) {      // the kept columns and their weights: pinned, so that the copy may outlive this frame
        uint32_t* d_kept; uint8_t* h_pin;
        const size_t kb = static_cast<size_t>(sh.kc) * 4;
        YA_TRY(ws_get(ctx, "feat_kept", kb * 2, (void**)&d_kept));
        YA_TRY(pinned_get(ctx, kb * 2, (void**)&h_pin));
        std::memcpy(h_pin, sh.kept.data(), kb);
        std::memcpy(h_pin + kb, sh.kept_w.data(), kb);
        YA_HIP(ctx, hipMemcpyAsync(d_kept, h_pin, kb * 2, hipMemcpyHostToDevice, st));
        a.kept = d_kept;
        a.kept_w = reinterpret_cast<const float*>(d_kept + sh.kc);
    }
    a.nsq = d_nsq;
    TimedRegion tr(ctx, "features_compose");
    hipError_t e = launch_features_row_nsq(st, a.dense, a.n, a.dim, a.kept, a.kept_w, a.kc, d_nsq);
    if (e == hipSuccess) e = launch_features_compose_store(st, a);
    if (e == hipSuccess) e = launch_features_compose_sketch(st, a);
    tr.end();
    YA_HIP(ctx, e);
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

} // namespace

extern "C" yams_status_t yams_features_compose_device(yams_accel_ctx* ctx, const float* dense, uint64_t n, uint32_t dim, const float* weights,
                                                      const float* entity, uint32_t k, const uint8_t* entity_on, const uint32_t* sig,
                                                      uint32_t sig_len, const uint8_t* sketch_on, uint32_t sketch_dim, float alpha_e,
                                                      float alpha_m, float* out, uint32_t out_stride, uint32_t* out_dims) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    ComposeShape sh;
    YA_TRY(check_compose(ctx, dense, n, dim, weights, entity, k, entity_on, sig, sig_len, sketch_on, sketch_dim, out, out_stride, out_dims, &sh));
    if (n == 0) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    FeatComposeArgs a{};
    a.dense = dense; a.n = n; a.dim = dim;
    a.entity = entity; a.k = k; a.entity_on = entity_on;
    a.sig = sig; a.sig_len = sig_len; a.sketch_on = sketch_on; a.sketch_dim = sketch_dim;
    a.alpha_e = alpha_e; a.alpha_m = alpha_m;
    a.out = out; a.out_stride = out_stride; a.out_dims = out_dims;
    return run_compose(ctx, sh, a);
}

extern "C" yams_status_t yams_features_compose_host(yams_accel_ctx* ctx, const float* dense, uint64_t n, uint32_t dim, const float* weights,
                                                    const float* entity, uint32_t k, const uint8_t* entity_on, const uint32_t* sig,
                                                    uint32_t sig_len, const uint8_t* sketch_on, uint32_t sketch_dim, float alpha_e,
                                                    float alpha_m, float* out, uint32_t out_stride, uint32_t* out_dims) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    ComposeShape sh;
    YA_TRY(check_compose(ctx, dense, n, dim, weights, entity, k, entity_on, sig, sig_len, sketch_on, sketch_dim, out, out_stride, out_dims, &sh));
    if (n == 0) return YAMS_OK;
    HostStage hs(ctx);
    const size_t nn = static_cast<size_t>(n);
    FeatComposeArgs a{};
    a.dense = hs.up("feat_host_rows", dense, nn * dim); a.n = n; a.dim = dim;
    a.k = k; a.sig_len = sig_len; a.sketch_dim = sketch_dim;
    if (sh.entity) {      // a part that is off travels nowhere
        a.entity = hs.up("feat_host_entity", entity, nn * k);
        a.entity_on = hs.up("feat_host_entity_on", entity_on, nn);
    }
    if (sh.sketch) {
        a.sig = hs.up("feat_host_sig", sig, nn * sig_len);
        a.sketch_on = hs.up("feat_host_sketch_on", sketch_on, nn);
    }
    a.alpha_e = alpha_e; a.alpha_m = alpha_m;
    a.out = hs.room<float>("feat_host_out", nn * out_stride); a.out_stride = out_stride;
    a.out_dims = hs.room<uint32_t>("feat_host_counts", nn);
    YA_TRY(hs.status());
    YA_TRY(run_compose(ctx, sh, a));
    hs.down(out, a.out, nn * out_stride);
    hs.down(out_dims, a.out_dims, nn);
    return hs.finish();
}
