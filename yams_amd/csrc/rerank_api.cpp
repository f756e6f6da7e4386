// rerank_api.cpp — yams_rerank_maxsim / yams_rerank_maxpool (_device and _host): OnnxColbertSession's computeMaxSim over a
// window of candidate documents, and maxPoolEmbeddings + normalizeEmbedding, behind the C ABI.  Every entry: the limits (no
// device needed) -> argument checks -> the pool's total read back -> ONE read-back of the check flags (the offsets' verdict) ->
// what the total sizes (the row limit, the overlaps) -> the work.  Nothing is written to an output before every refusal is known.
#include <cstdlib>
#include <cstring>

#include "accel_ctx.h"
#include "arg_checks.h"
#include "host_stage.h"
#include "rerank_launch.h"

using namespace yams_accel;

namespace {

static_assert(YAMS_RERANK_MAX_DIM == kRerankMaxDim && YAMS_RERANK_MAX_DOC_TOKENS == kRerankMaxDocTokens &&
                  YAMS_RERANK_MAX_QUERY_TOKENS == kRerankMaxQueryTokens && YAMS_RERANK_MAX_ROWS == kRerankMaxRows &&
                  YAMS_RERANK_MAX_DOCS == kRerankMaxDocs && YAMS_RERANK_MAX_ROWMAX == kRerankMaxRowMax,
              "the header's limits are the launchers'");
static_assert(YAMS_RERANK_PATH_VALU == kRerankValu && YAMS_RERANK_PATH_MFMA == kRerankMfma, "the diag's path is the launcher's");

RerankPath fused_path() {
#ifdef YAMS_ACCEL_MEASURE
    if (const char* e = std::getenv("YAMS_ACCEL_RERANK_FUSED_PATH")) return std::strcmp(e, "valu") == 0 ? kRerankValu : kRerankMfma;
#endif
    return kRerankFusedPath;
}

// what needs no device
yams_status_t check_maxsim(yams_accel_ctx* ctx, const float* query, uint32_t tq, uint32_t dim, const uint64_t* doc_offsets, uint64_t n_docs,
                           uint32_t form, const float* out_scores) {
    if (dim > YAMS_RERANK_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_RERANK_MAX_DIM");
    if (tq > YAMS_RERANK_MAX_QUERY_TOKENS) return fail(ctx, YAMS_ERR_UNSUPPORTED, "the query exceeds YAMS_RERANK_MAX_QUERY_TOKENS");
    if (n_docs > YAMS_RERANK_MAX_DOCS) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n_docs exceeds YAMS_RERANK_MAX_DOCS");
    if (n_docs * tq > YAMS_RERANK_MAX_ROWMAX) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n_docs * query tokens exceeds YAMS_RERANK_MAX_ROWMAX");
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (form != YAMS_RESIDUAL_SEPARATE && form != YAMS_RESIDUAL_FUSED) return fail(ctx, YAMS_ERR_INVALID_ARG, "unknown form");
    if (n_docs && (!doc_offsets || !out_scores)) return fail(ctx, YAMS_ERR_INVALID_ARG, "null doc_offsets or out_scores");
    if (n_docs && tq && !query) return fail(ctx, YAMS_ERR_INVALID_ARG, "null query");
    return YAMS_OK;
}
// once the pool's total is known
yams_status_t check_maxsim_total(yams_accel_ctx* ctx, const float* query, uint32_t tq, uint32_t dim, const float* rows, uint64_t total,
                                 uint64_t n_docs, const float* out_scores, const float* out_rowmax) {
    if (total > YAMS_RERANK_MAX_ROWS) return fail(ctx, YAMS_ERR_UNSUPPORTED, "the row pool exceeds YAMS_RERANK_MAX_ROWS");
    if (total && !rows) return fail(ctx, YAMS_ERR_INVALID_ARG, "null rows");
    const size_t rb = static_cast<size_t>(total) * dim * 4, qb = static_cast<size_t>(tq) * dim * 4, sb = static_cast<size_t>(n_docs) * 4,
                 mb = static_cast<size_t>(n_docs) * tq * 4;
    if (overlaps(out_scores, sb, rows, rb) || overlaps(out_scores, sb, query, qb) || overlaps(out_rowmax, mb, rows, rb) ||
        overlaps(out_rowmax, mb, query, qb) || overlaps(out_scores, sb, out_rowmax, mb))
        return fail(ctx, YAMS_ERR_INVALID_ARG, "an output overlaps an input or the other output");
    return YAMS_OK;
}

yams_status_t check_maxpool(yams_accel_ctx* ctx, uint32_t dim, const uint64_t* doc_offsets, uint64_t n_docs, const float* out) {
    if (dim > YAMS_RERANK_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_RERANK_MAX_DIM");
    if (n_docs > YAMS_RERANK_MAX_DOCS) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n_docs exceeds YAMS_RERANK_MAX_DOCS");
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (n_docs && (!doc_offsets || !out)) return fail(ctx, YAMS_ERR_INVALID_ARG, "null doc_offsets or out");
    return YAMS_OK;
}
yams_status_t check_maxpool_total(yams_accel_ctx* ctx, uint32_t dim, const float* rows, uint64_t total, uint64_t n_docs, const float* out) {
    if (total > YAMS_RERANK_MAX_ROWS) return fail(ctx, YAMS_ERR_UNSUPPORTED, "the row pool exceeds YAMS_RERANK_MAX_ROWS");
    if (total && !rows) return fail(ctx, YAMS_ERR_INVALID_ARG, "null rows");
    if (overlaps(out, static_cast<size_t>(n_docs) * dim * 4, rows, static_cast<size_t>(total) * dim * 4))
        return fail(ctx, YAMS_ERR_INVALID_ARG, "out overlaps rows");
    return YAMS_OK;
}

// The offsets as the host sees them.  A document too long in front of the first decrease is refused as such (the offsets
// are judged list by list); every other defect of the offsets is the shared verdict's.
yams_status_t check_offsets_host(yams_accel_ctx* ctx, const uint64_t* off, uint64_t n_docs) {
    for (uint64_t i = 0; off[0] == 0 && i < n_docs && off[i + 1] >= off[i]; ++i)
        if (off[i + 1] - off[i] > YAMS_RERANK_MAX_DOC_TOKENS) return fail(ctx, YAMS_ERR_UNSUPPORTED, "a document exceeds YAMS_RERANK_MAX_DOC_TOKENS");
    if (!offsets_ascend(off, n_docs)) return fail(ctx, YAMS_ERR_INVALID_ARG, "the offsets do not start at 0 or decrease");
    return YAMS_OK;
}

// The offsets' checks over device offsets (total: their last).  Synchronises.
yams_status_t device_check(yams_accel_ctx* ctx, const uint64_t* d_off, uint64_t n_docs, uint64_t total) {
    uint32_t* d_flags; uint32_t flags;
    YA_TRY(flags_get(ctx, 4, &d_flags));
    YA_HIP(ctx, launch_rerank_check(ctx->stream, d_off, n_docs, total, YAMS_RERANK_MAX_DOC_TOKENS, d_flags));
    YA_TRY(read_words(ctx, d_flags, 1, &flags));
    if (flags & 1u) return fail(ctx, YAMS_ERR_INVALID_ARG, "the offsets do not start at 0 or decrease");
    if (flags & 2u) return fail(ctx, YAMS_ERR_UNSUPPORTED, "a document exceeds YAMS_RERANK_MAX_DOC_TOKENS");
    return YAMS_OK;
}

} // namespace

// ---- MaxSim ------------------------------------------------------------------------------------------------------------------
extern "C" yams_status_t yams_rerank_maxsim_device(yams_accel_ctx* ctx, const float* query, uint32_t tq, uint32_t dim, const float* rows,
                                                   const uint64_t* doc_offsets, uint64_t n_docs, uint32_t form, float* out_scores,
                                                   float* out_rowmax, uint32_t* out_rowarg, yams_rerank_diag_t* diag) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_maxsim(ctx, query, tq, dim, doc_offsets, n_docs, form, out_scores));
    if (n_docs == 0) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    uint64_t total;
    YA_TRY(read_words(ctx, doc_offsets + n_docs, 2, &total));
    YA_TRY(device_check(ctx, doc_offsets, n_docs, total));      // the offsets first, as the host twin judges them: what they claim sizes the overlap test
    YA_TRY(check_maxsim_total(ctx, query, tq, dim, rows, total, n_docs, out_scores, out_rowmax));
    const bool fused = form == YAMS_RESIDUAL_FUSED;
    const RerankPath path = fused ? fused_path() : kRerankValu;
    float* d_rowmax = out_rowmax;
    if (!d_rowmax && tq) YA_TRY(ws_get(ctx, "rerank_rowmax", static_cast<size_t>(n_docs) * tq * 4, (void**)&d_rowmax));
    {
        TimedRegion tr(ctx, "rerank_maxsim");
        hipError_t e = launch_rerank_rowmax(st, query, tq, dim, rows, doc_offsets, static_cast<uint32_t>(n_docs), fused, path, d_rowmax,
                                            out_rowmax ? out_rowarg : nullptr);
        if (e == hipSuccess) e = launch_rerank_score(st, d_rowmax, tq, static_cast<uint32_t>(n_docs), out_scores);
        tr.end();
        YA_HIP(ctx, e);
    }
    YA_HIP(ctx, hipStreamSynchronize(st));
    if (diag) {
        diag->path = path;
        diag->form = form;
        diag->rows = total;
        diag->docs = n_docs;
        diag->query_tokens = tq;
        diag->reserved = 0;
    }
    return YAMS_OK;
}

extern "C" yams_status_t yams_rerank_maxsim_host(yams_accel_ctx* ctx, const float* query, uint32_t tq, uint32_t dim, const float* rows,
                                                 const uint64_t* doc_offsets, uint64_t n_docs, uint32_t form, float* out_scores,
                                                 float* out_rowmax, uint32_t* out_rowarg, yams_rerank_diag_t* diag) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_maxsim(ctx, query, tq, dim, doc_offsets, n_docs, form, out_scores));
    if (n_docs == 0) return YAMS_OK;
    YA_TRY(check_offsets_host(ctx, doc_offsets, n_docs));      // judged here, before an upload is sized by them
    const uint64_t total = doc_offsets[n_docs];
    YA_TRY(check_maxsim_total(ctx, query, tq, dim, rows, total, n_docs, out_scores, out_rowmax));
    HostStage hs(ctx);
    const size_t nd = static_cast<size_t>(n_docs), cells = nd * tq;
    const bool want_max = out_rowmax && cells, want_arg = want_max && out_rowarg;
    const float* d_q = hs.up("rerank_host_query", query, static_cast<size_t>(tq) * dim);
    const float* d_rows = hs.up("rerank_host_rows", rows, static_cast<size_t>(total) * dim);
    const uint64_t* d_off = hs.up("rerank_host_offsets", doc_offsets, nd + 1);
    float* d_scores = hs.room<float>("rerank_host_scores", nd);
    float* d_max = want_max ? hs.room<float>("rerank_host_rowmax", cells) : nullptr;
    uint32_t* d_arg = want_arg ? hs.room<uint32_t>("rerank_host_rowarg", cells) : nullptr;
    YA_TRY(hs.status());
    yams_rerank_diag_t dg{};
    YA_TRY(yams_rerank_maxsim_device(ctx, d_q, tq, dim, d_rows, d_off, n_docs, form, d_scores, d_max, d_arg, &dg));
    hs.down(out_scores, d_scores, nd);
    if (want_max) hs.down(out_rowmax, d_max, cells);
    if (want_arg) hs.down(out_rowarg, d_arg, cells);
    YA_TRY(hs.finish());
    if (diag) *diag = dg;
    return YAMS_OK;
}

// ---- max-pool + L2 normalisation ---------------------------------------------------------------------------------------------
extern "C" yams_status_t yams_rerank_maxpool_device(yams_accel_ctx* ctx, const float* rows, uint32_t dim, const uint64_t* doc_offsets,
                                                    uint64_t n_docs, float* out) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_maxpool(ctx, dim, doc_offsets, n_docs, out));
    if (n_docs == 0) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    uint64_t total;
    YA_TRY(read_words(ctx, doc_offsets + n_docs, 2, &total));
    YA_TRY(device_check(ctx, doc_offsets, n_docs, total));
    YA_TRY(check_maxpool_total(ctx, dim, rows, total, n_docs, out));
    {
        TimedRegion tr(ctx, "rerank_maxpool");
        YA_HIP(ctx, launch_rerank_maxpool(st, rows, dim, doc_offsets, static_cast<uint32_t>(n_docs), out));
        tr.end();
    }
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

extern "C" yams_status_t yams_rerank_maxpool_host(yams_accel_ctx* ctx, const float* rows, uint32_t dim, const uint64_t* doc_offsets,
                                                  uint64_t n_docs, float* out) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_maxpool(ctx, dim, doc_offsets, n_docs, out));
    if (n_docs == 0) return YAMS_OK;
    YA_TRY(check_offsets_host(ctx, doc_offsets, n_docs));
    const uint64_t total = doc_offsets[n_docs];
    YA_TRY(check_maxpool_total(ctx, dim, rows, total, n_docs, out));
    HostStage hs(ctx);
    const size_t nd = static_cast<size_t>(n_docs);
    const float* d_rows = hs.up("rerank_host_rows", rows, static_cast<size_t>(total) * dim);
    const uint64_t* d_off = hs.up("rerank_host_offsets", doc_offsets, nd + 1);
    float* d_out = hs.room<float>("rerank_host_pooled", nd * dim);
    YA_TRY(hs.status());
    YA_TRY(yams_rerank_maxpool_device(ctx, d_rows, dim, d_off, n_docs, d_out));
    hs.down(out, d_out, nd * dim);
    return hs.finish();
}
