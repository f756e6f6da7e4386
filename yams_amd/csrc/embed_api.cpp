// embed_api.cpp — yams_embed_pool / yams_embed_normalize (_device and _host): the pooling head of the embedding sessions
// (CLS, max or mean over the tokens of each text, then the L2 normalisation) behind the C ABI.  Every entry: the limits (no
// device needed) -> argument checks -> ONE read-back of the check kernel's words (the MEAN refusal and the count of active
// tokens) -> the work.  Nothing is written to an output before every refusal is known.
#include "accel_ctx.h"
#include "arg_checks.h"
#include "embed_launch.h"
#include "host_stage.h"

using namespace yams_accel;

namespace {

static_assert(YAMS_EMBED_MAX_DIM == kEmbedMaxDim && YAMS_EMBED_MAX_SEQ == kEmbedMaxSeq && YAMS_EMBED_MAX_ROWS == kEmbedMaxRows,
              "the header's limits are the launchers'");
static_assert(YAMS_EMBED_POOL_CLS == kEmbedCls && YAMS_EMBED_POOL_MAX == kEmbedMax && YAMS_EMBED_POOL_MEAN == kEmbedMean,
              "the header's modes are the launchers'");

uint32_t considered(uint32_t seq, uint32_t mask_len) { return seq < mask_len ? seq : mask_len; }

// what needs no device
yams_status_t check_pool(yams_accel_ctx* ctx, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask,
                         uint32_t mask_len, uint32_t mode, uint32_t flags, const float* out) {
    if (dim > YAMS_EMBED_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_EMBED_MAX_DIM");
    if (seq > YAMS_EMBED_MAX_SEQ) return fail(ctx, YAMS_ERR_UNSUPPORTED, "seq exceeds YAMS_EMBED_MAX_SEQ");
    if (batch > YAMS_EMBED_MAX_ROWS || batch * seq > YAMS_EMBED_MAX_ROWS) return fail(ctx, YAMS_ERR_UNSUPPORTED, "batch * seq exceeds YAMS_EMBED_MAX_ROWS");
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (seq == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "seq == 0");
    if (mode != YAMS_EMBED_POOL_CLS && mode != YAMS_EMBED_POOL_MAX && mode != YAMS_EMBED_POOL_MEAN) return fail(ctx, YAMS_ERR_INVALID_ARG, "unknown mode");
    if (flags & ~YAMS_EMBED_NORMALIZE) return fail(ctx, YAMS_ERR_INVALID_ARG, "unknown flag bit");
    if (batch == 0) return YAMS_OK;
    if (!hidden || !out) return fail(ctx, YAMS_ERR_INVALID_ARG, "null hidden or out");
    if (!mask && mode != YAMS_EMBED_POOL_CLS && mask_len) return fail(ctx, YAMS_ERR_INVALID_ARG, "null mask");
    const size_t ob = static_cast<size_t>(batch) * dim * 4;
    if (overlaps(out, ob, hidden, static_cast<size_t>(batch) * seq * dim * 4) || (mask && overlaps(out, ob, mask, static_cast<size_t>(batch) * mask_len * 4)))
        return fail(ctx, YAMS_ERR_INVALID_ARG, "out overlaps an input");
    return YAMS_OK;
}

yams_status_t check_normalize(yams_accel_ctx* ctx, const float* rows, uint64_t batch, uint32_t dim, const float* out) {
    if (dim > YAMS_EMBED_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_EMBED_MAX_DIM");
    if (batch > YAMS_EMBED_MAX_ROWS) return fail(ctx, YAMS_ERR_UNSUPPORTED, "batch exceeds YAMS_EMBED_MAX_ROWS");
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (batch == 0) return YAMS_OK;
    if (!rows || !out) return fail(ctx, YAMS_ERR_INVALID_ARG, "null rows or out");
    const size_t rb = static_cast<size_t>(batch) * dim * 4;
    if (overlaps(out, rb, rows, rb)) return fail(ctx, YAMS_ERR_INVALID_ARG, "out overlaps rows");
    return YAMS_OK;
}

// the MEAN refusal as the host sees it, before an upload
yams_status_t check_mask_host(yams_accel_ctx* ctx, const int32_t* mask, uint64_t batch, uint32_t mask_len, uint32_t t_len) {
    for (uint64_t b = 0; b < batch; ++b)
        for (uint32_t i = 0; i < t_len; ++i)
            if (mask[b * mask_len + i] > 1) return fail(ctx, YAMS_ERR_UNSUPPORTED, "a MEAN mask value above 1");
    return YAMS_OK;
}

} // namespace

extern "C" yams_status_t yams_embed_pool_device(yams_accel_ctx* ctx, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim,
                                                const int32_t* mask, uint32_t mask_len, uint32_t mode, uint32_t flags, float* out,
                                                yams_embed_diag_t* diag) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_pool(ctx, hidden, batch, seq, dim, mask, mask_len, mode, flags, out));
    if (batch == 0) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    if (mode == YAMS_EMBED_POOL_CLS) mask = nullptr;      // CLS never reads the mask
    const uint32_t t_len = mask ? considered(seq, mask_len) : 0u;
    uint32_t words[2] = {0u, 0u};
    if (t_len) {
        uint32_t* d_flags;
        YA_TRY(flags_get(ctx, 4, &d_flags));
        YA_HIP(ctx, launch_embed_check(st, mask, batch, mask_len, t_len, mode == YAMS_EMBED_POOL_MEAN, d_flags));
        YA_TRY(read_words(ctx, d_flags, 2, words));
        if (words[0] & 1u) return fail(ctx, YAMS_ERR_UNSUPPORTED, "a MEAN mask value above 1");
    }
    const uint32_t slab = embed_slab_dims(batch, dim, embed_vec4(hidden, out, dim));
    const bool mean = mode == YAMS_EMBED_POOL_MEAN, normalize = (flags & YAMS_EMBED_NORMALIZE) != 0;
    uint32_t* d_counts = nullptr;
    if (mean) YA_TRY(ws_get(ctx, "embed_counts", static_cast<size_t>(batch) * 4, (void**)&d_counts));
    {
        TimedRegion tr(ctx, "embed_pool");
        hipError_t e = launch_embed_pool(st, hidden, batch, seq, dim, mask, mask_len, t_len, static_cast<EmbedMode>(mode), slab, out, d_counts);
        if (e == hipSuccess && (mean || normalize)) e = launch_embed_finish(st, out, batch, dim, d_counts, normalize, out);
        tr.end();
        YA_HIP(ctx, e);
    }
    YA_HIP(ctx, hipStreamSynchronize(st));
    if (diag) {
        diag->mode = mode;
        diag->flags = flags;
        diag->batch = batch;
        diag->seq = seq;
        diag->dim = dim;
        diag->tokens_considered = batch * t_len;
        diag->active_tokens = words[1];
        diag->slab_dims = slab;
        diag->reserved = 0;
    }
    return YAMS_OK;
}

extern "C" yams_status_t yams_embed_pool_host(yams_accel_ctx* ctx, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim,
                                              const int32_t* mask, uint32_t mask_len, uint32_t mode, uint32_t flags, float* out,
                                              yams_embed_diag_t* diag) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_pool(ctx, hidden, batch, seq, dim, mask, mask_len, mode, flags, out));
    if (batch == 0) return YAMS_OK;
    if (mask && mode == YAMS_EMBED_POOL_MEAN) YA_TRY(check_mask_host(ctx, mask, batch, mask_len, considered(seq, mask_len)));      // before an upload
    HostStage hs(ctx);
    // CLS reads token 0 of every text and no mask: the copy is strided then
    const bool cls = mode == YAMS_EMBED_POOL_CLS;
    const uint32_t up_seq = cls ? 1u : seq;
    const size_t rows = static_cast<size_t>(batch), row = static_cast<size_t>(dim);
    const float* d_hidden;
    if (cls && seq > 1) {      // not a plain copy: the room is HostStage's, the 2D copy stays here
        float* d_cls = hs.room<float>("embed_host_hidden", rows * row);
        if (d_cls) YA_HIP(ctx, hipMemcpy2DAsync(d_cls, row * 4, hidden, seq * row * 4, row * 4, rows, hipMemcpyHostToDevice, ctx->stream));
        d_hidden = d_cls;
    } else {
        d_hidden = hs.up("embed_host_hidden", hidden, rows * up_seq * row);
    }
    // an empty mask (mask_len == 0) stays a NULL mask for the device twin, as a CLS call's does: a mask with an address is one
    // the pooling kernels consult
    const int32_t* d_mask = cls || !mask_len ? nullptr : hs.up("embed_host_mask", mask, rows * mask_len);
    float* d_out = hs.room<float>("embed_host_out", rows * row);
    YA_TRY(hs.status());
    yams_embed_diag_t dg{};
    YA_TRY(yams_embed_pool_device(ctx, d_hidden, batch, up_seq, dim, d_mask, mask_len, mode, flags, d_out, &dg));
    hs.down(out, d_out, rows * row);
    YA_TRY(hs.finish());
    if (diag) {
        dg.seq = seq;
        *diag = dg;
    }
    return YAMS_OK;
}

extern "C" yams_status_t yams_embed_normalize_device(yams_accel_ctx* ctx, const float* rows, uint64_t batch, uint32_t dim, float* out) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_normalize(ctx, rows, batch, dim, out));
    if (batch == 0) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    {
        TimedRegion tr(ctx, "embed_normalize");
        YA_HIP(ctx, launch_embed_finish(st, rows, batch, dim, nullptr, true, out));
        tr.end();
    }
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

extern "C" yams_status_t yams_embed_normalize_host(yams_accel_ctx* ctx, const float* rows, uint64_t batch, uint32_t dim, float* out) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_normalize(ctx, rows, batch, dim, out));
    if (batch == 0) return YAMS_OK;
    HostStage hs(ctx);
    const size_t count = static_cast<size_t>(batch) * dim;
    const float* d_rows = hs.up("embed_host_hidden", rows, count);
    float* d_out = hs.room<float>("embed_host_out", count);
    YA_TRY(hs.status());
    YA_TRY(yams_embed_normalize_device(ctx, d_rows, batch, dim, d_out));
    hs.down(out, d_out, count);
    return hs.finish();
}
