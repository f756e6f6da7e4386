// sgc_api.cpp — yams_graph_sgc_smooth_device / _host: the degree pass and the hop loop of applySGCSmoothing
// (src/topology/topology_sgc.cpp:114-161 of the reference) behind the C ABI.
//
//   offsets, columns, weights, rows checked + degrees -> ONE read-back (flags, nnz, hub rows, maximum degree) -> the edge
//   scales -> `hops` hop launches over ping-pong buffers, the last of which writes `out` -> the zero-scale count read back
//   with the final synchronisation.  Nothing is written to `out` before the refusals are known.
#include <cstring>

#include "accel_ctx.h"
#include "arg_checks.h"
#include "host_stage.h"
#include "sgc_launch.h"

using namespace yams_accel;

namespace {

constexpr uint64_t kMaxRows = 1ull << 31;

// The argument checks both entries share (no device needed).  *done: the call is complete (n == 0).
yams_status_t check_args(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint64_t* row_offsets, const float* out,
                         bool* done) {
    *done = false;
    if (n >= kMaxRows) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n must be < 2^31");
    if (dim > YAMS_SGC_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_SGC_MAX_DIM");
    if (n == 0) { *done = true; return YAMS_OK; }
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (!rows || !out || !row_offsets) return fail(ctx, YAMS_ERR_INVALID_ARG, "null rows, out or row_offsets");
    const size_t bytes = static_cast<size_t>(n) * dim * 4;
    if (overlaps(rows, bytes, out, bytes)) return fail(ctx, YAMS_ERR_INVALID_ARG, "out overlaps rows");
    return YAMS_OK;
}

} // namespace

extern "C" yams_status_t yams_graph_sgc_smooth_device(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                      const uint64_t* row_offsets, const uint32_t* cols, const float* weights,
                                                      uint32_t hops, float* out, yams_sgc_diag_t* out_diag) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (out_diag) std::memset(out_diag, 0, sizeof *out_diag);
    bool done;
    YA_TRY(check_args(ctx, rows, n, dim, row_offsets, out, &done));
    if (done) return YAMS_OK;
    if (sgc_hop_blocks(n, dim) > 0x7fffffffull) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n * dim exceeds the launch limit");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const size_t row_bytes = static_cast<size_t>(n) * dim * 4;
    if (hops == 0) {      // :25 nothing changes
        YA_HIP(ctx, hipMemcpyAsync(out, rows, row_bytes, hipMemcpyDeviceToDevice, st));
        YA_HIP(ctx, hipStreamSynchronize(st));
        return YAMS_OK;
    }

    double* d_inv; uint32_t* d_hubs; uint32_t* d_small; uint32_t h_small[8];
    YA_TRY(ws_get(ctx, "sgc_inv", static_cast<size_t>(n) * 8, (void**)&d_inv));
    YA_TRY(ws_get(ctx, "sgc_hub_rows", static_cast<size_t>(n) * 4, (void**)&d_hubs));
    YA_TRY(flags_get(ctx, 8, &d_small));      // [0] flags [1] hub rows [2..3] nnz [4] max degree [6..7] zero-scale edges
    {
        TimedRegion tr(ctx, "sgc_check");
        YA_HIP(ctx, launch_sgc_check(st, rows, n, dim, row_offsets, cols, weights, d_inv, d_hubs, d_small));
        tr.end();
    }
    YA_TRY(read_words(ctx, d_small, 8, h_small));
    const uint32_t flags = h_small[0], n_hubs = h_small[1], max_degree = h_small[4];
    uint64_t nnz;
    std::memcpy(&nnz, h_small + 2, 8);
    if (flags & 1u) return fail(ctx, YAMS_ERR_INVALID_ARG, "row_offsets does not start at 0 or decreases");
    if (flags & 16u) return fail(ctx, YAMS_ERR_UNSUPPORTED, "nnz must be < 2^32");
    if (flags & 2u) return fail(ctx, YAMS_ERR_INVALID_ARG, "a column is out of range (or cols / weights is null)");
    if (flags & 4u) return fail(ctx, YAMS_ERR_INVALID_ARG, "a weight is negative or not finite");
    if (flags & 8u) return fail(ctx, YAMS_ERR_INVALID_ARG, "rows holds a non-finite value");

    double* d_scale; float* d_tmp = nullptr;
    YA_TRY(ws_get(ctx, "sgc_scale", static_cast<size_t>(nnz ? nnz : 1) * 8, (void**)&d_scale));
    if (hops >= 2) YA_TRY(ws_get(ctx, "sgc_pong", row_bytes, (void**)&d_tmp));
    {
        TimedRegion tr(ctx, "sgc_scale");
        YA_HIP(ctx, launch_sgc_scale(st, n, row_offsets, cols, weights, d_inv, d_scale, d_small));
        tr.end();
    }
    const bool vec = sgc_vec_loads(dim, rows, out, d_tmp);
    {
        TimedRegion tr(ctx, "sgc_hops");
        const float* src = rows;
        for (uint32_t h = 0; h < hops; ++h) {      // the last hop writes out: hop h writes out when hops - 1 - h is even
            float* dst = ((hops - 1 - h) & 1u) ? d_tmp : out;
            YA_HIP(ctx, launch_sgc_hop(st, src, dst, n, dim, row_offsets, cols, d_scale, d_inv, d_hubs, n_hubs, vec));
            src = dst;
        }
        tr.end();
    }
    YA_TRY(read_words(ctx, d_small, 8, h_small));
    if (out_diag) {
        out_diag->nnz = nnz;
        std::memcpy(&out_diag->edges_skipped_zero_scale, h_small + 6, 8);
        out_diag->max_degree = max_degree;
        out_diag->hops = hops;
        out_diag->hub_rows = n_hubs;
    }
    return YAMS_OK;
}

extern "C" yams_status_t yams_graph_sgc_smooth_host(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                    const uint64_t* row_offsets, const uint32_t* cols, const float* weights, uint32_t hops,
                                                    float* out, yams_sgc_diag_t* out_diag) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (out_diag) std::memset(out_diag, 0, sizeof *out_diag);
    bool done;
    YA_TRY(check_args(ctx, rows, n, dim, row_offsets, out, &done));
    if (done) return YAMS_OK;
    const size_t row_bytes = static_cast<size_t>(n) * dim * 4;
    if (hops == 0) {
        std::memcpy(out, rows, row_bytes);
        return YAMS_OK;
    }
    // the offsets size the uploads: they are judged here first
    if (!offsets_ascend(row_offsets, n)) return fail(ctx, YAMS_ERR_INVALID_ARG, "row_offsets does not start at 0 or decreases");
    const uint64_t nnz = row_offsets[n];
    if (nnz >= (1ull << 32)) return fail(ctx, YAMS_ERR_UNSUPPORTED, "nnz must be < 2^32");
    if (nnz && (!cols || !weights)) return fail(ctx, YAMS_ERR_INVALID_ARG, "null cols or weights");
    HostStage hs(ctx);
    const size_t cells = static_cast<size_t>(n) * dim;
    const float* d_rows = hs.up("sgc_host_rows", rows, cells);
    const uint64_t* d_off = hs.up("sgc_host_offsets", row_offsets, static_cast<size_t>(n) + 1);
    const uint32_t* d_cols = hs.up("sgc_host_cols", cols, static_cast<size_t>(nnz));
    const float* d_w = hs.up("sgc_host_weights", weights, static_cast<size_t>(nnz));
    float* d_out = hs.room<float>("sgc_host_out", cells);
    YA_TRY(hs.status());
    YA_TRY(yams_graph_sgc_smooth_device(ctx, d_rows, n, dim, d_off, d_cols, d_w, hops, d_out, out_diag));
    hs.down(out, d_out, cells);
    return hs.finish();
}
