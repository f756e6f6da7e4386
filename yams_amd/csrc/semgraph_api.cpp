// semgraph_api.cpp — yams_graph_semantic_neighbors_device / _host: the pair loop of
// EmbeddingService::updateSemanticNeighborGraphUnlocked (src/daemon/components/EmbeddingService.cpp:612-648, :856-1076)
// behind the C ABI.
//
//   inverse norms (+ the refusal flags: non-finite rows, source indices, tie ranks) -> ONE 4-byte read-back -> the pairs
//   kernel over (source tiles x candidate stripes) -> the merge of the stripes' lists -> counts read back with the final
//   synchronisation.  Nothing is written to an output before the refusals are known.
#include <cmath>
#include <cstring>

#include "accel_ctx.h"
#include "host_stage.h"
#include "semgraph_launch.h"

using namespace yams_accel;

namespace {

constexpr uint64_t kMaxRows = 1ull << 31;

// The argument checks both entries share (no device needed).  *done: the call is complete (an empty result).
// *sources = the number of sources.
yams_status_t check_args(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint32_t* source_rows,
                         uint64_t n_sources, uint32_t k, uint32_t flags, float threshold, const uint32_t* out_rows, const float* out_sims,
                         const uint32_t* out_counts, uint64_t* sources, bool* done) {
    *done = false;
    *sources = source_rows ? n_sources : n;
    if (flags & ~YAMS_GRAPH_FLAG_EXPLICIT_THRESHOLD) return fail(ctx, YAMS_ERR_INVALID_ARG, "unknown flag");
    if ((flags & YAMS_GRAPH_FLAG_EXPLICIT_THRESHOLD) && !std::isfinite(threshold))
        return fail(ctx, YAMS_ERR_INVALID_ARG, "the explicit threshold is not finite");
    if (n >= kMaxRows || *sources >= kMaxRows) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n and n_sources must be < 2^31");
    if (dim > YAMS_GRAPH_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_GRAPH_MAX_DIM");
    if (k > YAMS_GRAPH_MAX_K) return fail(ctx, YAMS_ERR_UNSUPPORTED, "k exceeds YAMS_GRAPH_MAX_K");
    if (k == 0 || n < 2 || *sources == 0) { *done = true; return YAMS_OK; }      // :890
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (!rows) return fail(ctx, YAMS_ERR_INVALID_ARG, "null rows");
    if (!out_rows || !out_sims || !out_counts) return fail(ctx, YAMS_ERR_INVALID_ARG, "null output");
    return YAMS_OK;
}

} // namespace

extern "C" yams_status_t yams_graph_semantic_neighbors_device(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                              const uint32_t* tie_rank, const uint32_t* source_rows, uint64_t n_sources,
                                                              uint32_t k, uint32_t flags, float threshold, uint32_t* out_rows,
                                                              float* out_sims, uint32_t* out_counts, float* out_inv_norm,
                                                              yams_graph_diag_t* out_diag) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (out_diag) std::memset(out_diag, 0, sizeof *out_diag);
    uint64_t S;
    bool done;
    YA_TRY(check_args(ctx, rows, n, dim, source_rows, n_sources, k, flags, threshold, out_rows, out_sims, out_counts, &S, &done));
    if (done) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;

    uint32_t source_tiles, stripes, tiles_per_stripe;
    semgraph_geometry(n, S, &source_tiles, &stripes, &tiles_per_stripe);
    float* d_inv; uint32_t* d_small; uint32_t* d_ror = nullptr; uint64_t* d_part; uint32_t h_small[8];
    YA_TRY(ws_get(ctx, "sg_inv_norm", static_cast<size_t>(n) * 4, (void**)&d_inv));
    YA_TRY(flags_get(ctx, 8, &d_small));              // [0] refusal flags, [2..5] the two 64-bit counts
    if (tie_rank) YA_TRY(ws_get(ctx, "sg_row_of_rank", static_cast<size_t>(n) * 4, (void**)&d_ror));
    YA_TRY(ws_get(ctx, "sg_part", static_cast<size_t>(S) * stripes * k * 8, (void**)&d_part));
    auto* d_counts = reinterpret_cast<unsigned long long*>(d_small + 2);

    {
        TimedRegion tr(ctx, "semgraph_norm");
        YA_HIP(ctx, launch_semgraph_norm(st, rows, n, dim, d_inv, d_small));
        YA_HIP(ctx, launch_semgraph_check(st, n, tie_rank, source_rows, S, d_ror, d_small));
        tr.end();
    }
    YA_TRY(read_words(ctx, d_small, 1, h_small));
    if (h_small[0] & 1u) return fail(ctx, YAMS_ERR_INVALID_ARG, "a row holds a non-finite value or has an infinite inverse norm");
    if (h_small[0] & 2u) return fail(ctx, YAMS_ERR_INVALID_ARG, "a source index is out of range");
    if (h_small[0] & 4u) return fail(ctx, YAMS_ERR_INVALID_ARG, "tie_rank is not a permutation of [0, n)");
    {
        TimedRegion tr(ctx, "semgraph_pairs");
        YA_HIP(ctx, launch_semgraph_pairs(st, rows, n, dim, d_inv, tie_rank, source_rows, S, k, (flags & YAMS_GRAPH_FLAG_EXPLICIT_THRESHOLD) != 0,
                                          threshold, source_tiles, stripes, tiles_per_stripe, d_part, d_counts));
        tr.end();
    }
    {
        TimedRegion tr(ctx, "semgraph_merge");
        YA_HIP(ctx, launch_semgraph_merge(st, d_part, stripes, k, S, rows, dim, d_inv, source_rows, d_ror, out_rows, out_sims, out_counts));
        tr.end();
    }
    if (out_inv_norm) YA_HIP(ctx, hipMemcpyAsync(out_inv_norm, d_inv, static_cast<size_t>(n) * 4, hipMemcpyDeviceToDevice, st));
    YA_TRY(read_words(ctx, d_small, 8, h_small));
    if (out_diag) {
        out_diag->stripes = stripes;
        out_diag->source_tiles = source_tiles;
        std::memcpy(&out_diag->pairs_scored, h_small + 2, 8);
        std::memcpy(&out_diag->pairs_admitted, h_small + 4, 8);
    }
    return YAMS_OK;
}

extern "C" yams_status_t yams_graph_semantic_neighbors_host(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                            const uint32_t* tie_rank, const uint32_t* source_rows, uint64_t n_sources,
                                                            uint32_t k, uint32_t flags, float threshold, uint32_t* out_rows, float* out_sims,
                                                            uint32_t* out_counts, float* out_inv_norm, yams_graph_diag_t* out_diag) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (out_diag) std::memset(out_diag, 0, sizeof *out_diag);
    uint64_t S;
    bool done;
    YA_TRY(check_args(ctx, rows, n, dim, source_rows, n_sources, k, flags, threshold, out_rows, out_sims, out_counts, &S, &done));
    if (done) return YAMS_OK;
    HostStage hs(ctx);
    const size_t nn = static_cast<size_t>(n), ns = static_cast<size_t>(S), slots = ns * k;
    const float* d_rows = hs.up("sg_host_rows", rows, nn * dim);
    const uint32_t* d_tie = hs.up("sg_host_tie", tie_rank, nn);
    const uint32_t* d_src = hs.up("sg_host_sources", source_rows, ns);
    uint32_t* d_or = hs.room<uint32_t>("sg_host_out_rows", slots);
    float* d_os = hs.room<float>("sg_host_out_sims", slots);
    uint32_t* d_oc = hs.room<uint32_t>("sg_host_out_counts", ns);
    float* d_oi = out_inv_norm ? hs.room<float>("sg_host_out_inv", nn) : nullptr;
    YA_TRY(hs.status());
    YA_TRY(yams_graph_semantic_neighbors_device(ctx, d_rows, n, dim, d_tie, d_src, S, k, flags, threshold, d_or, d_os, d_oc, d_oi, out_diag));
    hs.down(out_rows, d_or, slots);
    hs.down(out_sims, d_os, slots);
    hs.down(out_counts, d_oc, ns);
    hs.down(out_inv_norm, d_oi, nn);
    return hs.finish();
}
