// artifact_api.cpp — yams_cluster_centroids / _representatives / _residuals (_device and _host): the tail every topology engine
// runs after clustering (meanEmbedding, selectDiverseRoutingRepresentatives, the chains of applyOrthogonalBoundarySpill) behind
// the C ABI.  Every entry: argument checks without the device -> the list totals read back -> the checks that need the arrays
// -> ONE read-back of the flags -> the work.  Nothing is written to an output before the refusals are known.
#include <algorithm>
#include <cstring>
#include <vector>

#include "accel_ctx.h"
#include "arg_checks.h"
#include "artifact_launch.h"
#include "host_stage.h"
#include "kmeans_launch.h"

using namespace yams_accel;

namespace {

constexpr uint64_t kMaxRows = 1ull << 31;
constexpr uint64_t kMaxEntries = 1ull << 32;
constexpr size_t kHostOutBytes = 256ull << 20;      // what a _host call's outputs may occupy on the device at a time

// The limits and the checks every entry shares (no device needed).
yams_status_t check_shape(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, uint32_t c) {
    if (n >= kMaxRows) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n must be < 2^31");
    if (dim > YAMS_CLUSTER_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_CLUSTER_MAX_DIM");
    if (c > YAMS_CLUSTER_MAX_K) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n_clusters exceeds YAMS_CLUSTER_MAX_K");
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (n && !rows) return fail(ctx, YAMS_ERR_INVALID_ARG, "null rows");
    return YAMS_OK;
}

// The list checks: offsets from 0, never decreasing, entries < limit.  Synchronises.
yams_status_t check_lists(yams_accel_ctx* ctx, const uint64_t* d_off, uint64_t lists, uint64_t total, const uint32_t* d_idx, uint32_t limit,
                          const uint32_t* d_primary, uint64_t n, uint32_t c, const char* what) {
    hipStream_t st = ctx->stream;
    uint32_t* d_flags; uint32_t flags;
    YA_TRY(flags_get(ctx, 4, &d_flags));
    if (d_off) YA_HIP(ctx, launch_artifact_check(st, d_off, lists, total, d_idx, limit, d_flags));
    if (d_primary) YA_HIP(ctx, launch_artifact_check_primary(st, d_primary, n, c, d_flags));
    YA_TRY(read_words(ctx, d_flags, 1, &flags));
    if (flags & 1u) return fail(ctx, YAMS_ERR_INVALID_ARG, std::string(what) + ": the offsets do not start at 0 or decrease");
    if (flags & 2u) return fail(ctx, YAMS_ERR_INVALID_ARG, std::string(what) + ": an index is out of range");
    return YAMS_OK;
}

} // namespace

// ---- centroids ------------------------------------------------------------------------------------------------------------
extern "C" yams_status_t yams_cluster_centroids_device(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                       const uint64_t* cluster_offsets, const uint32_t* members, uint32_t n_clusters,
                                                       float* out_centroids, uint32_t* out_counts) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_shape(ctx, rows, n, dim, n_clusters));
    if (n_clusters == 0) return YAMS_OK;
    if (!cluster_offsets || !out_centroids || !out_counts) return fail(ctx, YAMS_ERR_INVALID_ARG, "null cluster_offsets or output");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    uint64_t total;
    YA_TRY(read_words(ctx, cluster_offsets + n_clusters, 2, &total));
    if (total >= kMaxEntries) return fail(ctx, YAMS_ERR_UNSUPPORTED, "the lists must hold fewer than 2^32 entries");
    if (total && !members) return fail(ctx, YAMS_ERR_INVALID_ARG, "null members");
    YA_TRY(check_lists(ctx, cluster_offsets, n_clusters, total, members, static_cast<uint32_t>(n), nullptr, 0, 0, "members"));
    {
        TimedRegion tr(ctx, "artifact_centroids");
        YA_HIP(ctx, launch_artifact_centroids(st, rows, dim, cluster_offsets, members, n_clusters, out_centroids, out_counts));
        tr.end();
    }
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

extern "C" yams_status_t yams_cluster_centroids_host(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                     const uint64_t* cluster_offsets, const uint32_t* members, uint32_t n_clusters,
                                                     float* out_centroids, uint32_t* out_counts) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_shape(ctx, rows, n, dim, n_clusters));
    if (n_clusters == 0) return YAMS_OK;
    if (!cluster_offsets || !out_centroids || !out_counts) return fail(ctx, YAMS_ERR_INVALID_ARG, "null cluster_offsets or output");
    // judged here, before an upload is sized by them
    if (!offsets_ascend(cluster_offsets, n_clusters)) return fail(ctx, YAMS_ERR_INVALID_ARG, "the offsets do not start at 0 or decrease");
    const uint64_t total = cluster_offsets[n_clusters];
    if (total >= kMaxEntries) return fail(ctx, YAMS_ERR_UNSUPPORTED, "the lists must hold fewer than 2^32 entries");
    if (total && !members) return fail(ctx, YAMS_ERR_INVALID_ARG, "null members");
    HostStage hs(ctx);
    const size_t c = n_clusters;
    const float* d_rows = hs.up("art_host_rows", rows, static_cast<size_t>(n) * dim);
    const uint64_t* d_off = hs.up("art_host_offsets", cluster_offsets, c + 1);
    const uint32_t* d_mem = hs.up("art_host_list", members, static_cast<size_t>(total));
    float* d_cent = hs.room<float>("art_host_centroids", c * dim);
    uint32_t* d_cnt = hs.room<uint32_t>("art_host_counts", c);
    YA_TRY(hs.status());
    YA_TRY(yams_cluster_centroids_device(ctx, d_rows, n, dim, d_off, d_mem, n_clusters, d_cent, d_cnt));
    hs.down(out_centroids, d_cent, c * dim);
    hs.down(out_counts, d_cnt, c);
    return hs.finish();
}

// ---- representatives ------------------------------------------------------------------------------------------------------
extern "C" yams_status_t yams_cluster_representatives_device(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                             const uint64_t* cluster_offsets, const uint32_t* candidates,
                                                             const float* centroids, const uint8_t* centroid_empty, uint32_t n_clusters,
                                                             uint32_t n_extra, uint32_t* out_selected, uint32_t* out_counts) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_shape(ctx, rows, n, dim, n_clusters));
    if (n_extra > YAMS_CLUSTER_MAX_REPRESENTATIVES) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n_extra exceeds YAMS_CLUSTER_MAX_REPRESENTATIVES");
    if (n_clusters == 0) return YAMS_OK;
    if (!cluster_offsets || !centroids || !out_counts || (n_extra && !out_selected))
        return fail(ctx, YAMS_ERR_INVALID_ARG, "null cluster_offsets, centroids or output");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    uint64_t total;
    YA_TRY(read_words(ctx, cluster_offsets + n_clusters, 2, &total));
    if (total >= kMaxEntries) return fail(ctx, YAMS_ERR_UNSUPPORTED, "the lists must hold fewer than 2^32 entries");
    if (total && !candidates) return fail(ctx, YAMS_ERR_INVALID_ARG, "null candidates");
    YA_TRY(check_lists(ctx, cluster_offsets, n_clusters, total, candidates, static_cast<uint32_t>(n), nullptr, 0, 0, "candidates"));

    // (lhsNorm, sqrt) of every row and of every centroid, once: the same chain whoever asks.  A non-finite row refuses the call.
    double2* d_na; double2* d_nb; uint32_t* d_flag; uint32_t nonfinite;
    YA_TRY(ws_get(ctx, "art_row_norm", static_cast<size_t>(n ? n : 1) * sizeof(double2), (void**)&d_na));
    YA_TRY(ws_get(ctx, "art_cent_norm", static_cast<size_t>(n_clusters) * sizeof(double2), (void**)&d_nb));
    YA_TRY(flags_get(ctx, 4, &d_flag));
    YA_HIP(ctx, launch_kmeans_norm(st, rows, n, dim, d_na, d_flag));
    YA_HIP(ctx, launch_kmeans_norm(st, centroids, n_clusters, dim, d_nb, nullptr));
    YA_TRY(read_words(ctx, d_flag, 1, &nonfinite));
    if (nonfinite) return fail(ctx, YAMS_ERR_INVALID_ARG, "a row holds a non-finite value");

    uint32_t* d_owner; uint32_t* d_limit; uint32_t* d_last; uint8_t* d_used; double* d_min;
    const size_t t1 = static_cast<size_t>(total ? total : 1);
    YA_TRY(ws_get(ctx, "art_owner", t1 * 4, (void**)&d_owner));
    YA_TRY(ws_get(ctx, "art_last", static_cast<size_t>(n_clusters) * 4, (void**)&d_last));
    YA_TRY(ws_get(ctx, "art_used", t1, (void**)&d_used));
    YA_TRY(ws_get(ctx, "art_min_dist", t1 * 8, (void**)&d_min));
    d_limit = out_counts;      // extraLimit is the number selected: a pass always finds a winner among the unused candidates
    {
        TimedRegion tr(ctx, "artifact_representatives");
        YA_HIP(ctx, hipMemsetAsync(d_used, 0, t1, st));
        // minDist starts at 0x7f7f7f7f7f7f7f7f = 1.38e306 (what a byte fill can write) instead of DBL_MAX: it only has to exceed
        // every distance (<= 2; a NaN never replaces it) and be the same for every candidate.
        YA_HIP(ctx, hipMemsetAsync(d_min, 0x7f, t1 * 8, st));
        if (n_extra) YA_HIP(ctx, hipMemsetAsync(out_selected, 0xff, static_cast<size_t>(n_clusters) * n_extra * 4, st));
        YA_HIP(ctx, launch_artifact_owner(st, cluster_offsets, n_clusters, total, d_owner));
        YA_HIP(ctx, launch_artifact_rep_init(st, cluster_offsets, n_clusters, centroid_empty, n_extra, d_limit, d_last));
        for (uint32_t s = 0; s < n_extra; ++s)      // the dependent selections, enqueued at once
            YA_HIP(ctx, launch_artifact_rep_pass(st, rows, dim, d_na, cluster_offsets, candidates, d_owner, total, n_clusters, centroids, d_nb,
                                                 d_limit, d_last, s, n_extra, d_used, d_min, out_selected));
        tr.end();
    }
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

extern "C" yams_status_t yams_cluster_representatives_host(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                           const uint64_t* cluster_offsets, const uint32_t* candidates,
                                                           const float* centroids, const uint8_t* centroid_empty, uint32_t n_clusters,
                                                           uint32_t n_extra, uint32_t* out_selected, uint32_t* out_counts) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_shape(ctx, rows, n, dim, n_clusters));
    if (n_extra > YAMS_CLUSTER_MAX_REPRESENTATIVES) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n_extra exceeds YAMS_CLUSTER_MAX_REPRESENTATIVES");
    if (n_clusters == 0) return YAMS_OK;
    if (!cluster_offsets || !centroids || !out_counts || (n_extra && !out_selected))
        return fail(ctx, YAMS_ERR_INVALID_ARG, "null cluster_offsets, centroids or output");
    if (!offsets_ascend(cluster_offsets, n_clusters)) return fail(ctx, YAMS_ERR_INVALID_ARG, "the offsets do not start at 0 or decrease");
    const uint64_t total = cluster_offsets[n_clusters];
    if (total >= kMaxEntries) return fail(ctx, YAMS_ERR_UNSUPPORTED, "the lists must hold fewer than 2^32 entries");
    if (total && !candidates) return fail(ctx, YAMS_ERR_INVALID_ARG, "null candidates");
    HostStage hs(ctx);
    const size_t c = n_clusters;
    const float* d_rows = hs.up("art_host_rows", rows, static_cast<size_t>(n) * dim);
    const uint64_t* d_off = hs.up("art_host_offsets", cluster_offsets, c + 1);
    const uint32_t* d_cand = hs.up("art_host_list", candidates, static_cast<size_t>(total));
    const float* d_cent = hs.up("art_host_centroids", centroids, c * dim);
    const uint8_t* d_empty = hs.up("art_host_empty", centroid_empty, c);
    uint32_t* d_sel = hs.room<uint32_t>("art_host_selected", c * n_extra);
    uint32_t* d_cnt = hs.room<uint32_t>("art_host_counts", c);
    YA_TRY(hs.status());
    YA_TRY(yams_cluster_representatives_device(ctx, d_rows, n, dim, d_off, d_cand, d_cent, d_empty, n_clusters, n_extra, d_sel, d_cnt));
    hs.down(out_selected, d_sel, c * n_extra);
    hs.down(out_counts, d_cnt, c);
    return hs.finish();
}

// ---- residuals ------------------------------------------------------------------------------------------------------------
namespace {

yams_status_t check_residual_args(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t c,
                                  const uint32_t* primary, const uint64_t* cand_offsets, const uint32_t* cand, uint32_t form,
                                  const double* out_primary, const double* out_norm, const double* out_dot) {
    YA_TRY(check_shape(ctx, rows, n, dim, c));
    if (form != YAMS_RESIDUAL_SEPARATE && form != YAMS_RESIDUAL_FUSED) return fail(ctx, YAMS_ERR_INVALID_ARG, "unknown residual form");
    if ((cand_offsets == nullptr) != (cand == nullptr)) return fail(ctx, YAMS_ERR_INVALID_ARG, "cand_offsets and cand go together");
    if (n == 0) return YAMS_OK;
    if (c && !centroids) return fail(ctx, YAMS_ERR_INVALID_ARG, "null centroids");
    if (primary && (!out_primary || !out_dot)) return fail(ctx, YAMS_ERR_INVALID_ARG, "a primary needs out_primary_norm_sq and out_residual_dot");
    if (!out_norm && (cand_offsets || c)) return fail(ctx, YAMS_ERR_INVALID_ARG, "null out_cand_norm_sq");
    return YAMS_OK;
}

} // namespace

extern "C" yams_status_t yams_cluster_residuals_device(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                       const float* centroids, uint32_t n_clusters, const uint32_t* primary,
                                                       const uint64_t* cand_offsets, const uint32_t* cand, uint32_t form,
                                                       double* out_primary_norm_sq, double* out_cand_norm_sq, double* out_residual_dot) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_residual_args(ctx, rows, n, dim, centroids, n_clusters, primary, cand_offsets, cand, form, out_primary_norm_sq,
                               out_cand_norm_sq, out_residual_dot));
    if (n == 0) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const bool fused = form == YAMS_RESIDUAL_FUSED;
    uint64_t total = 0;
    if (cand_offsets) {
        YA_TRY(read_words(ctx, cand_offsets + n, 2, &total));
        if (total >= kMaxEntries) return fail(ctx, YAMS_ERR_UNSUPPORTED, "the lists must hold fewer than 2^32 entries");
    }
    if (cand_offsets || primary)
        YA_TRY(check_lists(ctx, cand_offsets, n, total, cand, n_clusters, primary, n, n_clusters, "primary / cand"));
    uint32_t* d_owner = nullptr;
    if (cand_offsets) YA_TRY(ws_get(ctx, "art_owner", static_cast<size_t>(total ? total : 1) * 4, (void**)&d_owner));
    TimedRegion tr(ctx, "artifact_residuals");
    hipError_t e = hipSuccess;
    if (primary) e = launch_artifact_primary_norm(st, rows, n, dim, centroids, primary, fused, out_primary_norm_sq);
    if (e == hipSuccess && cand_offsets) {
        e = launch_artifact_owner(st, cand_offsets, static_cast<uint32_t>(n), total, d_owner);
        if (e == hipSuccess)
            e = launch_artifact_residual_list(st, rows, dim, centroids, primary, d_owner, cand, total, fused, out_cand_norm_sq,
                                              primary ? out_residual_dot : nullptr);
    } else if (e == hipSuccess && n_clusters) {
        e = launch_artifact_residual_dense(st, rows, n, dim, centroids, n_clusters, primary, fused, out_cand_norm_sq,
                                           primary ? out_residual_dot : nullptr);
    }
    tr.end();
    YA_HIP(ctx, e);
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

// Documents are served in slices whose pair outputs fit kHostOutBytes on the device; rows and centroids are uploaded once.
extern "C" yams_status_t yams_cluster_residuals_host(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                     const float* centroids, uint32_t n_clusters, const uint32_t* primary,
                                                     const uint64_t* cand_offsets, const uint32_t* cand, uint32_t form,
                                                     double* out_primary_norm_sq, double* out_cand_norm_sq, double* out_residual_dot) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_residual_args(ctx, rows, n, dim, centroids, n_clusters, primary, cand_offsets, cand, form, out_primary_norm_sq,
                               out_cand_norm_sq, out_residual_dot));
    if (n == 0) return YAMS_OK;
    uint64_t total = 0;
    if (cand_offsets) {
        if (!offsets_ascend(cand_offsets, n)) return fail(ctx, YAMS_ERR_INVALID_ARG, "the offsets do not start at 0 or decrease");
        total = cand_offsets[n];
        if (total >= kMaxEntries) return fail(ctx, YAMS_ERR_UNSUPPORTED, "the lists must hold fewer than 2^32 entries");
    }
    // judged here for the whole call, so that no slice is written before a later one is refused
    if ((primary && !indices_below(primary, n, n_clusters, true)) || !indices_below(cand, total, n_clusters))
        return fail(ctx, YAMS_ERR_INVALID_ARG, "primary / cand: an index is out of range");
    HostStage hs(ctx);
    const float* d_rows = hs.up("art_host_rows", rows, static_cast<size_t>(n) * dim);
    const float* d_cent = hs.up("art_host_centroids", centroids, static_cast<size_t>(n_clusters) * dim);
    const uint32_t* d_pri = hs.up("art_host_primary", primary, static_cast<size_t>(n));
    // slices of documents: [lo, hi) holds at most kHostOutBytes / 16 pairs (two fp64 outputs per pair), at least one document
    const uint64_t max_pairs = kHostOutBytes / 16;
    std::vector<uint64_t> local;
    for (uint64_t lo = 0; lo < n;) {
        uint64_t hi, pairs;
        if (cand_offsets) {
            hi = lo + 1;
            while (hi < n && cand_offsets[hi + 1] - cand_offsets[lo] <= max_pairs) ++hi;
            pairs = cand_offsets[hi] - cand_offsets[lo];
        } else {
            const uint64_t per = std::max<uint64_t>(1, max_pairs / std::max<uint32_t>(1, n_clusters));
            hi = std::min(n, lo + per);
            pairs = (hi - lo) * n_clusters;
        }
        const uint64_t m = hi - lo;
        const size_t np = static_cast<size_t>(pairs);
        double* d_cn = hs.room<double>("art_host_cand_norm", np);
        double* d_pn = primary ? hs.room<double>("art_host_primary_norm", static_cast<size_t>(m)) : nullptr;
        double* d_rd = primary ? hs.room<double>("art_host_residual_dot", np) : nullptr;
        const uint64_t* d_off = nullptr; const uint32_t* d_cand = nullptr;
        if (cand_offsets) {
            local.resize(m + 1);
            for (uint64_t i = 0; i <= m; ++i) local[i] = cand_offsets[lo + i] - cand_offsets[lo];
            d_off = hs.up("art_host_offsets", local.data(), static_cast<size_t>(m + 1));
            d_cand = hs.up("art_host_list", cand + cand_offsets[lo], np);
            YA_TRY(hs.finish());      // `local` is reused by the next slice
        }
        YA_TRY(hs.status());
        const size_t o = static_cast<size_t>(cand_offsets ? cand_offsets[lo] : lo * n_clusters);
        YA_TRY(yams_cluster_residuals_device(ctx, d_rows + lo * dim, m, dim, d_cent, n_clusters, primary ? d_pri + lo : nullptr, d_off, d_cand,
                                             form, d_pn, d_cn, d_rd));
        hs.down(out_cand_norm_sq + o, d_cn, np);
        if (primary) {
            hs.down(out_primary_norm_sq + lo, d_pn, static_cast<size_t>(m));
            hs.down(out_residual_dot + o, d_rd, np);
        }
        YA_TRY(hs.finish());
        lo = hi;
    }
    return YAMS_OK;
}
