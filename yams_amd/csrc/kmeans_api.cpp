// kmeans_api.cpp — yams_cluster_kmeans_device / _host, yams_cluster_assign_device: runKMeans and nearestCentroid of the
// topology engine "kmeans_v1" behind the C ABI.
//
// Mirrors runKMeans (src/topology/topology_alternate_engines.cpp:341-478) over the usable rows:
//   row norms (+ the finiteness test) -> initialisation: centroid 0, then k - 1 steps of [distance to the last centroid, minDist,
//   block arg-max] + [arg-max, normalized(row) as the next centroid], all enqueued at once -> per iteration: assignment,
//   grouping, centroids, then ONE read-back of (member counts, changed) -> the repair path, host-driven, when a count is zero.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "accel_ctx.h"
#include "host_stage.h"
#include "kmeans_launch.h"

using namespace yams_accel;

namespace {

constexpr uint64_t kMaxRows = 1ull << 31;

// The argument checks the three entries share (no device needed).  *done: the call is complete (n == 0).
yams_status_t check_shape(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, bool* done) {
    *done = false;
    if (n == 0) { *done = true; return YAMS_OK; }
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (!rows) return fail(ctx, YAMS_ERR_INVALID_ARG, "null rows");
    if (n >= kMaxRows) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n must be < 2^31");
    if (dim > YAMS_CLUSTER_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_CLUSTER_MAX_DIM");
    return YAMS_OK;
}

// k of :367-371
uint64_t effective_k(uint64_t n, uint32_t k) {
    uint64_t kk = k;
    if (kk == 0) kk = static_cast<uint64_t>(std::round(std::sqrt(static_cast<double>(n))));
    return std::min<uint64_t>(std::max<uint64_t>(kk, 2), n);
}

// (na, sqrt(na)) of every row; a non-finite row refuses the call.  Synchronises.
yams_status_t row_norms(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, double2** out) {
    hipStream_t st = ctx->stream;
    double2* d_na; uint32_t* d_flag; uint32_t nonfinite;
    YA_TRY(ws_get(ctx, "km_row_norm", static_cast<size_t>(n) * sizeof(double2), (void**)&d_na));
    YA_TRY(flags_get(ctx, 4, &d_flag));
    YA_HIP(ctx, launch_kmeans_norm(st, rows, n, dim, d_na, d_flag));
    YA_TRY(read_words(ctx, d_flag, 1, &nonfinite));
    if (nonfinite) return fail(ctx, YAMS_ERR_INVALID_ARG, "a row holds a non-finite value");
    *out = d_na;
    return YAMS_OK;
}

} // namespace

extern "C" yams_status_t yams_cluster_kmeans_device(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, uint32_t k,
                                                    uint32_t max_iterations, uint32_t* out_membership, float* out_centroids,
                                                    uint32_t* out_k, uint32_t* out_iterations) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (out_k) *out_k = 0;
    if (out_iterations) *out_iterations = 0;
    bool done;
    YA_TRY(check_shape(ctx, rows, n, dim, &done));
    if (done) return YAMS_OK;
    if (n < 2) return fail(ctx, YAMS_ERR_INVALID_ARG, "k-means of fewer than two rows");
    if (!out_membership) return fail(ctx, YAMS_ERR_INVALID_ARG, "null out_membership");
    const uint64_t k64 = effective_k(n, k);
    if (k64 > YAMS_CLUSTER_MAX_K) return fail(ctx, YAMS_ERR_UNSUPPORTED, "k exceeds YAMS_CLUSTER_MAX_K");
    const uint32_t K = static_cast<uint32_t>(k64);
    const uint32_t iterations = max_iterations == 0 ? 10u : max_iterations;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;

    double2* d_na;
    YA_TRY(row_norms(ctx, rows, n, dim, &d_na));
    const uint32_t n_parts = static_cast<uint32_t>((n + 255) / 256);
    float* d_cent; double2* d_nb; double* d_dist; uint8_t* d_sel; double* d_pv; uint32_t* d_pi;
    uint32_t* d_counts; uint32_t* d_offsets; uint32_t* d_members; uint32_t* h_counts;
    YA_TRY(ws_get(ctx, "km_centroids", static_cast<size_t>(K) * dim * 4, (void**)&d_cent));
    YA_TRY(ws_get(ctx, "km_cent_norm", static_cast<size_t>(K) * sizeof(double2), (void**)&d_nb));
    YA_TRY(ws_get(ctx, "km_dist", static_cast<size_t>(n) * 8, (void**)&d_dist));      // minDist, later the repair's distances
    YA_TRY(ws_get(ctx, "km_selected", static_cast<size_t>(n), (void**)&d_sel));
    YA_TRY(ws_get(ctx, "km_part_val", static_cast<size_t>(n_parts) * 8, (void**)&d_pv));
    YA_TRY(ws_get(ctx, "km_part_idx", static_cast<size_t>(n_parts) * 4, (void**)&d_pi));
    YA_TRY(ws_get(ctx, "km_counts", (static_cast<size_t>(K) + 1) * 4, (void**)&d_counts));   // [K] counts, [K] changed
    YA_TRY(ws_get(ctx, "km_offsets", (static_cast<size_t>(K) + 1) * 4, (void**)&d_offsets));
    YA_TRY(ws_get(ctx, "km_members", static_cast<size_t>(n) * 4, (void**)&d_members));
    YA_TRY(pinned_get(ctx, (static_cast<size_t>(K) + 1) * 4 + 64, (void**)&h_counts));
    uint32_t* d_changed = d_counts + K;

    // ---- initialisation (:373-401): minDist = DBL_MAX, nothing selected; K - 1 dependent steps without a host round trip
    {
        TimedRegion tr(ctx, "kmeans_init");
        YA_HIP(ctx, hipMemsetAsync(d_sel, 0, static_cast<size_t>(n), st));
        // minDist starts at 0x7f7f7f7f7f7f7f7f = 1.38e306 (what a byte fill can write) instead of DBL_MAX: the initial value
        // only has to exceed every distance (<= 2; a NaN never replaces it) and be the same for every row.
        YA_HIP(ctx, hipMemsetAsync(d_dist, 0x7f, static_cast<size_t>(n) * 8, st));
        YA_HIP(ctx, launch_kmeans_pick(st, nullptr, nullptr, 0, 0, rows, dim, d_sel, d_cent, d_nb, 0));
        for (uint32_t s = 1; s < K; ++s) {
            YA_HIP(ctx, launch_kmeans_init_dist(st, rows, n, dim, d_na, d_cent, d_nb, s - 1, d_sel, d_dist, d_pv, d_pi));
            YA_HIP(ctx, launch_kmeans_pick(st, d_pv, d_pi, n_parts, 0, rows, dim, d_sel, d_cent, d_nb, s));
        }
        tr.end();
    }

    // ---- Lloyd iterations (:412-466)
    YA_HIP(ctx, hipMemsetAsync(out_membership, 0, static_cast<size_t>(n) * 4, st));
    uint32_t ran = 0;
    std::vector<uint32_t> hm;
    std::vector<double> hd;
    for (uint32_t iter = 0; iter < iterations; ++iter) {
        YA_HIP(ctx, hipMemsetAsync(d_counts, 0, (static_cast<size_t>(K) + 1) * 4, st));
        {
            TimedRegion tr(ctx, "kmeans_assign");
            YA_HIP(ctx, launch_kmeans_assign(st, rows, n, dim, d_na, d_cent, d_nb, K, nullptr, out_membership, d_changed, nullptr, nullptr));
            tr.end();
        }
        {
            TimedRegion tr(ctx, "kmeans_update");
            YA_HIP(ctx, launch_kmeans_group(st, out_membership, n, K, d_counts, d_offsets, d_members));
            YA_HIP(ctx, launch_kmeans_centroids(st, rows, dim, d_members, d_offsets, d_counts, K, -1, d_cent, d_nb));
            tr.end();
        }
        YA_HIP(ctx, hipMemcpyAsync(h_counts, d_counts, (static_cast<size_t>(K) + 1) * 4, hipMemcpyDeviceToHost, st));
        YA_HIP(ctx, hipStreamSynchronize(st));
        ++ran;
        bool changed = h_counts[K] != 0;
        if (std::find(h_counts, h_counts + K, 0u) != h_counts + K) {
            // ---- the repair path (:433-462), host-driven
            std::vector<uint32_t> cnt(h_counts, h_counts + K);
            hm.resize(n); hd.resize(n);
            YA_HIP(ctx, hipMemcpyAsync(hm.data(), out_membership, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, st));
            YA_HIP(ctx, hipStreamSynchronize(st));
            for (uint32_t c = 0; c < K; ++c) {
                if (cnt[c] != 0) continue;
                YA_HIP(ctx, launch_kmeans_own_dist(st, rows, n, dim, d_na, d_cent, d_nb, out_membership, d_dist));
                YA_HIP(ctx, hipMemcpyAsync(hd.data(), d_dist, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost, st));
                YA_HIP(ctx, hipStreamSynchronize(st));
                uint64_t worst = n; uint32_t donor = K; double worst_d = -1.0;
                for (uint64_t u = 0; u < n; ++u) {
                    const uint32_t mc = hm[u];
                    if (cnt[mc] <= 1) continue;
                    if (hd[u] > worst_d) { worst_d = hd[u]; worst = u; donor = mc; }
                }
                if (worst == n) continue;
                hm[worst] = c; --cnt[donor]; cnt[c] = 1;
                YA_HIP(ctx, hipMemcpyAsync(out_membership + worst, &hm[worst], 4, hipMemcpyHostToDevice, st));
                YA_HIP(ctx, launch_kmeans_pick(st, nullptr, nullptr, 0, static_cast<uint32_t>(worst), rows, dim, nullptr, d_cent, d_nb, c));
                YA_HIP(ctx, hipMemsetAsync(d_counts, 0, static_cast<size_t>(K) * 4, st));
                YA_HIP(ctx, launch_kmeans_group(st, out_membership, n, K, d_counts, d_offsets, d_members));
                YA_HIP(ctx, launch_kmeans_centroids(st, rows, dim, d_members, d_offsets, d_counts, K, static_cast<int>(donor), d_cent, d_nb));
                YA_HIP(ctx, hipStreamSynchronize(st));   // (hm[worst] was the source of an asynchronous copy)
                changed = true;
            }
        }
        if (!changed) break;
    }
    if (out_centroids) YA_HIP(ctx, hipMemcpyAsync(out_centroids, d_cent, static_cast<size_t>(K) * dim * 4, hipMemcpyDeviceToDevice, st));
    YA_HIP(ctx, hipStreamSynchronize(st));
    if (out_k) *out_k = K;
    if (out_iterations) *out_iterations = ran;
    return YAMS_OK;
}

extern "C" yams_status_t yams_cluster_assign_device(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                    const float* centroids, uint32_t n_centroids, const uint8_t* centroid_empty,
                                                    uint32_t* out_assign, double* out_distance) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    bool done;
    YA_TRY(check_shape(ctx, rows, n, dim, &done));
    if (done) return YAMS_OK;
    if (!out_assign) return fail(ctx, YAMS_ERR_INVALID_ARG, "null out_assign");
    if (n_centroids && !centroids) return fail(ctx, YAMS_ERR_INVALID_ARG, "null centroids");
    if (n_centroids > YAMS_CLUSTER_MAX_K) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n_centroids exceeds YAMS_CLUSTER_MAX_K");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    double2* d_na;
    YA_TRY(row_norms(ctx, rows, n, dim, &d_na));
    double2* d_nb;
    YA_TRY(ws_get(ctx, "km_cent_norm", (static_cast<size_t>(n_centroids) + 1) * sizeof(double2), (void**)&d_nb));
    YA_HIP(ctx, launch_kmeans_norm(st, centroids, n_centroids, dim, d_nb, nullptr));
    {
        TimedRegion tr(ctx, "kmeans_assign");
        YA_HIP(ctx, launch_kmeans_assign(st, rows, n, dim, d_na, centroids, d_nb, n_centroids, centroid_empty, nullptr, nullptr,
                                         out_assign, out_distance));
        tr.end();
    }
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

extern "C" yams_status_t yams_cluster_kmeans_host(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, uint32_t k,
                                                  uint32_t max_iterations, uint32_t* out_membership, float* out_centroids,
                                                  uint32_t* out_k, uint32_t* out_iterations) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (out_k) *out_k = 0;
    if (out_iterations) *out_iterations = 0;
    bool done;
    YA_TRY(check_shape(ctx, rows, n, dim, &done));
    if (done) return YAMS_OK;
    if (n < 2) return fail(ctx, YAMS_ERR_INVALID_ARG, "k-means of fewer than two rows");
    if (!out_membership) return fail(ctx, YAMS_ERR_INVALID_ARG, "null out_membership");
    const uint64_t k64 = effective_k(n, k);
    if (k64 > YAMS_CLUSTER_MAX_K) return fail(ctx, YAMS_ERR_UNSUPPORTED, "k exceeds YAMS_CLUSTER_MAX_K");
    HostStage hs(ctx);
    const float* d_rows = hs.up("km_host_rows", rows, static_cast<size_t>(n) * dim);
    uint32_t* d_mem = hs.room<uint32_t>("km_host_membership", static_cast<size_t>(n));
    float* d_cent = out_centroids ? hs.room<float>("km_host_centroids", static_cast<size_t>(k64) * dim) : nullptr;
    YA_TRY(hs.status());
    uint32_t ke = 0;
    YA_TRY(yams_cluster_kmeans_device(ctx, d_rows, n, dim, k, max_iterations, d_mem, d_cent, &ke, out_iterations));
    hs.down(out_membership, d_mem, static_cast<size_t>(n));
    hs.down(out_centroids, d_cent, static_cast<size_t>(ke) * dim);
    YA_TRY(hs.finish());
    if (out_k) *out_k = ke;
    return YAMS_OK;
}
