// plugin_topology.cpp — the plugin door's topology families: topology_cluster_v1, semantic_graph_v1, topology_smooth_v1,
// topology_artifacts_v1, topology_route_v1, topology_quality_v1, topology_features_v1, late_interaction_rerank_v1 and
// embedding_pool_v1.  A door here allocates what it hands out (OwnedArrays), keeps what lives across calls (the route indexes,
// a HandleTable) or only leases a work context and forwards (Leased); the arithmetic is the flat entries'.
#include <cmath>

#include "plugin_state.h"

namespace yams_accel {
namespace door {
namespace {

// ---- topology_cluster_v1: the topology build's k-means over host memory (yams_cluster_kmeans_host / _assign_device) --------
yams_status_t tc_kmeans(void*, const float* rows, uint64_t n, uint32_t dim, uint32_t k, uint32_t max_iterations,
                        uint32_t** out_membership, float** out_centroids, uint32_t* out_k, uint32_t* out_iterations) {
    NEED_INIT();
    if (!out_membership) return YAMS_ERR_INVALID_ARG;
    *out_membership = nullptr;
    if (out_centroids) *out_centroids = nullptr;
    if (out_k) *out_k = 0;
    if (out_iterations) *out_iterations = 0;
    if (n == 0) return YAMS_OK;
    if (dim == 0 || !rows || n < 2) return YAMS_ERR_INVALID_ARG;
    if (n >= (1ull << 31) || dim > YAMS_CLUSTER_MAX_DIM) return YAMS_ERR_UNSUPPORTED;
    // the clamped k bounds the centroid array (:367-371)
    uint64_t kk = k ? k : static_cast<uint64_t>(std::round(std::sqrt(static_cast<double>(n))));
    kk = std::min<uint64_t>(std::max<uint64_t>(kk, 2), n);
    if (kk > YAMS_CLUSTER_MAX_K) return YAMS_ERR_UNSUPPORTED;
    OwnedArrays res;
    uint32_t* mem = res.add(out_membership, static_cast<size_t>(n));
    float* cent = res.add(out_centroids, static_cast<size_t>(kk) * dim, out_centroids != nullptr);
    if (!res.ok()) return YAMS_ERR_RESOURCE_EXHAUSTED;
    Lease<yams_accel_ctx*> w(g.work_ctx);
    YA_TRY(yams_cluster_kmeans_host(w.v, rows, n, dim, k, max_iterations, mem, cent, out_k, out_iterations));
    return res.commit();
}

yams_status_t tc_assign(void*, const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t n_centroids,
                        const uint8_t* centroid_empty, uint32_t** out_assign, double** out_distance) {
    NEED_INIT();
    if (!out_assign) return YAMS_ERR_INVALID_ARG;
    *out_assign = nullptr;
    if (out_distance) *out_distance = nullptr;
    if (n == 0) return YAMS_OK;
    if (dim == 0 || !rows || (n_centroids && !centroids)) return YAMS_ERR_INVALID_ARG;
    if (n >= (1ull << 31) || dim > YAMS_CLUSTER_MAX_DIM || n_centroids > YAMS_CLUSTER_MAX_K) return YAMS_ERR_UNSUPPORTED;
    OwnedArrays res;
    uint32_t* asg = res.add(out_assign, static_cast<size_t>(n));
    double* dist = res.add(out_distance, static_cast<size_t>(n), out_distance != nullptr);
    if (!res.ok()) return YAMS_ERR_RESOURCE_EXHAUSTED;
    Lease<yams_accel_ctx*> w(g.work_ctx);
    yams_accel_ctx* x = w.v;
    const size_t rb = static_cast<size_t>(n) * dim * 4, cb = static_cast<size_t>(n_centroids) * dim * 4;
    float* d_rows; float* d_cent; uint8_t* d_empty = nullptr; uint32_t* d_asg; double* d_dist = nullptr;
    YA_TRY(yams_accel::ws_get(x, "plugin_tc_rows", rb, (void**)&d_rows));
    YA_TRY(yams_accel::ws_get(x, "plugin_tc_centroids", cb + 16, (void**)&d_cent));
    YA_TRY(yams_accel::ws_get(x, "plugin_tc_assign", static_cast<size_t>(n) * 4, (void**)&d_asg));
    if (out_distance) YA_TRY(yams_accel::ws_get(x, "plugin_tc_distance", static_cast<size_t>(n) * 8, (void**)&d_dist));
    if (centroid_empty && n_centroids) {
        YA_TRY(yams_accel::ws_get(x, "plugin_tc_empty", n_centroids, (void**)&d_empty));
        if (yams_accel_upload(x, d_empty, centroid_empty, n_centroids) != YAMS_OK) return YAMS_ERR_INTERNAL;
    }
    if (yams_accel_upload(x, d_rows, rows, rb) != YAMS_OK || (cb && yams_accel_upload(x, d_cent, centroids, cb) != YAMS_OK)) return YAMS_ERR_INTERNAL;
    YA_TRY(yams_cluster_assign_device(x, d_rows, n, dim, d_cent, n_centroids, d_empty, d_asg, d_dist));
    if (yams_accel_download(x, asg, d_asg, static_cast<size_t>(n) * 4) != YAMS_OK ||
        (dist && yams_accel_download(x, dist, d_dist, static_cast<size_t>(n) * 8) != YAMS_OK)) return YAMS_ERR_INTERNAL;
    return res.commit();
}

// ---- semantic_graph_v1: the semantic-neighbour graph over host memory (yams_graph_semantic_neighbors_host) ------------------
yams_status_t sg_neighbors(void*, const float* rows, uint64_t n, uint32_t dim, const uint32_t* tie_rank, const uint32_t* source_rows,
                           uint64_t n_sources, uint32_t k, uint32_t flags, float threshold, uint32_t** out_rows, float** out_sims,
                           uint32_t** out_counts, float** out_inv_norm, yams_graph_diag_t* out_diag) {
    NEED_INIT();
    if (!out_rows || !out_sims || !out_counts) return YAMS_ERR_INVALID_ARG;
    *out_rows = nullptr; *out_sims = nullptr; *out_counts = nullptr;
    if (out_inv_norm) *out_inv_norm = nullptr;
    if (out_diag) std::memset(out_diag, 0, sizeof *out_diag);
    const uint64_t S = source_rows ? n_sources : n;
    // the limits bound the arrays allocated here; every other check is the flat entry's
    if (n >= (1ull << 31) || S >= (1ull << 31) || dim > YAMS_GRAPH_MAX_DIM || k > YAMS_GRAPH_MAX_K) return YAMS_ERR_UNSUPPORTED;
    // an empty result: no array is wanted, the out parameters keep their nulls (the flat entry still judges flags and threshold)
    const bool some = k != 0 && n >= 2 && S != 0;
    const size_t slots = static_cast<size_t>(S) * k;
    OwnedArrays res;
    uint32_t* r = res.add(out_rows, slots, some);
    float* s = res.add(out_sims, slots, some);
    uint32_t* c = res.add(out_counts, static_cast<size_t>(S), some);
    float* iv = res.add(out_inv_norm, static_cast<size_t>(n), some && out_inv_norm != nullptr);
    if (!res.ok()) return YAMS_ERR_RESOURCE_EXHAUSTED;
    Lease<yams_accel_ctx*> w(g.work_ctx);
    YA_TRY(yams_graph_semantic_neighbors_host(w.v, rows, n, dim, tie_rank, source_rows, n_sources, k, flags, threshold, r, s, c, iv, out_diag));
    return res.commit();
}

// ---- topology_artifacts_v1: centroids, representatives, residuals over host memory (yams_cluster_*_host) -------------------
// the limits bound the arrays allocated here; every other check is the flat entries'
yams_status_t ta_centroids(void*, const float* rows, uint64_t n, uint32_t dim, const uint64_t* cluster_offsets, const uint32_t* members,
                           uint32_t n_clusters, float** out_centroids, uint32_t** out_counts) {
    NEED_INIT();
    if (!out_centroids || !out_counts) return YAMS_ERR_INVALID_ARG;
    *out_centroids = nullptr; *out_counts = nullptr;
    if (n >= (1ull << 31) || dim > YAMS_CLUSTER_MAX_DIM || n_clusters > YAMS_CLUSTER_MAX_K) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0) return YAMS_ERR_INVALID_ARG;
    if (n_clusters == 0) return YAMS_OK;
    OwnedArrays res;
    float* cent = res.add(out_centroids, static_cast<size_t>(n_clusters) * dim);
    uint32_t* cnt = res.add(out_counts, static_cast<size_t>(n_clusters));
    if (!res.ok()) return YAMS_ERR_RESOURCE_EXHAUSTED;
    Lease<yams_accel_ctx*> w(g.work_ctx);
    YA_TRY(yams_cluster_centroids_host(w.v, rows, n, dim, cluster_offsets, members, n_clusters, cent, cnt));
    return res.commit();
}

yams_status_t ta_representatives(void*, const float* rows, uint64_t n, uint32_t dim, const uint64_t* cluster_offsets,
                                 const uint32_t* candidates, const float* centroids, const uint8_t* centroid_empty, uint32_t n_clusters,
                                 uint32_t n_extra, uint32_t** out_selected, uint32_t** out_counts) {
    NEED_INIT();
    if (!out_selected || !out_counts) return YAMS_ERR_INVALID_ARG;
    *out_selected = nullptr; *out_counts = nullptr;
    if (n >= (1ull << 31) || dim > YAMS_CLUSTER_MAX_DIM || n_clusters > YAMS_CLUSTER_MAX_K || n_extra > YAMS_CLUSTER_MAX_REPRESENTATIVES)
        return YAMS_ERR_UNSUPPORTED;
    if (dim == 0) return YAMS_ERR_INVALID_ARG;
    if (n_clusters == 0) return YAMS_OK;
    OwnedArrays res;
    uint32_t* sel = res.add(out_selected, static_cast<size_t>(n_clusters) * n_extra, n_extra != 0);
    uint32_t* cnt = res.add(out_counts, static_cast<size_t>(n_clusters));
    if (!res.ok()) return YAMS_ERR_RESOURCE_EXHAUSTED;
    Lease<yams_accel_ctx*> w(g.work_ctx);
    YA_TRY(yams_cluster_representatives_host(w.v, rows, n, dim, cluster_offsets, candidates, centroids, centroid_empty, n_clusters, n_extra, sel, cnt));
    return res.commit();
}

yams_status_t ta_residuals(void*, const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t n_clusters,
                           const uint32_t* primary, const uint64_t* cand_offsets, const uint32_t* cand, uint32_t form,
                           double** out_primary_norm_sq, double** out_cand_norm_sq, double** out_residual_dot) {
    NEED_INIT();
    if (!out_cand_norm_sq || (primary && (!out_primary_norm_sq || !out_residual_dot))) return YAMS_ERR_INVALID_ARG;
    *out_cand_norm_sq = nullptr;
    if (out_primary_norm_sq) *out_primary_norm_sq = nullptr;
    if (out_residual_dot) *out_residual_dot = nullptr;
    if (n >= (1ull << 31) || dim > YAMS_CLUSTER_MAX_DIM || n_clusters > YAMS_CLUSTER_MAX_K) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0 || (cand_offsets == nullptr) != (cand == nullptr)) return YAMS_ERR_INVALID_ARG;
    if (n == 0) return YAMS_OK;
    if (cand_offsets)      // the offsets size the arrays: judged here first
        for (uint64_t i = 0; i < n; ++i)
            if (cand_offsets[0] != 0 || cand_offsets[i + 1] < cand_offsets[i]) return YAMS_ERR_INVALID_ARG;
    const uint64_t pairs = cand_offsets ? cand_offsets[n] : n * n_clusters;
    const size_t p1 = static_cast<size_t>(pairs ? pairs : 1);
    OwnedArrays res;
    double* cn = res.add(out_cand_norm_sq, p1);
    double* pn = res.add(out_primary_norm_sq, static_cast<size_t>(n), primary != nullptr);
    double* rd = res.add(out_residual_dot, p1, primary != nullptr);
    if (!res.ok()) return YAMS_ERR_RESOURCE_EXHAUSTED;
    Lease<yams_accel_ctx*> w(g.work_ctx);
    YA_TRY(yams_cluster_residuals_host(w.v, rows, n, dim, centroids, n_clusters, primary, cand_offsets, cand, form, pn, cn, rd));
    return res.commit();
}

// ---- topology_route_v1: the cluster router's dense signal over a resident index (yams_route_index_* / yams_route_dense_host) ----
using RouteIndex = Handle<yams_route_index, yams_route_index_destroy>;
HandleTable<RouteIndex> route_indexes;

yams_status_t tr_index_create(void*, const float* vectors, uint64_t n_vectors, uint32_t dim, const uint32_t* cluster_offsets,
                              const uint8_t* has_centroid, const uint16_t* position, uint32_t n_clusters, uint64_t* out_id, float* out_norms) {
    NEED_INIT();
    if (!out_id) return YAMS_ERR_INVALID_ARG;
    auto e = std::make_shared<RouteIndex>();
    yams_status_t st = yams_accel_ctx_create(g.devices[0], nullptr, &e->ctx);
    if (st != YAMS_OK) return st;
    st = yams_route_index_create_host(e->ctx, vectors, n_vectors, dim, cluster_offsets, has_centroid, position, n_clusters, &e->obj, out_norms);
    if (st != YAMS_OK) { e->destroy(); return st; }
    *out_id = route_indexes.insert(e);
    return YAMS_OK;
}
yams_status_t tr_index_info(void*, uint64_t id, yams_route_index_info_t* out_info) {
    NEED_INIT();
    auto e = route_indexes.find(id);
    if (!e) return YAMS_ERR_NOT_FOUND;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->obj) return YAMS_ERR_NOT_FOUND;
    return yams_route_index_info(e->obj, out_info);
}
yams_status_t tr_dense(void*, uint64_t id, const float* queries, uint32_t n_queries, uint32_t rep_limit, const uint32_t* candidates,
                       float* out_dense, uint8_t* out_observed, uint32_t* out_evals, yams_route_diag_t* out_diag) {
    NEED_INIT();
    auto e = route_indexes.find(id);
    if (!e) return YAMS_ERR_NOT_FOUND;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->obj) return YAMS_ERR_NOT_FOUND;
    return yams_route_dense_host(e->obj, queries, n_queries, rep_limit, candidates, out_dense, out_observed, out_evals, out_diag);
}
yams_status_t tr_index_destroy(void*, uint64_t id) {
    NEED_INIT();
    auto e = route_indexes.take(id);
    if (!e) return YAMS_ERR_NOT_FOUND;
    std::lock_guard<std::mutex> lk(e->mu);
    e->destroy();
    return YAMS_OK;
}

// ---- topology_quality_v1: computePersistenceH0 over host memory (yams_quality_persistence_h0_host) --------------------------
// the limits bound the arrays allocated here; every other check is the flat entry's
yams_status_t tq_persistence_h0(void*, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select,
                                uint32_t form, yams_persistence_h0_t* out, double** out_distances, double** out_merge_weights) {
    NEED_INIT();
    if (!out) return YAMS_ERR_INVALID_ARG;
    const uint64_t m = select ? n_select : n;
    if (m > YAMS_QUALITY_MAX_POINTS || dim > YAMS_CLUSTER_MAX_DIM || n >= (1ull << 31)) return YAMS_ERR_UNSUPPORTED;
    OwnedArrays arrays;      // (nothing is nulled up front here: a refusal leaves the result and both out parameters as they were)
    double* dist = arrays.add(out_distances, static_cast<size_t>(m) * m, out_distances && m);
    double* w = arrays.add(out_merge_weights, static_cast<size_t>(m - 1), out_merge_weights && m >= 2);
    if (!arrays.ok()) return YAMS_ERR_RESOURCE_EXHAUSTED;
    yams_persistence_h0_t res{};
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    YA_TRY(yams_quality_persistence_h0_host(lease.v, rows, n, dim, select, n_select, form, &res, dist, w, nullptr));
    *out = res;
    return arrays.commit();
}

// ---- embedding_pool_v1: the embedding model's pooling head (yams_embed_*) over device addresses (over host memory: forwarded) --
// the hidden states (the rows) at a DEVICE address, everything else in host memory: the mask goes up, the B * dim result comes back
yams_status_t ep_pool_device(void*, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask, uint32_t mask_len,
                             uint32_t mode, uint32_t flags, float* out, yams_embed_diag_t* diag) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    yams_accel_ctx* ctx = lease.v;
    // what the flat entry refuses (or, batch == 0, answers) before it looks at a mask or an output: its verdict, nothing is staged
    if (batch == 0 || !out || dim == 0 || seq == 0 || dim > YAMS_EMBED_MAX_DIM || seq > YAMS_EMBED_MAX_SEQ || batch > YAMS_EMBED_MAX_ROWS / seq)
        return yams_embed_pool_device(ctx, hidden, batch, seq, dim, nullptr, mask_len, mode, flags, out, diag);
    // only the considered columns of the mask go up: at most batch * seq values
    if (mode == YAMS_EMBED_POOL_CLS) mask = nullptr;
    const uint32_t cols = mask_len < seq ? mask_len : seq;
    const size_t mb = mask ? static_cast<size_t>(batch) * cols * 4 : 0, ob = static_cast<size_t>(batch) * dim * 4;
    int32_t* d_mask = nullptr; float* d_out;
    if (mb) YA_TRY(yams_accel::ws_get(ctx, "embed_door_mask", mb, (void**)&d_mask));
    YA_TRY(yams_accel::ws_get(ctx, "embed_door_out", ob, (void**)&d_out));
    if (mb && cols == mask_len) YA_HIP(ctx, yams_accel::staged_h2d(d_mask, mask, mb, ctx->stream));
    else if (mb) YA_HIP(ctx, hipMemcpy2DAsync(d_mask, static_cast<size_t>(cols) * 4, mask, static_cast<size_t>(mask_len) * 4, static_cast<size_t>(cols) * 4, batch, hipMemcpyHostToDevice, ctx->stream));
    if (mask && !mb) mask_len = 0;
    else if (mask) mask_len = cols;
    YA_TRY(yams_embed_pool_device(ctx, hidden, batch, seq, dim, d_mask, mask_len, mode, flags, d_out, diag));
    YA_HIP(ctx, hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    YA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return YAMS_OK;
}
yams_status_t ep_normalize_device(void*, const float* rows, uint64_t batch, uint32_t dim, float* out) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    yams_accel_ctx* ctx = lease.v;
    if (batch == 0 || !out || dim == 0 || dim > YAMS_EMBED_MAX_DIM || batch > YAMS_EMBED_MAX_ROWS)
        return yams_embed_normalize_device(ctx, rows, batch, dim, out);      // its verdict; nothing is staged
    const size_t ob = static_cast<size_t>(batch) * dim * 4;
    float* d_out;
    YA_TRY(yams_accel::ws_get(ctx, "embed_door_out", ob, (void**)&d_out));
    YA_TRY(yams_embed_normalize_device(ctx, rows, batch, dim, d_out));
    YA_HIP(ctx, hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    YA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return YAMS_OK;
}

} // namespace

// ---- the nine tables.  topology_smooth_v1 (SGC smoothing, yams_graph_sgc_smooth_host), topology_features_v1 (yams_features_*_host),
// late_interaction_rerank_v1 (yams_rerank_*_host) and the host-memory half of embedding_pool_v1 have no function above: every
// array is the caller's and every check the flat entry's (which also zeroes its diagnostics on every path), so they are Leased.
yams_topology_cluster_v1 g_topology_cluster = {YAMS_IFACE_TOPOLOGY_CLUSTER_V1_VERSION, nullptr, GUARDED(tc_kmeans), GUARDED(tc_assign),
                                               GUARDED(free_arrays<uint32_t, float>), GUARDED(free_arrays<uint32_t, double>)};
yams_semantic_graph_v1 g_semantic_graph = {YAMS_IFACE_SEMANTIC_GRAPH_V1_VERSION, nullptr, GUARDED(sg_neighbors), GUARDED(free_arrays<uint32_t, float, uint32_t, float>)};
yams_topology_smooth_v1 g_topology_smooth = {YAMS_IFACE_TOPOLOGY_SMOOTH_V1_VERSION, nullptr, GUARDED(Leased<&yams_graph_sgc_smooth_host>::call)};
yams_topology_artifacts_v1 g_topology_artifacts = {YAMS_IFACE_TOPOLOGY_ARTIFACTS_V1_VERSION, nullptr, GUARDED(ta_centroids),
                                                   GUARDED(ta_representatives), GUARDED(ta_residuals), GUARDED(free_arrays<float, uint32_t>),
                                                   GUARDED(free_arrays<uint32_t, uint32_t>), GUARDED(free_arrays<double, double, double>)};
yams_topology_route_v1 g_topology_route = {YAMS_IFACE_TOPOLOGY_ROUTE_V1_VERSION, nullptr, GUARDED(tr_index_create), GUARDED(tr_index_info),
                                           GUARDED(tr_dense), GUARDED(tr_index_destroy)};
yams_topology_quality_v1 g_topology_quality = {YAMS_IFACE_TOPOLOGY_QUALITY_V1_VERSION, nullptr, GUARDED(tq_persistence_h0),
                                               GUARDED(free_arrays<double, double>)};
yams_topology_features_v1 g_topology_features = {YAMS_IFACE_TOPOLOGY_FEATURES_V1_VERSION, nullptr, GUARDED(Leased<&yams_features_aggregate_host>::call), GUARDED(Leased<&yams_features_variance_host>::call),
                                                 GUARDED(Leased<&yams_features_compose_host>::call)};
yams_late_interaction_rerank_v1 g_late_rerank = {YAMS_IFACE_LATE_INTERACTION_RERANK_V1_VERSION, nullptr, GUARDED(Leased<&yams_rerank_maxsim_host>::call), GUARDED(Leased<&yams_rerank_maxpool_host>::call)};
yams_embedding_pool_v1 g_embedding_pool = {YAMS_IFACE_EMBEDDING_POOL_V1_VERSION, nullptr, GUARDED(Leased<&yams_embed_pool_host>::call), GUARDED(Leased<&yams_embed_normalize_host>::call),
                                           GUARDED(ep_pool_device), GUARDED(ep_normalize_device)};

void teardown_topology() { route_indexes.drain([](RouteIndex& e) { e.destroy(); }); }

} // namespace door
} // namespace yams_accel
