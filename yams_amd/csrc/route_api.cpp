// route_api.cpp — yams_route_index_create / _destroy / _info and yams_route_dense (_device and _host): the dense signal of
// SparseGuidedClusterRouter::route over a resident table of cluster vectors, behind the C ABI.  Every entry: argument checks
// -> the checks that need the small arrays (on host copies of them) -> the work.  Nothing is written to an output, and no
// index is handed out, before the refusals are known.
#include <algorithm>
#include <cstring>
#include <vector>

#include "accel_ctx.h"
#include "host_stage.h"
#include "route_launch.h"

using namespace yams_accel;

struct yams_route_index {
    yams_accel_ctx* ctx = nullptr;
    uint32_t n_vectors = 0, n_clusters = 0, dim = 0;
    size_t bytes = 0;
    char* base = nullptr;            // one allocation: the five arrays below
    float* vectors = nullptr;        // [n_vectors][dim], 256-byte aligned
    float* norms = nullptr;          // [n_vectors]
    uint32_t* offsets = nullptr;     // [n_clusters + 1]
    uint32_t* owner = nullptr;       // [n_vectors]: the cluster of every row
    uint16_t* position = nullptr;    // [n_vectors]: kRouteCentroid for a centroid row
};

namespace {

constexpr size_t kHostOutBytes = 256ull << 20;   // what a _host call's outputs may occupy on the device at a time
constexpr size_t kPairBytes = 256ull << 20;      // what the (query, row) values of one slice may occupy

size_t up256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

// The checks of create, on host copies of the small arrays; fills owner / pos (the index's own row tables).
yams_status_t check_table(yams_accel_ctx* ctx, uint64_t v, uint32_t dim, uint32_t c, const uint32_t* off, const uint8_t* has,
                          const uint16_t* position, std::vector<uint32_t>& owner, std::vector<uint16_t>& pos) {
    if (off[0] != 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "cluster_offsets do not start at 0");
    owner.resize(v ? v : 1);
    pos.resize(v ? v : 1);
    for (uint32_t k = 0; k < c; ++k) {
        if (off[k + 1] < off[k] || off[k + 1] > v) return fail(ctx, YAMS_ERR_INVALID_ARG, "cluster_offsets decrease or pass n_vectors");
        const uint32_t size = off[k + 1] - off[k], cen = has[k] ? 1u : 0u;
        if (cen > size) return fail(ctx, YAMS_ERR_INVALID_ARG, "a cluster without rows is flagged as having a centroid");
        if (size - cen > YAMS_ROUTE_MAX_REPRESENTATIVES)
            return fail(ctx, YAMS_ERR_INVALID_ARG, "a cluster has more than YAMS_ROUTE_MAX_REPRESENTATIVES representatives");
        for (uint32_t r = off[k]; r < off[k + 1]; ++r) {
            owner[r] = k;
            if (cen && r == off[k]) { pos[r] = kRouteCentroid; continue; }
            if (position[r] == kRouteCentroid) return fail(ctx, YAMS_ERR_INVALID_ARG, "a representative's position is 0xffff");
            pos[r] = position[r];
        }
    }
    if (off[c] != v) return fail(ctx, YAMS_ERR_INVALID_ARG, "cluster_offsets do not end at n_vectors");
    return YAMS_OK;
}

yams_status_t check_create_args(yams_accel_ctx* ctx, const float* vectors, uint64_t v, uint32_t dim, const uint32_t* off, const uint8_t* has,
                                const uint16_t* position, uint32_t c, yams_route_index** out) {
    if (dim == 0 || dim > YAMS_ROUTE_MAX_DIM) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim must be in [1, YAMS_ROUTE_MAX_DIM]");
    if (c > YAMS_ROUTE_MAX_CLUSTERS) return fail(ctx, YAMS_ERR_INVALID_ARG, "n_clusters exceeds YAMS_ROUTE_MAX_CLUSTERS");
    if (v > static_cast<uint64_t>(c) * (YAMS_ROUTE_MAX_REPRESENTATIVES + 1)) return fail(ctx, YAMS_ERR_INVALID_ARG, "more vectors than the clusters can hold");
    if (!out || !off || (c && !has) || (v && (!vectors || !position))) return fail(ctx, YAMS_ERR_INVALID_ARG, "null array or out_index");
    return YAMS_OK;
}

// Allocates the index, fills it (vectors from `vectors` with `kind`, the row tables from the host vectors) and computes the norms.
yams_status_t build_index(yams_accel_ctx* ctx, const float* vectors, hipMemcpyKind kind, uint64_t v64, uint32_t dim, uint32_t c,
                          const uint32_t* off, const std::vector<uint32_t>& owner, const std::vector<uint16_t>& pos,
                          yams_route_index** out_index) {
    const uint32_t v = static_cast<uint32_t>(v64);
    const size_t v1 = v ? v : 1;
    const size_t b_vec = up256(v1 * dim * 4), b_norm = up256(v1 * 4), b_off = up256((static_cast<size_t>(c) + 1) * 4),
                 b_own = up256(v1 * 4), b_pos = up256(v1 * 2);
    auto* ix = new yams_route_index();
    ix->ctx = ctx; ix->n_vectors = v; ix->n_clusters = c; ix->dim = dim;
    ix->bytes = b_vec + b_norm + b_off + b_own + b_pos;
    (void)hipSetDevice(ctx->device);
    hipError_t e = ya_malloc(reinterpret_cast<void**>(&ix->base), ix->bytes);
    if (e != hipSuccess) {
        delete ix;
        (void)hipGetLastError();
        return fail(ctx, YAMS_ERR_RESOURCE_EXHAUSTED, "device memory for the route index could not be had");
    }
    char* p = ix->base;
    ix->vectors = reinterpret_cast<float*>(p); p += b_vec;
    ix->norms = reinterpret_cast<float*>(p); p += b_norm;
    ix->offsets = reinterpret_cast<uint32_t*>(p); p += b_off;
    ix->owner = reinterpret_cast<uint32_t*>(p); p += b_own;
    ix->position = reinterpret_cast<uint16_t*>(p);
    hipStream_t st = ctx->stream;
    auto run = [&]() -> hipError_t {
        hipError_t r = hipSuccess;
        if (v) {
            r = kind == hipMemcpyHostToDevice ? staged_h2d(ix->vectors, vectors, static_cast<size_t>(v) * dim * 4, st)
                                              : hipMemcpyAsync(ix->vectors, vectors, static_cast<size_t>(v) * dim * 4, kind, st);
            if (r == hipSuccess) r = hipMemcpyAsync(ix->owner, owner.data(), static_cast<size_t>(v) * 4, hipMemcpyHostToDevice, st);
            if (r == hipSuccess) r = hipMemcpyAsync(ix->position, pos.data(), static_cast<size_t>(v) * 2, hipMemcpyHostToDevice, st);
        }
        if (r == hipSuccess) r = hipMemcpyAsync(ix->offsets, off, (static_cast<size_t>(c) + 1) * 4, hipMemcpyHostToDevice, st);
        if (r == hipSuccess) r = launch_route_norms(st, ix->vectors, v, dim, ix->norms);
        if (r == hipSuccess) r = hipStreamSynchronize(st);     // the host vectors are the caller's stack
        return r;
    };
    e = run();
    if (e != hipSuccess) {
        (void)hipFree(ix->base);
        delete ix;
        return hip_fail(ctx, e, "route index build");
    }
    *out_index = ix;
    return YAMS_OK;
}

} // namespace

extern "C" yams_status_t yams_route_index_create_host(yams_accel_ctx* ctx, const float* vectors, uint64_t n_vectors, uint32_t dim,
                                                      const uint32_t* cluster_offsets, const uint8_t* has_centroid,
                                                      const uint16_t* position, uint32_t n_clusters, yams_route_index** out_index,
                                                      float* out_norms) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_create_args(ctx, vectors, n_vectors, dim, cluster_offsets, has_centroid, position, n_clusters, out_index));
    std::vector<uint32_t> owner;
    std::vector<uint16_t> pos;
    YA_TRY(check_table(ctx, n_vectors, dim, n_clusters, cluster_offsets, has_centroid, position, owner, pos));
    yams_route_index* ix = nullptr;
    YA_TRY(build_index(ctx, vectors, hipMemcpyHostToDevice, n_vectors, dim, n_clusters, cluster_offsets, owner, pos, &ix));
    if (out_norms && n_vectors) {
        hipError_t e = hipMemcpyAsync(out_norms, ix->norms, static_cast<size_t>(n_vectors) * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { yams_route_index_destroy(ix); return hip_fail(ctx, e, "route index norms"); }
    }
    *out_index = ix;
    return YAMS_OK;
}

extern "C" yams_status_t yams_route_index_create_device(yams_accel_ctx* ctx, const float* vectors, uint64_t n_vectors, uint32_t dim,
                                                        const uint32_t* cluster_offsets, const uint8_t* has_centroid,
                                                        const uint16_t* position, uint32_t n_clusters, yams_route_index** out_index,
                                                        float* out_norms) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    YA_TRY(check_create_args(ctx, vectors, n_vectors, dim, cluster_offsets, has_centroid, position, n_clusters, out_index));
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    // the small arrays come to the host: the checks and the row tables are made there
    std::vector<uint32_t> off(static_cast<size_t>(n_clusters) + 1);
    std::vector<uint8_t> has(n_clusters ? n_clusters : 1);
    std::vector<uint16_t> position_h(n_vectors ? n_vectors : 1);
    YA_HIP(ctx, hipMemcpyAsync(off.data(), cluster_offsets, off.size() * 4, hipMemcpyDeviceToHost, st));
    if (n_clusters) YA_HIP(ctx, hipMemcpyAsync(has.data(), has_centroid, n_clusters, hipMemcpyDeviceToHost, st));
    if (n_vectors) YA_HIP(ctx, hipMemcpyAsync(position_h.data(), position, static_cast<size_t>(n_vectors) * 2, hipMemcpyDeviceToHost, st));
    YA_HIP(ctx, hipStreamSynchronize(st));
    std::vector<uint32_t> owner;
    std::vector<uint16_t> pos;
    YA_TRY(check_table(ctx, n_vectors, dim, n_clusters, off.data(), has.data(), position_h.data(), owner, pos));
    yams_route_index* ix = nullptr;
    YA_TRY(build_index(ctx, vectors, hipMemcpyDeviceToDevice, n_vectors, dim, n_clusters, off.data(), owner, pos, &ix));
    if (out_norms && n_vectors) {
        hipError_t e = hipMemcpyAsync(out_norms, ix->norms, static_cast<size_t>(n_vectors) * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { yams_route_index_destroy(ix); return hip_fail(ctx, e, "route index norms"); }
    }
    *out_index = ix;
    return YAMS_OK;
}

extern "C" void yams_route_index_destroy(yams_route_index* index) {
    if (!index) return;
    (void)hipSetDevice(index->ctx->device);
    (void)hipStreamSynchronize(index->ctx->stream);
    (void)hipFree(index->base);
    delete index;
}

extern "C" yams_status_t yams_route_index_info(const yams_route_index* index, yams_route_index_info_t* out_info) {
    if (!index || !out_info) return YAMS_ERR_INVALID_ARG;
    out_info->n_vectors = index->n_vectors;
    out_info->n_clusters = index->n_clusters;
    out_info->dim = index->dim;
    out_info->bytes = index->bytes;
    return YAMS_OK;
}

namespace {

yams_status_t check_dense_args(yams_route_index* ix, const float* queries, uint32_t nq, const float* out_dense, const uint8_t* out_observed,
                               const uint32_t* out_evals) {
    if (nq > YAMS_ROUTE_MAX_QUERIES) return fail(ix->ctx, YAMS_ERR_INVALID_ARG, "n_queries exceeds YAMS_ROUTE_MAX_QUERIES");
    if (nq && (!queries || !out_evals || (ix->n_clusters && (!out_dense || !out_observed))))
        return fail(ix->ctx, YAMS_ERR_INVALID_ARG, "null queries or output");
    return YAMS_OK;
}

} // namespace

extern "C" yams_status_t yams_route_dense_device(yams_route_index* ix, const float* queries, uint32_t nq, uint32_t rep_limit,
                                                 const uint32_t* candidates, float* out_dense, uint8_t* out_observed,
                                                 uint32_t* out_evals, yams_route_diag_t* diag) {
    if (!ix) return YAMS_ERR_INVALID_ARG;
    yams_accel_ctx* ctx = ix->ctx;
    YA_TRY(check_dense_args(ix, queries, nq, out_dense, out_observed, out_evals));
    if (diag) *diag = yams_route_diag_t{};
    if (nq == 0) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t v = ix->n_vectors, c = ix->n_clusters, words = (c + 31) / 32;
    // positions < pos_limit are looked at: the whole list (positions are < 0xffff), or maxRoutingRepresentatives - 1
    const uint32_t pos_limit = rep_limit == 0 ? kRouteCentroid : std::min<uint32_t>(rep_limit - 1, kRouteCentroid);
    // slices of queries whose (query, row) values fit kPairBytes
    const uint32_t per = static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(nq, kPairBytes / (static_cast<size_t>(v ? v : 1) * 4))));
    float* d_qnorm; float* d_pair;
    YA_TRY(ws_get(ctx, "route_qnorm", static_cast<size_t>(nq) * 4, (void**)&d_qnorm));
    YA_TRY(ws_get(ctx, "route_pair", static_cast<size_t>(per) * (v ? v : 1) * 4, (void**)&d_pair));
    TimedRegion tr(ctx, "route_dense");
    hipError_t e = hipMemsetAsync(out_evals, 0, static_cast<size_t>(nq) * 4, st);
    if (e == hipSuccess) e = launch_route_norms(st, queries, nq, ix->dim, d_qnorm);
    for (uint32_t q0 = 0; q0 < nq && e == hipSuccess; q0 += per) {
        const uint32_t m = std::min(per, nq - q0);
        const uint32_t* cand = candidates ? candidates + static_cast<size_t>(q0) * words : nullptr;
        e = launch_route_score(st, ix->vectors, ix->norms, ix->owner, ix->position, v, ix->dim, queries + static_cast<size_t>(q0) * ix->dim,
                               d_qnorm + q0, m, pos_limit, cand, words, d_pair);
        if (e == hipSuccess)
            e = launch_route_fold(st, d_pair, ix->offsets, ix->position, v, c, m, cand, words, out_dense + static_cast<size_t>(q0) * c,
                                  out_observed + static_cast<size_t>(q0) * c, out_evals + q0);
        if (diag) {
            diag->pairs += static_cast<uint64_t>(m) * v;
            diag->slices += 1;
            diag->form = m <= kRouteRowsFormMax ? 0u : 1u;
        }
    }
    tr.end();
    YA_HIP(ctx, e);
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

extern "C" yams_status_t yams_route_dense_host(yams_route_index* ix, const float* queries, uint32_t nq, uint32_t rep_limit,
                                               const uint32_t* candidates, float* out_dense, uint8_t* out_observed,
                                               uint32_t* out_evals, yams_route_diag_t* diag) {
    if (!ix) return YAMS_ERR_INVALID_ARG;
    yams_accel_ctx* ctx = ix->ctx;
    YA_TRY(check_dense_args(ix, queries, nq, out_dense, out_observed, out_evals));
    if (diag) *diag = yams_route_diag_t{};
    if (nq == 0) return YAMS_OK;
    HostStage hs(ctx);
    const uint32_t c = ix->n_clusters, words = (c + 31) / 32;
    // slices of queries whose outputs (dense, observed, evals) fit kHostOutBytes
    const uint32_t per = static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(nq, kHostOutBytes / (static_cast<size_t>(c ? c : 1) * 5 + 4))));
    const float* d_q = hs.up("route_host_queries", queries, static_cast<size_t>(nq) * ix->dim);
    // (without clusters a candidate set has no words: it stays a null pointer, as it is for the device twin's callers)
    const uint32_t* d_cand = words ? hs.up("route_host_candidates", candidates, static_cast<size_t>(nq) * words) : nullptr;
    float* d_dense = hs.room<float>("route_host_dense", static_cast<size_t>(per) * c);
    uint8_t* d_obs = hs.room<uint8_t>("route_host_observed", static_cast<size_t>(per) * c);
    uint32_t* d_evals = hs.room<uint32_t>("route_host_evals", per);
    YA_TRY(hs.status());
    for (uint32_t q0 = 0; q0 < nq; q0 += per) {
        const uint32_t m = std::min(per, nq - q0);
        yams_route_diag_t d{};
        YA_TRY(yams_route_dense_device(ix, d_q + static_cast<size_t>(q0) * ix->dim, m, rep_limit,
                                       d_cand ? d_cand + static_cast<size_t>(q0) * words : nullptr, d_dense, d_obs, d_evals, &d));
        if (diag) { diag->pairs += d.pairs; diag->slices += d.slices; diag->form = d.form; }
        if (c) {
            hs.down(out_dense + static_cast<size_t>(q0) * c, d_dense, static_cast<size_t>(m) * c);
            hs.down(out_observed + static_cast<size_t>(q0) * c, d_obs, static_cast<size_t>(m) * c);
        }
        hs.down(out_evals + q0, d_evals, m);
        YA_TRY(hs.finish());
    }
    return YAMS_OK;
}
