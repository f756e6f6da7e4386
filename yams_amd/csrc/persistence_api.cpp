// persistence_api.cpp — yams_quality_persistence_h0 (_device and _host): computePersistenceH0 over a point cloud behind the C
// ABI.  Order: the limits (no device needed, nothing allocated) -> argument checks -> ONE read-back of the check flags -> the
// workspace -> the work.  Nothing is written to an output before every refusal is known.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "accel_ctx.h"
#include "arg_checks.h"
#include "host_stage.h"
#include "persistence_launch.h"

using namespace yams_accel;

namespace {

static_assert(YAMS_QUALITY_MAX_POINTS == kPersistMaxPoints, "the header's limit is the launchers'");

struct Shape { uint32_t m; uint64_t edges; uint64_t index; };

// What needs no device.  *shape is filled on YAMS_OK.
yams_status_t check_args(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select,
                         uint32_t form, const yams_persistence_h0_t* out, Shape* shape) {
    const uint64_t m = select ? n_select : n;
    if (m > YAMS_QUALITY_MAX_POINTS) return fail(ctx, YAMS_ERR_UNSUPPORTED, "more than YAMS_QUALITY_MAX_POINTS points");
    if (dim > YAMS_CLUSTER_MAX_DIM) return fail(ctx, YAMS_ERR_UNSUPPORTED, "dim exceeds YAMS_CLUSTER_MAX_DIM");
    if (n >= (1ull << 31)) return fail(ctx, YAMS_ERR_UNSUPPORTED, "n must be < 2^31");
    if (dim == 0) return fail(ctx, YAMS_ERR_INVALID_ARG, "dim == 0");
    if (form != YAMS_RESIDUAL_SEPARATE && form != YAMS_RESIDUAL_FUSED) return fail(ctx, YAMS_ERR_INVALID_ARG, "unknown chain form");
    if (!out) return fail(ctx, YAMS_ERR_INVALID_ARG, "null out");
    if (m && !rows) return fail(ctx, YAMS_ERR_INVALID_ARG, "null rows");
    shape->m = static_cast<uint32_t>(m);
    shape->edges = m < 2 ? 0 : m * (m - 1) / 2;
    // percentile(), topological_quality.cpp:66-67, with q = 0.95, in the reference's own expression
    shape->index = shape->edges == 0 ? 0 : static_cast<size_t>(std::clamp(0.95 * static_cast<double>(shape->edges - 1), 0.0,
                                                                           static_cast<double>(shape->edges - 1)));
    return YAMS_OK;
}

// The call over device rows.  d_dist: a device [m][m] the distances are computed into, or null (the workspace then).  The
// merge weights come back sorted in h_weights (host, m - 1 values).  Synchronises.
yams_status_t run(yams_accel_ctx* ctx, const float* d_rows, uint64_t n, uint32_t dim, const uint32_t* d_select, const Shape& sh,
                  uint32_t form, yams_persistence_h0_t* res, double* d_dist, double** d_dist_used, std::vector<double>& h_weights,
                  float* out_stage_ms) {
    const uint32_t m = sh.m;
    hipStream_t st = ctx->stream;
    *res = yams_persistence_h0_t{};
    res->n_points = m;
    res->n_edges = sh.edges;
    res->norm_index = sh.index;
    h_weights.clear();
    if (d_dist_used) *d_dist_used = nullptr;
    if (m == 0) return YAMS_OK;
    uint32_t* d_flags; uint32_t flags;
    YA_TRY(flags_get(ctx, 4, &d_flags));
    YA_HIP(ctx, launch_persist_check(st, d_rows, n, dim, d_select, m, d_flags));
    YA_TRY(read_words(ctx, d_flags, 1, &flags));
    if (flags & kPersistFlagRange) return fail(ctx, YAMS_ERR_INVALID_ARG, "a select entry is out of range");
    if (flags & kPersistFlagNonFinite) return fail(ctx, YAMS_ERR_INVALID_ARG, "a selected row holds a non-finite value");

    double* d_mat = d_dist; uint32_t* d_hist; uint64_t* d_state; double* d_w; void* d_tree; uint64_t* h_pin;
    if (!d_mat) YA_TRY(ws_get(ctx, "persist_matrix", static_cast<size_t>(m) * m * 8, (void**)&d_mat));
    YA_TRY(ws_get(ctx, "persist_hist", kPersistSelectPasses * 256 * 4, (void**)&d_hist));
    YA_TRY(ws_get(ctx, "persist_state", kPersistSelectStateWords * 8, (void**)&d_state));
    YA_TRY(ws_get(ctx, "persist_weights", static_cast<size_t>(m) * 8, (void**)&d_w));
    YA_TRY(ws_get(ctx, "persist_tree", persist_tree_scratch_bytes(m), &d_tree));
    YA_TRY(pinned_get(ctx, 64 + static_cast<size_t>(m) * 8, (void**)&h_pin));      // [0]: the percentile's pattern, [8 ..]: the weights
    if (d_dist_used) *d_dist_used = d_mat;

    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto drop_events = [&] { for (auto& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } };
    if (out_stage_ms)
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) { drop_events(); return hip_fail(ctx, hipGetLastError(), "hipEventCreate"); }
    auto mark = [&](int i) { return out_stage_ms ? hipEventRecord(ev[i], st) : hipSuccess; };
    auto work = [&]() -> hipError_t {
        hipError_t e = mark(0);
        if (e == hipSuccess) e = launch_persist_pairs(st, d_rows, dim, d_select, m, form == YAMS_RESIDUAL_FUSED, d_mat);
        if (e == hipSuccess) e = mark(1);
        if (e == hipSuccess) e = launch_persist_select(st, d_mat, m, sh.index, d_hist, d_state);
        if (e == hipSuccess) e = mark(2);
        if (e == hipSuccess) e = launch_persist_tree(st, d_mat, m, d_w, d_tree);
        if (e == hipSuccess) e = mark(3);
        if (e == hipSuccess && m >= 2) {
            e = hipMemcpyAsync(h_pin, d_state, 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(h_pin + 8, d_w, static_cast<size_t>(m - 1) * 8, hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        return e;
    };
    const hipError_t e = work();
    if (e != hipSuccess) { drop_events(); return hip_fail(ctx, e, "persistence_h0"); }
    float stage[3] = {0.f, 0.f, 0.f};
    if (out_stage_ms) {
        for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&stage[i], ev[i], ev[i + 1]);
        drop_events();
    }
    if (m >= 2) {
        std::memcpy(&res->norm, h_pin, 8);
        h_weights.resize(m - 1);
        std::memcpy(h_weights.data(), h_pin + 8, static_cast<size_t>(m - 1) * 8);
        std::sort(h_weights.begin(), h_weights.end());
        // :103-126 — Kruskal's merges ascending are the tree's edges ascending; the heaviest (the essential class) is left out
        if (res->norm > 0.0) {
            double total = 0.0;
            for (uint32_t i = 0; i + 2 < m; ++i) total += h_weights[i] / res->norm;
            res->value = total;
            res->n_merges = m - 2;
        }
    }
    if (out_stage_ms) std::memcpy(out_stage_ms, stage, sizeof stage);
    return YAMS_OK;
}

} // namespace

extern "C" yams_status_t yams_quality_persistence_h0_device(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                            const uint32_t* select, uint64_t n_select, uint32_t form,
                                                            yams_persistence_h0_t* out, double* out_distances,
                                                            double* out_merge_weights, float* out_stage_ms) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    Shape sh{};
    YA_TRY(check_args(ctx, rows, n, dim, select, n_select, form, out, &sh));
    (void)hipSetDevice(ctx->device);
    yams_persistence_h0_t res{};
    std::vector<double> w;
    YA_TRY(run(ctx, rows, n, dim, select, sh, form, &res, out_distances, nullptr, w, out_stage_ms));
    if (out_merge_weights && !w.empty()) {
        YA_HIP(ctx, hipMemcpyAsync(out_merge_weights, w.data(), w.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        YA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *out = res;
    return YAMS_OK;
}

extern "C" yams_status_t yams_quality_persistence_h0_host(yams_accel_ctx* ctx, const float* rows, uint64_t n, uint32_t dim,
                                                          const uint32_t* select, uint64_t n_select, uint32_t form,
                                                          yams_persistence_h0_t* out, double* out_distances,
                                                          double* out_merge_weights, float* out_stage_ms) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    Shape sh{};
    YA_TRY(check_args(ctx, rows, n, dim, select, n_select, form, out, &sh));
    const uint32_t m = sh.m;
    if (select && !indices_below(select, m, n)) return fail(ctx, YAMS_ERR_INVALID_ARG, "a select entry is out of range");
    // only the selected rows travel, packed in the order given
    std::vector<float> packed;
    if (select && m) {
        packed.resize(static_cast<size_t>(m) * dim);
        gather_rows(rows, dim, select, m, packed.data());
    }
    HostStage hs(ctx);
    const float* d_rows = hs.up("persist_host_rows", packed.empty() ? rows : packed.data(), static_cast<size_t>(m) * dim);
    YA_TRY(m ? hs.finish() : hs.status());      // `packed` goes away (without points nothing was enqueued, and run() reads no row)
    yams_persistence_h0_t res{};
    std::vector<double> w;
    double* d_mat = nullptr;
    YA_TRY(run(ctx, d_rows, m, dim, nullptr, sh, form, &res, nullptr, &d_mat, w, out_stage_ms));
    if (out_distances && d_mat) {
        hs.down(out_distances, d_mat, static_cast<size_t>(m) * m);
        YA_TRY(hs.finish());
    }
    if (out_merge_weights && !w.empty()) std::memcpy(out_merge_weights, w.data(), w.size() * 8);
    *out = res;
    return YAMS_OK;
}
