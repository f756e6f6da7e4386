// route_kernels.hip — gfx950 kernels of the cluster router's dense signal (SparseGuidedClusterRouter::route).
//
// Reference semantics being reproduced (paths relative to the reference checkout; the contract is restated line by line in
// include/yams_mi355x_accel.h):
//   src/topology/topology_baseline.cpp:669-689   dotProduct / vectorNorm: one fp64 chain in element order, rounded to float
//                                                (norm: float(sqrt(chain)))
//   src/topology/topology_baseline.cpp:873-920   per candidate cluster: the centroid ASSIGNS dense when queryNorm > 0 and
//                                                centroidNorm > 0; representative positions below the limit fold with
//                                                std::max unless queryNorm <= 0 or representativeNorm <= 0
//
// Launches per call:
//   route_norm_kernel         float(sqrt(chain of squares)) of every query (and, at index build, of every index row): the
//                             staging and the chain of row_chains.h, no query
//   per slice of queries:
//   route_score_rows_kernel   1 to 8 queries: a lane owns an index row and carries one chain per query (row_chains.h as it
//                             is: 128-byte row chunks through LDS, the next chunk prefetched); a row no query of the group
//                             admits is never read
//   route_score_tile_kernel   more queries: the 128 x 64 fp64 tile of fp64_tile.h, A = index rows, B = queries
//                             Both apply the epilogue (float cast, one multiply, one divide, map, clamp) to the sums in
//                             registers and store one float per (query, row): the mapped cosine, or -1.0f where the
//                             reference evaluates nothing (the map's range is [0, 1] or NaN: -1.0f is free).
//   route_fold_kernel         one lane per (query, cluster) walks the cluster's segment (at most 65 floats) in row order
//
// The fold needs no float atomics and no order argument beyond this: a segment's row 0 is the centroid when the cluster has
// one, and only it ASSIGNS; every other row goes through max(cur, d) = (cur < d) ? d : cur.  If the centroid left a NaN, cur
// stays NaN whatever follows (NaN < d is false).  Otherwise cur is never a NaN (a NaN d fails cur < d), and the fold is the
// maximum of values in [0, 1] with no -0.0f among them ((cos + 1) * 0.5 of cos >= -1 is +0.0f at the least; a negative sum
// clamps to the literal +0.0f): the same whatever the order.  One lane walking the segment in row order is the reference's
// loop anyway.
//
// Float steps are spelled __fmul_rn / __fadd_rn / __fdiv_rn / __dsqrt_rn (no contraction, the correctly rounded divide and
// square root); the device code keeps f32 denormals (the kernel descriptors carry float_denorm_mode_32 = 3).
#include "common.h"
#include "fp64_tile.h"
#include "route_launch.h"
#include "row_chains.h"

namespace yams_accel {

constexpr float kRouteSkipped = -1.0f;

// :880-883 / :910-912 — float(dot) / (queryNorm * norm), mapped to [0, 1]; std::clamp's comparisons (a NaN passes through)
__device__ __forceinline__ float route_dense(double dot, float qn, float vn) {
    const float cosine = __fdiv_rn(static_cast<float>(dot), __fmul_rn(qn, vn));
    const float v = __fmul_rn(__fadd_rn(cosine, 1.0f), 0.5f);
    return (v < 0.0f) ? 0.0f : (1.0f < v) ? 1.0f : v;
}

// Does the reference evaluate (query, row)?  Centroid (:879): queryNorm > 0 && centroidNorm > 0, false for a NaN norm.
// Representative (:906): skipped only if queryNorm <= 0 || norm <= 0, so a NaN norm IS evaluated (and yields a NaN).
__device__ __forceinline__ bool route_evaluates(bool centroid, float qn, float vn) {
    return centroid ? (qn > 0.0f && vn > 0.0f) : !(qn <= 0.0f || vn <= 0.0f);
}

// Is the row inside what the query looks at: its cluster a candidate, its position below the limit (a centroid always is)
__device__ __forceinline__ bool route_admits(uint16_t pos, uint32_t pos_limit, const uint32_t* __restrict__ cand, uint32_t cand_words,
                                             uint32_t q, uint32_t cluster) {
    if (pos != kRouteCentroid && pos >= pos_limit) return false;
    return !cand || ((cand[static_cast<uint64_t>(q) * cand_words + (cluster >> 5)] >> (cluster & 31u)) & 1u);
}

__global__ __launch_bounds__(kRowThreads) void route_norm_kernel(const float* __restrict__ rows, uint64_t n, uint32_t dim, int vec4,
                                                                 float* __restrict__ norms) {
    __shared__ RowLdsRows s_rows;
    __shared__ RowLdsQueries<1> s_q;
    __shared__ RowLdsOrdinals s_row;
    const uint64_t row = static_cast<uint64_t>(blockIdx.x) * kRowThreads + threadIdx.x;
    const bool on = row < n;
    double nsq, dot[1];
    // n_slots = 0: no query is read, the query tile is zeros
    row_chains<1>(s_rows, s_q, s_row, on ? static_cast<uint32_t>(row) : kRowNone, rows, dim, vec4, rows, 0, 0, 0, on, nsq, dot);
    if (on) norms[row] = static_cast<float>(__dsqrt_rn(nsq));
}

template <int QG>
__global__ __launch_bounds__(kRowThreads) void route_score_rows_kernel(
    const float* __restrict__ vectors, const float* __restrict__ vnorm, const uint32_t* __restrict__ owner,
    const uint16_t* __restrict__ position, uint32_t n_rows, uint32_t dim, int vec4, const float* __restrict__ queries,
    const float* __restrict__ qnorm, uint32_t n_slots, uint32_t pos_limit, const uint32_t* __restrict__ cand, uint32_t cand_words,
    float* __restrict__ pair) {
    __shared__ RowLdsRows s_rows;
    __shared__ RowLdsQueries<QG> s_q;
    __shared__ RowLdsOrdinals s_row;
    const uint32_t slot0 = blockIdx.y * QG;
    const uint32_t row = blockIdx.x * kRowThreads + threadIdx.x;
    const bool in = row < n_rows;
    const uint16_t pos = in ? position[row] : kRouteCentroid;
    const uint32_t cluster = in ? owner[row] : 0u;
    const float vn = in ? vnorm[row] : 0.0f;
    uint32_t adm = 0;
#pragma unroll
    for (int j = 0; j < QG; ++j) {
        const uint32_t slot = slot0 + j;
        if (in && slot < n_slots && route_admits(pos, pos_limit, cand, cand_words, slot, cluster) &&
            route_evaluates(pos == kRouteCentroid, qnorm[slot], vn))
            adm |= 1u << j;
    }
    const bool on = adm != 0;   // a row no query of the group evaluates is never read
    double nsq, dot[QG];
    row_chains<QG>(s_rows, s_q, s_row, on ? row : kRowNone, vectors, dim, vec4, queries, 0, slot0, n_slots, on, nsq, dot);
    if (!in) return;
#pragma unroll
    for (int j = 0; j < QG; ++j) {
        const uint32_t slot = slot0 + j;
        if (slot < n_slots)
            pair[static_cast<uint64_t>(slot) * n_rows + row] = ((adm >> j) & 1u) ? route_dense(dot[j], qnorm[slot], vn) : kRouteSkipped;
    }
}

// Grid: x = one workgroup per 128 index rows, y = one per 64 queries.  Lane (ty, tx) owns rows ty*8 .. +7 and queries
// tx*4 .. +3; the epilogue runs on its 32 sums in registers.
template <bool VEC>
__global__ __launch_bounds__(kTileThreads, 2) void route_score_tile_kernel(
    const float* __restrict__ vectors, const float* __restrict__ vnorm, const uint32_t* __restrict__ owner,
    const uint16_t* __restrict__ position, uint32_t n_rows, uint32_t dim, const float* __restrict__ queries,
    const float* __restrict__ qnorm, uint32_t nq, uint32_t pos_limit, const uint32_t* __restrict__ cand, uint32_t cand_words,
    float* __restrict__ pair) {
    __shared__ __attribute__((aligned(16))) TileLdsA sa;
    __shared__ __attribute__((aligned(16))) TileLdsB sb;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const uint32_t row0 = blockIdx.x * kTileA, q0 = blockIdx.y * kTileB;
    const uint32_t a_row = row0 + tile_a_row(t), b_row = q0 + tile_b_row(t);
    const bool a_live = a_row < n_rows, b_live = b_row < nq;
    const float* a_src = vectors + static_cast<uint64_t>(a_live ? a_row : 0) * dim;
    const float* b_src = queries + static_cast<uint64_t>(b_live ? b_row : 0) * dim;
    double acc[kTileRB][kTileCB];
    tile_chains<VEC>(sa, sb, a_src, a_live, b_src, b_live, dim, acc);
#pragma unroll
    for (int i = 0; i < kTileRB; ++i) {
        const uint32_t row = row0 + ty * kTileRB + i;
        if (row >= n_rows) continue;
        const uint16_t pos = position[row];
        const uint32_t cluster = owner[row];
        const float vn = vnorm[row];
#pragma unroll
        for (int j = 0; j < kTileCB; ++j) {
            const uint32_t q = q0 + tx * kTileCB + j;
            if (q >= nq) continue;
            const float qn = qnorm[q];
            const bool ev = route_admits(pos, pos_limit, cand, cand_words, q, cluster) && route_evaluates(pos == kRouteCentroid, qn, vn);
            pair[static_cast<uint64_t>(q) * n_rows + row] = ev ? route_dense(acc[i][j], qn, vn) : kRouteSkipped;
        }
    }
}

// Grid: x over the clusters, y = the query of the slice.  :873-920 of one (query, cluster); the evaluations of a query are
// summed over a wave, then added to out_evals[q] (an integer: the order is free).
__global__ __launch_bounds__(256) void route_fold_kernel(const float* __restrict__ pair, const uint32_t* __restrict__ offsets,
                                                         const uint16_t* __restrict__ position, uint32_t n_rows, uint32_t n_clusters,
                                                         const uint32_t* __restrict__ cand, uint32_t cand_words,
                                                         float* __restrict__ out_dense, uint8_t* __restrict__ out_observed,
                                                         uint32_t* __restrict__ out_evals) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
    uint32_t evals = 0;
    if (c < n_clusters) {
        float cur = 0.0f;
        bool observed = false;
        if (!cand || ((cand[static_cast<uint64_t>(q) * cand_words + (c >> 5)] >> (c & 31u)) & 1u)) {
            const float* p = pair + static_cast<uint64_t>(q) * n_rows;
            const uint32_t end = offsets[c + 1];
            for (uint32_t r = offsets[c]; r < end; ++r) {
                const float d = p[r];
                if (d == kRouteSkipped) continue;
                cur = (position[r] == kRouteCentroid) ? d : ((cur < d) ? d : cur);
                observed = true;
                ++evals;
            }
        }
        out_dense[static_cast<uint64_t>(q) * n_clusters + c] = cur;
        out_observed[static_cast<uint64_t>(q) * n_clusters + c] = observed ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) evals += __shfl_xor(evals, o);
    if ((threadIdx.x & 63) == 0 && evals) atomicAdd(out_evals + q, evals);
}

hipError_t launch_route_norms(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, float* norms) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(route_norm_kernel, dim3(static_cast<uint32_t>((n + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0, st, rows, n,
                       dim, row_vec4_loads(rows, dim), norms);
    return hipGetLastError();
}

hipError_t launch_route_score(hipStream_t st, const float* vectors, const float* vnorm, const uint32_t* owner, const uint16_t* position,
                              uint32_t n_rows, uint32_t dim, const float* queries, const float* qnorm, uint32_t nq, uint32_t pos_limit,
                              const uint32_t* cand, uint32_t cand_words, float* pair) {
    if (n_rows == 0 || nq == 0) return hipSuccess;
    if (nq <= kRouteRowsFormMax) {
        const int vec4 = row_vec4_loads(vectors, dim);
        row_chains_dispatch(n_rows, nq, [&](auto qg, dim3 grid) {
            hipLaunchKernelGGL((route_score_rows_kernel<decltype(qg)::value>), grid, dim3(kRowThreads), 0, st, vectors, vnorm, owner, position,
                               n_rows, dim, vec4, queries, qnorm, nq, pos_limit, cand, cand_words, pair);
        });
    } else {
        const dim3 grid((n_rows + kTileA - 1) / kTileA, (nq + kTileB - 1) / kTileB);
        if (tile_vec_loads(dim, vectors, queries))
            hipLaunchKernelGGL((route_score_tile_kernel<true>), grid, dim3(kTileThreads), 0, st, vectors, vnorm, owner, position, n_rows, dim,
                               queries, qnorm, nq, pos_limit, cand, cand_words, pair);
        else
            hipLaunchKernelGGL((route_score_tile_kernel<false>), grid, dim3(kTileThreads), 0, st, vectors, vnorm, owner, position, n_rows, dim,
                               queries, qnorm, nq, pos_limit, cand, cand_words, pair);
    }
    return hipGetLastError();
}

hipError_t launch_route_fold(hipStream_t st, const float* pair, const uint32_t* offsets, const uint16_t* position, uint32_t n_rows,
                             uint32_t n_clusters, uint32_t nq, const uint32_t* cand, uint32_t cand_words, float* out_dense,
                             uint8_t* out_observed, uint32_t* out_evals) {
    if (n_clusters == 0 || nq == 0) return hipSuccess;
    hipLaunchKernelGGL(route_fold_kernel, dim3((n_clusters + 255) / 256, nq), dim3(256), 0, st, pair, offsets, position, n_rows, n_clusters,
                       cand, cand_words, out_dense, out_observed, out_evals);
    return hipGetLastError();
}

} // namespace yams_accel
