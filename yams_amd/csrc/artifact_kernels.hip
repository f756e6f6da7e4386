// artifact_kernels.hip — gfx950 kernels of the tail every topology engine runs after clustering: centroids, routing
// representatives, the residual chains of the boundary spill.
//
// Reference semantics being reproduced (paths relative to the reference checkout):
//   src/topology/topology_build_utils.h:27-56            meanEmbedding: fp32 running sum over the members IN LIST ORDER, / float(count),
//                                                        no normalisation
//   src/topology/topology_representatives.cpp:13-29      cosineDistance: three fp64 chains in element order (cosine_tail.h has the tail)
//   :58-90                                               farthest-first selection inside a cluster: minDist = std::min(minDist, d) over
//                                                        the unused candidates, the first strictly largest minDist wins
//   :119-141, :189-198, :235-252                         residual = double(e) - double(c); normSq += residual * residual;
//                                                        residualDot += primaryResidual * residual
//
// Exactness.  A chain is one lane's, walks its elements in the reference's order and is never split.  The products of the cosine
// chains are exact in fp64 (fp64_tile.h has the argument), so fma is the reference's `+=` there.  The residual products are NOT
// exact: the bits depend on whether the host's compiler contracted `x += a * b`, so both forms exist, written with explicit
// intrinsics (and contraction is off for this file besides): SEPARATE = __dmul_rn then __dadd_rn, FUSED = one fma per `+=`.
// Elements past `dim` are staged as +0.0: residual 0, product +0, and a chain that starts at +0.0 never holds -0.0, so adding
// +0 changes nothing, NaN and infinities included.
//
// Kernels:
//   artifact_check_offsets / _check_index    the argument checks that need the arrays
//   artifact_centroid_kernel      one fp32 chain per (cluster, dimension): a workgroup owns 256 dimensions of one cluster
//   artifact_owner_kernel         the list (cluster / document) every entry of a flat array belongs to
//   artifact_rep_init / _dist / _pick   the selection: per pass one launch over ALL candidates (one lane per candidate, its row
//                                 staged through LDS, the cluster's centroid or last winner read directly), then one workgroup per
//                                 cluster takes the strictly largest minDist at the lowest list position
//   artifact_residual_dense_kernel   64 documents x 64 clusters per workgroup, 4 x 4 pairs x 2 chains per lane, operands staged in
//                                 LDS as fp64 (the primary residual is formed while staging: the same single rounded subtraction)
//   artifact_residual_pairs_kernel   one lane per listed (document, cluster) pair, the three rows gathered through LDS; also the
//                                 primary norm (one lane per document)
#pragma clang fp contract(off)
#include <cfloat>

#include "common.h"
#include "artifact_launch.h"
#include "cosine_tail.h"
#include "form_step.h"
#include "row_walk.h"

namespace yams_accel {

namespace {

constexpr int kArThreads = 256;
constexpr uint32_t kArNone = 0xffffffffu;
static_assert(kArThreads == kRwRows, "the row walk is built for this workgroup");

// Stages elements [d0, d0 + 16) of the rows idx[0 .. 256) of `base` into tile (zero-filled for idx == kArNone and past dim):
// rw_stage_rows with a gather.  The caller puts a barrier before and after.
__device__ __forceinline__ void ar_stage_gather(const float* __restrict__ base, uint32_t dim, const uint32_t* idx, uint32_t d0,
                                                RowWalkTile& tile) {
    const int t = threadIdx.x, dc = t & 15;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = (t >> 4) + 16 * i;
        const uint32_t row = idx[r];
        tile[r][dc] = (row != kArNone && d0 + dc < dim) ? base[static_cast<uint64_t>(row) * dim + d0 + dc] : 0.0f;
    }
}

} // namespace

// flags |= 1 unless off[0] == 0 and off[i] <= off[i + 1] <= total for i < count
__global__ __launch_bounds__(kArThreads) void artifact_check_offsets_kernel(const uint64_t* __restrict__ off, uint64_t count, uint64_t total,
                                                                            uint32_t* __restrict__ flags) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kArThreads + threadIdx.x;
    if (i >= count) return;
    const uint64_t a = off[i], b = off[i + 1];
    if (a > b || b > total || (i == 0 && a != 0)) atomicOr(flags, 1u);
}

// flags |= 2 when an index is >= limit (none_ok: kArNone passes)
__global__ __launch_bounds__(kArThreads) void artifact_check_index_kernel(const uint32_t* __restrict__ idx, uint64_t count, uint32_t limit,
                                                                          int none_ok, uint32_t* __restrict__ flags) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kArThreads + threadIdx.x;
    if (i >= count) return;
    const uint32_t v = idx[i];
    if (v >= limit && !(none_ok && v == kArNone)) atomicOr(flags, 2u);
}

// owner[p] = the list p belongs to: the i with off[i] <= p < off[i + 1] (off checked; empty lists own nothing)
__global__ __launch_bounds__(kArThreads) void artifact_owner_kernel(const uint64_t* __restrict__ off, uint32_t lists, uint64_t total,
                                                                    uint32_t* __restrict__ owner) {
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kArThreads + threadIdx.x;
    if (p >= total) return;
    uint32_t lo = 0, hi = lists - 1;      // the first i with off[i + 1] > p; one exists because p < off[lists]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid + 1] > p) hi = mid; else lo = mid + 1;
    }
    owner[p] = lo;
}

// meanEmbedding (h:27-56) of cluster blockIdx.x, dimensions blockIdx.y * 256 ..: s = 0.0f + row[m0][d] + row[m1][d] + ... in the
// order of the member list, / float(count), the IEEE divide.  A cluster without members has no centroid: count 0, zeros.
__global__ __launch_bounds__(kArThreads) void artifact_centroid_kernel(const float* __restrict__ x, uint32_t dim,
                                                                       const uint64_t* __restrict__ off, const uint32_t* __restrict__ members,
                                                                       float* __restrict__ out, uint32_t* __restrict__ out_counts) {
    const uint32_t c = blockIdx.x;
    const uint32_t d = blockIdx.y * kArThreads + threadIdx.x;
    const uint64_t lo = off[c];
    const uint32_t cnt = static_cast<uint32_t>(off[c + 1] - lo);
    if (blockIdx.y == 0 && threadIdx.x == 0) out_counts[c] = cnt;
    if (d >= dim) return;
    const uint32_t* list = members + lo;
    float s = 0.0f;
#pragma unroll 4
    for (uint32_t m = 0; m < cnt; ++m) s += x[static_cast<uint64_t>(list[m]) * dim + d];
    out[static_cast<uint64_t>(c) * dim + d] = cnt ? s / static_cast<float>(cnt) : 0.0f;
}

// limit[c] = extraLimit (:58-59) = min(n_extra, candidates), 0 for a cluster whose centroid is empty (:37)
__global__ __launch_bounds__(kArThreads) void artifact_rep_init_kernel(const uint64_t* __restrict__ off, uint32_t c,
                                                                       const uint8_t* __restrict__ centroid_empty, uint32_t n_extra,
                                                                       uint32_t* __restrict__ limit, uint32_t* __restrict__ last) {
    const uint32_t i = blockIdx.x * kArThreads + threadIdx.x;
    if (i >= c) return;
    const uint64_t size = off[i + 1] - off[i];
    limit[i] = (centroid_empty && centroid_empty[i]) ? 0u : static_cast<uint32_t>(size < n_extra ? size : n_extra);
    last[i] = 0;
}

// Pass `s` of the selection (:67-75) for every unused candidate of every cluster that still selects: d = cosineDistance(candidate,
// s == 0 ? centroid : last selected); minDist = std::min(minDist, d) (b < a ? b : a: a NaN d leaves it).
__global__ __launch_bounds__(kArThreads) void artifact_rep_dist_kernel(const float* __restrict__ x, uint32_t dim,
                                                                       const double2* __restrict__ row_norm, const uint64_t* __restrict__ off,
                                                                       const uint32_t* __restrict__ cand, const uint32_t* __restrict__ owner,
                                                                       uint64_t total, const float* __restrict__ cents,
                                                                       const double2* __restrict__ cent_norm, const uint32_t* __restrict__ limit,
                                                                       const uint32_t* __restrict__ last, uint32_t s,
                                                                       const uint8_t* __restrict__ used, double* __restrict__ min_dist) {
    __shared__ RowWalkTile tile;
    __shared__ uint32_t s_row[kArThreads];
    const int t = threadIdx.x;
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kArThreads + t;
    uint32_t row = kArNone, cl = 0;
    if (p < total) {
        cl = owner[p];
        if (s < limit[cl] && !used[p]) row = cand[p];
    }
    const bool live = row != kArNone;
    s_row[t] = row;
    if (!__syncthreads_or(live)) return;
    const float* tv = cents;
    double2 nb = make_double2(0.0, 0.0);
    if (live) {
        if (s == 0) {
            tv = cents + static_cast<uint64_t>(cl) * dim;
            nb = cent_norm[cl];
        } else {
            const uint32_t lr = cand[off[cl] + last[cl]];
            tv = x + static_cast<uint64_t>(lr) * dim;
            nb = row_norm[lr];
        }
    }
    double dot = 0.0;
    for (uint32_t d0 = 0; d0 < dim; d0 += kRwChunk) {
        __syncthreads();
        ar_stage_gather(x, dim, s_row, d0, tile);
        __syncthreads();
        if (live) {
#pragma unroll
            for (int e = 0; e < kRwChunk; ++e) {
                const float b = (d0 + e < dim) ? tv[d0 + e] : 0.0f;
                dot = fma(static_cast<double>(tile[t][e]), static_cast<double>(b), dot);
            }
        }
    }
    if (!live) return;
    const double2 na = row_norm[row];
    const double d = km_distance(dot, na.x, na.y, nb.x, nb.y);
    if (d < min_dist[p]) min_dist[p] = d;
}

// The end of pass `s` for cluster blockIdx.x (:66-88): among the unused candidates, the first in list order whose minDist is
// strictly the largest (bestDistance starts at -1.0; a minDist is never NaN and never below 0).  It becomes used, the cluster's
// last selected, and out_selected[cluster][s].
__global__ __launch_bounds__(kArThreads) void artifact_rep_pick_kernel(const uint64_t* __restrict__ off, const uint32_t* __restrict__ limit,
                                                                       uint32_t s, uint32_t n_extra, uint8_t* __restrict__ used,
                                                                       const double* __restrict__ min_dist, uint32_t* __restrict__ last,
                                                                       uint32_t* __restrict__ out_selected) {
    __shared__ double r_val[kArThreads];
    __shared__ uint32_t r_idx[kArThreads];
    const uint32_t cl = blockIdx.x;
    if (s >= limit[cl]) return;
    const int t = threadIdx.x;
    const uint64_t lo = off[cl];
    const uint32_t size = static_cast<uint32_t>(off[cl + 1] - lo);
    double val = -1.0;
    uint32_t idx = kArNone;
    for (uint32_t i = t; i < size; i += kArThreads) {
        if (used[lo + i]) continue;
        const double m = min_dist[lo + i];
        if (m > val) { val = m; idx = i; }
    }
    r_val[t] = val; r_idx[t] = idx;
    __syncthreads();
    for (int h = kArThreads / 2; h > 0; h >>= 1) {
        if (t < h && (r_val[t + h] > r_val[t] || (r_val[t + h] == r_val[t] && r_idx[t + h] < r_idx[t]))) {
            r_val[t] = r_val[t + h]; r_idx[t] = r_idx[t + h];
        }
        __syncthreads();
    }
    if (t == 0 && r_idx[0] != kArNone) {
        used[lo + r_idx[0]] = 1;
        last[cl] = r_idx[0];
        out_selected[static_cast<uint64_t>(cl) * n_extra + s] = r_idx[0];
    }
}

// ---- residuals ------------------------------------------------------------------------------------------------------------
constexpr int kRsTile = 64, kRsChunk = 8, kRsBlock = 4;      // documents = clusters per workgroup, dimensions per stage, per lane
constexpr int kRsLd = kRsTile + 2;                           // LDS stride in doubles (rows stay 16-byte aligned)

// Every cluster for every document (:214-252 without an index): out_norm / out_dot [doc][c].  Lane (ty, tx) of 16 x 16 owns
// documents ty*4 .. +3 and clusters tx*4 .. +3.  Staging: thread t loads dimensions (t%4)*2 .. +1 of the chunk of document t/4,
// of that document's primary centroid and of cluster t/4.
template <bool FUSED>
__global__ __launch_bounds__(kArThreads) void artifact_residual_dense_kernel(const float* __restrict__ x, uint64_t n, uint32_t dim,
                                                                             const float* __restrict__ cents, uint32_t c,
                                                                             const uint32_t* __restrict__ primary,
                                                                             double* __restrict__ out_norm, double* __restrict__ out_dot) {
    __shared__ __attribute__((aligned(16))) double se[kRsChunk][kRsLd];      // double(e)
    __shared__ __attribute__((aligned(16))) double sp[kRsChunk][kRsLd];      // primaryResidual
    __shared__ __attribute__((aligned(16))) double sc[kRsChunk][kRsLd];      // double(c)
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const uint64_t doc0 = static_cast<uint64_t>(blockIdx.x) * kRsTile;
    const uint32_t cl0 = blockIdx.y * kRsTile;
    const int sr = t >> 2, sd = (t & 3) * 2;
    const uint64_t sdoc = doc0 + sr;
    const bool d_live = sdoc < n;
    const uint32_t pr = (d_live && primary) ? primary[sdoc] : kArNone;
    const bool p_live = pr != kArNone;
    const bool c_live = cl0 + sr < c;
    const float* e_src = x + (d_live ? sdoc : 0) * dim;
    const float* p_src = cents + static_cast<uint64_t>(p_live ? pr : 0) * dim;
    const float* c_src = cents + static_cast<uint64_t>(c_live ? cl0 + sr : 0) * dim;

    double an[kRsBlock][kRsBlock], ad[kRsBlock][kRsBlock];
#pragma unroll
    for (int i = 0; i < kRsBlock; ++i)
#pragma unroll
        for (int j = 0; j < kRsBlock; ++j) { an[i][j] = 0.0; ad[i][j] = 0.0; }

    for (uint32_t d0 = 0; d0 < dim; d0 += kRsChunk) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const uint32_t dd = d0 + sd + e;
            const bool in = dd < dim;
            const double ev = (d_live && in) ? static_cast<double>(e_src[dd]) : 0.0;
            const double pv = (p_live && in) ? static_cast<double>(p_src[dd]) : 0.0;
            se[sd + e][sr] = ev;
            sp[sd + e][sr] = (p_live && in) ? __dsub_rn(ev, pv) : 0.0;
            sc[sd + e][sr] = (c_live && in) ? static_cast<double>(c_src[dd]) : 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int e = 0; e < kRsChunk; ++e) {
            double a[kRsBlock], q[kRsBlock], b[kRsBlock];
#pragma unroll
            for (int i = 0; i < kRsBlock; i += 2) {
                const double2 v = *reinterpret_cast<const double2*>(&se[e][ty * kRsBlock + i]);
                a[i] = v.x; a[i + 1] = v.y;
                const double2 w = *reinterpret_cast<const double2*>(&sp[e][ty * kRsBlock + i]);
                q[i] = w.x; q[i + 1] = w.y;
                const double2 u = *reinterpret_cast<const double2*>(&sc[e][tx * kRsBlock + i]);
                b[i] = u.x; b[i + 1] = u.y;
            }
#pragma unroll
            for (int i = 0; i < kRsBlock; ++i)
#pragma unroll
                for (int j = 0; j < kRsBlock; ++j) {
                    const double r = __dsub_rn(a[i], b[j]);
                    an[i][j] = form_mul_add<FUSED>(r, r, an[i][j]);
                    ad[i][j] = form_mul_add<FUSED>(q[i], r, ad[i][j]);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < kRsBlock; ++i) {
        const uint64_t doc = doc0 + ty * kRsBlock + i;
        if (doc >= n) continue;
#pragma unroll
        for (int j = 0; j < kRsBlock; ++j) {
            const uint32_t cl = cl0 + tx * kRsBlock + j;
            if (cl >= c) continue;
            out_norm[doc * c + cl] = an[i][j];
            if (out_dot) out_dot[doc * c + cl] = ad[i][j];
        }
    }
}

// One lane per pair p of a flat list: document doc_of[p] (nullptr: p itself), cluster cand[p].  CAND: out_norm[p], out_dot[p]
// (nullable).  !CAND (cand unused, one pair per document): out_norm[p] = primaryNormSquared (:189-195), 0.0 without a primary.
template <bool FUSED, bool CAND>
__global__ __launch_bounds__(kArThreads) void artifact_residual_pairs_kernel(const float* __restrict__ x, uint32_t dim,
                                                                             const float* __restrict__ cents,
                                                                             const uint32_t* __restrict__ primary,
                                                                             const uint32_t* __restrict__ doc_of,
                                                                             const uint32_t* __restrict__ cand, uint64_t total,
                                                                             double* __restrict__ out_norm, double* __restrict__ out_dot) {
    __shared__ RowWalkTile te, tp, tc;
    __shared__ uint32_t s_doc[kArThreads], s_pri[kArThreads], s_cl[kArThreads];
    const int t = threadIdx.x;
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kArThreads + t;
    const bool live = p < total;
    const uint32_t doc = live ? (doc_of ? doc_of[p] : static_cast<uint32_t>(p)) : kArNone;
    const uint32_t pr = (live && primary) ? primary[doc] : kArNone;
    const bool has = pr != kArNone;
    s_doc[t] = doc; s_pri[t] = pr;
    if (CAND) s_cl[t] = live ? cand[p] : kArNone;
    double nrm = 0.0, dot = 0.0;
    for (uint32_t d0 = 0; d0 < dim; d0 += kRwChunk) {
        __syncthreads();
        ar_stage_gather(x, dim, s_doc, d0, te);
        if (primary) ar_stage_gather(cents, dim, s_pri, d0, tp);
        if (CAND) ar_stage_gather(cents, dim, s_cl, d0, tc);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kRwChunk; ++e) {
            const double ev = static_cast<double>(te[t][e]);
            const double q = has ? __dsub_rn(ev, static_cast<double>(tp[t][e])) : 0.0;
            if (CAND) {
                const double r = __dsub_rn(ev, static_cast<double>(tc[t][e]));
                nrm = form_mul_add<FUSED>(r, r, nrm);
                dot = form_mul_add<FUSED>(q, r, dot);
            } else {
                nrm = form_mul_add<FUSED>(q, q, nrm);
            }
        }
    }
    if (!live) return;
    out_norm[p] = nrm;
    if (CAND && out_dot) out_dot[p] = dot;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static inline uint32_t ar_blocks(uint64_t n, uint32_t per) { return static_cast<uint32_t>((n + per - 1) / per); }

hipError_t launch_artifact_check(hipStream_t st, const uint64_t* off, uint64_t lists, uint64_t total, const uint32_t* idx, uint32_t limit,
                                 uint32_t* flags) {
    if (lists) artifact_check_offsets_kernel<<<ar_blocks(lists, kArThreads), kArThreads, 0, st>>>(off, lists, total, flags);
    if (total) artifact_check_index_kernel<<<ar_blocks(total, kArThreads), kArThreads, 0, st>>>(idx, total, limit, 0, flags);
    return hipGetLastError();
}

hipError_t launch_artifact_check_primary(hipStream_t st, const uint32_t* primary, uint64_t n, uint32_t c, uint32_t* flags) {
    if (n) artifact_check_index_kernel<<<ar_blocks(n, kArThreads), kArThreads, 0, st>>>(primary, n, c, 1, flags);
    return hipGetLastError();
}

hipError_t launch_artifact_owner(hipStream_t st, const uint64_t* off, uint32_t lists, uint64_t total, uint32_t* owner) {
    if (total) artifact_owner_kernel<<<ar_blocks(total, kArThreads), kArThreads, 0, st>>>(off, lists, total, owner);
    return hipGetLastError();
}

hipError_t launch_artifact_centroids(hipStream_t st, const float* x, uint32_t dim, const uint64_t* off, const uint32_t* members, uint32_t c,
                                     float* out, uint32_t* out_counts) {
    artifact_centroid_kernel<<<dim3(c, ar_blocks(dim, kArThreads)), kArThreads, 0, st>>>(x, dim, off, members, out, out_counts);
    return hipGetLastError();
}

hipError_t launch_artifact_rep_init(hipStream_t st, const uint64_t* off, uint32_t c, const uint8_t* centroid_empty, uint32_t n_extra,
                                    uint32_t* limit, uint32_t* last) {
    artifact_rep_init_kernel<<<ar_blocks(c, kArThreads), kArThreads, 0, st>>>(off, c, centroid_empty, n_extra, limit, last);
    return hipGetLastError();
}

hipError_t launch_artifact_rep_pass(hipStream_t st, const float* x, uint32_t dim, const double2* row_norm, const uint64_t* off,
                                    const uint32_t* cand, const uint32_t* owner, uint64_t total, uint32_t c, const float* cents,
                                    const double2* cent_norm, const uint32_t* limit, uint32_t* last, uint32_t s, uint32_t n_extra,
                                    uint8_t* used, double* min_dist, uint32_t* out_selected) {
    if (total == 0) return hipSuccess;
    artifact_rep_dist_kernel<<<ar_blocks(total, kArThreads), kArThreads, 0, st>>>(x, dim, row_norm, off, cand, owner, total, cents, cent_norm,
                                                                                  limit, last, s, used, min_dist);
    artifact_rep_pick_kernel<<<c, kArThreads, 0, st>>>(off, limit, s, n_extra, used, min_dist, last, out_selected);
    return hipGetLastError();
}

hipError_t launch_artifact_residual_dense(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const float* cents, uint32_t c,
                                          const uint32_t* primary, bool fused, double* out_norm, double* out_dot) {
    const dim3 grid(ar_blocks(n, kRsTile), ar_blocks(c, kRsTile));
    if (fused) artifact_residual_dense_kernel<true><<<grid, kArThreads, 0, st>>>(x, n, dim, cents, c, primary, out_norm, out_dot);
    else artifact_residual_dense_kernel<false><<<grid, kArThreads, 0, st>>>(x, n, dim, cents, c, primary, out_norm, out_dot);
    return hipGetLastError();
}

hipError_t launch_artifact_residual_list(hipStream_t st, const float* x, uint32_t dim, const float* cents, const uint32_t* primary,
                                         const uint32_t* doc_of, const uint32_t* cand, uint64_t total, bool fused, double* out_norm,
                                         double* out_dot) {
    if (total == 0) return hipSuccess;
    const uint32_t blocks = ar_blocks(total, kArThreads);
    if (fused) artifact_residual_pairs_kernel<true, true><<<blocks, kArThreads, 0, st>>>(x, dim, cents, primary, doc_of, cand, total, out_norm, out_dot);
    else artifact_residual_pairs_kernel<false, true><<<blocks, kArThreads, 0, st>>>(x, dim, cents, primary, doc_of, cand, total, out_norm, out_dot);
    return hipGetLastError();
}

hipError_t launch_artifact_primary_norm(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const float* cents, const uint32_t* primary,
                                        bool fused, double* out_norm) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = ar_blocks(n, kArThreads);
    if (fused) artifact_residual_pairs_kernel<true, false><<<blocks, kArThreads, 0, st>>>(x, dim, cents, primary, nullptr, nullptr, n, out_norm, nullptr);
    else artifact_residual_pairs_kernel<false, false><<<blocks, kArThreads, 0, st>>>(x, dim, cents, primary, nullptr, nullptr, n, out_norm, nullptr);
    return hipGetLastError();
}

} // namespace yams_accel
