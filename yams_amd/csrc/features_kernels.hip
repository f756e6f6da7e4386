// features_kernels.hip — gfx950 kernels of the topology build's input features (TopologyInputExtractor::extract).
//
// Reference semantics being reproduced (paths relative to the reference checkout; the contract is restated line by line in
// include/yams_mi355x_accel.h):
//   src/topology/topology_input_extractor.cpp:397-430   aggregateEmbedding: the first contributing record ASSIGNS, the later
//                                                       ones are added in fp32, / float(count) when count > 1
//   src/topology/topology_input_extractor.cpp:123-152   computeVarianceWeights' two passes: per dimension two fp64 chains in
//                                                       sample order
//   src/topology/topology_input_extractor.cpp:98-110    l2NormalizeInPlace: one fp64 chain of squares, float(sqrt), fp32 divides
//   src/topology/topology_input_extractor.cpp:172-186   applyMatryoshkaCoarse: dense[kept[j]] * weights[kept[j]] in fp32
//   src/topology/topology_input_extractor.cpp:192-203   bucketCountSketch
//   src/topology/topology_input_extractor.cpp:362-387   the weighted concatenation
//
// Launches:
//   features_aggregate_kernel          one lane per (document, dimension) walks the record list in order
//   features_variance_kernel           one lane per dimension, 64 dimensions per workgroup (coalesced across lanes); a chain is
//                                      never split, so the call is a LATENCY chain of 2 m dependent fp64 steps; the loads of
//                                      the next kFeatVarRows sample rows are issued before this batch's chain runs
//   features_row_nsq_kernel            the chain of squares of every ungathered row: the staging and the chain of
//                                      row_chains.h, no query
//   features_row_nsq_gather_kernel     the same over dense[kept[j]] * w[j]: 256 rows x 32 kept columns through LDS, one lane
//                                      per row chains them in order
//   features_compose_store_kernel      one lane per output element: gather, multiply, divide by the norm, scale, or the entity
//                                      part, or the zero fill; out_dims
//   features_compose_sketch_kernel     one workgroup per row with a sketch: bucket counts by LDS integer atomics
//
// The sketch's chain of squares needs no order: the counts are integers with sum sig_len <= 65536, so every partial sum of
// their squares is an integer <= 2^32, exact in fp64 whatever the order; it is summed in uint64 and converted once.
// Float steps are spelled __fadd_rn / __fmul_rn / __fdiv_rn / __dsqrt_rn (no contraction, the correctly rounded divide and
// square root); the device code keeps f32 denormals.  The squares of floats are exact in fp64: fma(v, v, acc) == acc + v * v.
#include "common.h"
#include "features_launch.h"
#include "form_step.h"
#include "row_chains.h"

namespace yams_accel {

namespace {

constexpr int kFeatThreads = 256;
constexpr int kFeatGatherChunk = 32;                    // kept columns per LDS stage
constexpr int kFeatGatherLds = kFeatGatherChunk + 1;    // padded row stride: thread t reads row t, conflict-free
constexpr uint32_t kFeatMaxBuckets = kFeatMaxDim;
static_assert(kFeatThreads == kRowThreads, "one row per thread, as row_chains has it");

inline uint32_t feat_blocks(uint64_t items, uint32_t per) { return static_cast<uint32_t>((items + per - 1) / per); }

// :363-370 — which parts a row has, and the three fusion weights
struct FeatRowParts { bool e_on, m_on; uint32_t e_len, m_len; float a_d, a_e, a_m; };
__device__ __forceinline__ FeatRowParts feat_row_parts(const FeatComposeArgs& a, uint64_t i) {
    FeatRowParts p;
    p.e_on = a.entity && a.k && a.entity_on[i];
    p.m_on = a.sig && a.sig_len && a.sketch_dim && a.sketch_on[i];
    p.e_len = p.e_on ? a.k : 0u;
    p.m_len = p.m_on ? a.sketch_dim : 0u;
    p.a_e = p.e_on ? a.alpha_e : 0.0f;
    p.a_m = p.m_on ? a.alpha_m : 0.0f;
    const float t = __fsub_rn(__fsub_rn(1.0f, p.a_e), p.a_m);
    p.a_d = (0.0f < t) ? t : 0.0f;      // std::max(0.0F, t) = (0.0F < t) ? t : 0.0F: a NaN gives 0.0F
    return p;
}

} // namespace

// Grid: x = the document, y = 256 dimensions.
__global__ __launch_bounds__(kFeatThreads) void features_aggregate_kernel(const float* __restrict__ rows, uint32_t dim,
                                                                          const uint64_t* __restrict__ off,
                                                                          const uint32_t* __restrict__ records, float* __restrict__ out,
                                                                          uint32_t* __restrict__ out_counts) {
    const uint32_t doc = blockIdx.x;
    const uint32_t d = blockIdx.y * kFeatThreads + threadIdx.x;
    const uint64_t lo = off[doc];
    const uint32_t cnt = static_cast<uint32_t>(off[doc + 1] - lo);
    if (blockIdx.y == 0 && threadIdx.x == 0) out_counts[doc] = cnt;
    if (d >= dim) return;
    const uint32_t* list = records + lo;
    float s = 0.0f;
    if (cnt) {
        s = rows[static_cast<uint64_t>(list[0]) * dim + d];      // :411 — assigned: the bits are kept
#pragma unroll 4
        for (uint32_t m = 1; m < cnt; ++m) s = __fadd_rn(s, rows[static_cast<uint64_t>(list[m]) * dim + d]);
        if (cnt > 1) s = __fdiv_rn(s, static_cast<float>(cnt));
    }
    out[static_cast<uint64_t>(doc) * dim + d] = s;
}

// Grid: x = 64 dimensions.  Lane = dimension; the sample rows are walked in order, kFeatVarRows at a time.
template <bool FUSED>
__global__ __launch_bounds__(kFeatVarLanes) void features_variance_kernel(const float* __restrict__ rows, uint32_t dim,
                                                                          const uint32_t* __restrict__ select, uint32_t m,
                                                                          double* __restrict__ out_mean, double* __restrict__ out_var) {
    const uint32_t d = blockIdx.x * kFeatVarLanes + threadIdx.x;
    const bool on = d < dim;
    const float* col = rows + (on ? d : 0u);
    auto fetch = [&](float (&v)[kFeatVarRows], uint32_t i0) {
#pragma unroll
        for (int j = 0; j < kFeatVarRows; ++j) {
            const uint32_t i = i0 + j;
            v[j] = 0.0f;
            if (on && i < m) v[j] = col[static_cast<uint64_t>(select ? select[i] : i) * dim];
        }
    };
    float cur[kFeatVarRows], nxt[kFeatVarRows] = {};
    // :123-139 — mean[i] += e[i] in sample order, /= double(n)
    double mean = 0.0;
    fetch(cur, 0);
    for (uint32_t i0 = 0; i0 < m; i0 += kFeatVarRows) {
        if (i0 + kFeatVarRows < m) fetch(nxt, i0 + kFeatVarRows);
#pragma unroll
        for (int j = 0; j < kFeatVarRows; ++j)
            if (i0 + j < m) mean = __dadd_rn(mean, static_cast<double>(cur[j]));
#pragma unroll
        for (int j = 0; j < kFeatVarRows; ++j) cur[j] = nxt[j];
    }
    mean = __ddiv_rn(mean, static_cast<double>(m));
    // :140-152 — d = double(e[i]) - mean[i]; var[i] += d * d; /= double(n)
    double var = 0.0;
    fetch(cur, 0);
    for (uint32_t i0 = 0; i0 < m; i0 += kFeatVarRows) {
        if (i0 + kFeatVarRows < m) fetch(nxt, i0 + kFeatVarRows);
#pragma unroll
        for (int j = 0; j < kFeatVarRows; ++j)
            if (i0 + j < m) {
                const double r = __dsub_rn(static_cast<double>(cur[j]), mean);
                var = form_mul_add<FUSED>(r, r, var);
            }
#pragma unroll
        for (int j = 0; j < kFeatVarRows; ++j) cur[j] = nxt[j];
    }
    var = __ddiv_rn(var, static_cast<double>(m));
    if (on) {
        out_mean[d] = mean;
        out_var[d] = var;
    }
}

__global__ __launch_bounds__(kRowThreads) void features_row_nsq_kernel(const float* __restrict__ rows, uint64_t n, uint32_t dim, int vec4,
                                                                       double* __restrict__ nsq_out) {
    __shared__ RowLdsRows s_rows;
    __shared__ RowLdsQueries<1> s_q;
    __shared__ RowLdsOrdinals s_row;
    const uint64_t row = static_cast<uint64_t>(blockIdx.x) * kRowThreads + threadIdx.x;
    const bool on = row < n;
    double nsq, dot[1];
    // n_slots = 0: no query is read, the query tile is zeros
    row_chains<1>(s_rows, s_q, s_row, on ? static_cast<uint32_t>(row) : kRowNone, rows, dim, vec4, rows, 0, 0, 0, on, nsq, dot);
    if (on) nsq_out[row] = nsq;
}

// Grid: x = 256 rows.  Per stage of 32 kept columns, 32 lanes read one row's kept elements (ascending columns), 8 rows per
// pass; thread t then chains row t's 32 products in order.
__global__ __launch_bounds__(kFeatThreads) void features_row_nsq_gather_kernel(const float* __restrict__ dense, uint64_t n, uint32_t dim,
                                                                               const uint32_t* __restrict__ kept,
                                                                               const float* __restrict__ kept_w, uint32_t kc,
                                                                               double* __restrict__ nsq_out) {
    __shared__ float s_x[kFeatThreads * kFeatGatherLds];
    __shared__ uint32_t s_k[kFeatGatherChunk];
    __shared__ float s_w[kFeatGatherChunk];
    const int t = threadIdx.x, e = t & (kFeatGatherChunk - 1);
    const uint64_t row0 = static_cast<uint64_t>(blockIdx.x) * kFeatThreads;
    const bool on = row0 + t < n;
    double acc = 0.0;
    for (uint32_t c0 = 0; c0 < kc; c0 += kFeatGatherChunk) {
        const uint32_t cl = kc - c0 < static_cast<uint32_t>(kFeatGatherChunk) ? kc - c0 : static_cast<uint32_t>(kFeatGatherChunk);
        if (t < kFeatGatherChunk) {
            const bool in = static_cast<uint32_t>(t) < cl;
            s_k[t] = in ? kept[c0 + t] : 0u;
            s_w[t] = in ? kept_w[c0 + t] : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int it = 0; it < kFeatThreads / 8; ++it) {
            const int r = (t >> 5) + 8 * it;
            const uint64_t row = row0 + r;
            s_x[r * kFeatGatherLds + e] =
                (row < n && static_cast<uint32_t>(e) < cl) ? __fmul_rn(dense[row * dim + s_k[e]], s_w[e]) : 0.0f;      // :183
        }
        __syncthreads();
        if (on) {
            const float* x = s_x + t * kFeatGatherLds;
#pragma unroll 4
            for (uint32_t i = 0; i < cl; ++i) {
                const double v = static_cast<double>(x[i]);
                acc = fma(v, v, acc);
            }
        }
        __syncthreads();
    }
    if (on) nsq_out[row0 + t] = acc;
}

// Grid: x = the row, y = 256 output elements (at least one workgroup per row: out_dims).
__global__ __launch_bounds__(kFeatThreads) void features_compose_store_kernel(FeatComposeArgs a) {
    const uint64_t i = blockIdx.x;
    const uint32_t j = blockIdx.y * kFeatThreads + threadIdx.x;
    const FeatRowParts p = feat_row_parts(a, i);
    const uint32_t dlen = a.kc;
    if (j == 0) a.out_dims[i] = dlen + p.e_len + p.m_len;
    if (j >= a.out_stride) return;
    float v = 0.0f;      // behind the row's length: zeros
    if (j < dlen) {
        float x = a.kept ? __fmul_rn(a.dense[i * a.dim + a.kept[j]], a.kept_w[j]) : a.dense[i * a.dim + j];
        const double q = a.nsq[i];
        if (!(q <= 0.0)) x = __fdiv_rn(x, static_cast<float>(__dsqrt_rn(q)));      // :103-109 — a NaN sumSq does divide
        v = (p.e_on || p.m_on) ? __fmul_rn(x, p.a_d) : x;                          // :365-366 — both off: no multiply
    } else if (j < dlen + p.e_len) {
        v = __fmul_rn(a.entity[i * a.k + (j - dlen)], p.a_e);
    } else if (j < dlen + p.e_len + p.m_len) {
        return;      // features_compose_sketch_kernel's
    }
    a.out[i * a.out_stride + j] = v;
}

// Grid: x = the row.  Rows without a sketch leave at once.
__global__ __launch_bounds__(kFeatThreads) void features_compose_sketch_kernel(FeatComposeArgs a) {
    __shared__ uint32_t s_cnt[kFeatMaxBuckets];
    __shared__ unsigned long long s_sum;
    const uint64_t i = blockIdx.x;
    const FeatRowParts p = feat_row_parts(a, i);
    if (!p.m_on) return;
    const int t = threadIdx.x;
    const uint32_t sd = a.sketch_dim;
    for (uint32_t b = t; b < sd; b += kFeatThreads) s_cnt[b] = 0u;
    if (t == 0) s_sum = 0ull;
    __syncthreads();
    const uint32_t* sig = a.sig + i * a.sig_len;
    for (uint32_t e = t; e < a.sig_len; e += kFeatThreads) atomicAdd(&s_cnt[sig[e] % sd], 1u);      // :197-200
    __syncthreads();
    unsigned long long local = 0ull;
    for (uint32_t b = t; b < sd; b += kFeatThreads) {
        const unsigned long long c = s_cnt[b];
        local += c * c;
    }
    if (local) atomicAdd(&s_sum, local);
    __syncthreads();
    // the counts sum to sig_len >= 1: sumSq >= 1, the `<= 0.0` branch is never taken
    const float norm = static_cast<float>(__dsqrt_rn(static_cast<double>(s_sum)));
    float* dst = a.out + i * a.out_stride + a.kc + p.e_len;
    for (uint32_t b = t; b < sd; b += kFeatThreads) dst[b] = __fmul_rn(__fdiv_rn(static_cast<float>(s_cnt[b]), norm), p.a_m);
}

hipError_t launch_features_aggregate(hipStream_t st, const float* rows, uint32_t dim, const uint64_t* doc_offsets, const uint32_t* records,
                                     uint32_t n_docs, float* out, uint32_t* out_counts) {
    if (n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(features_aggregate_kernel, dim3(n_docs, feat_blocks(dim, kFeatThreads)), dim3(kFeatThreads), 0, st, rows, dim,
                       doc_offsets, records, out, out_counts);
    return hipGetLastError();
}

hipError_t launch_features_variance(hipStream_t st, const float* rows, uint32_t dim, const uint32_t* select, uint32_t m, bool fused,
                                    double* out_mean, double* out_var) {
    if (m == 0) return hipSuccess;
    const dim3 grid(feat_blocks(dim, kFeatVarLanes));
    if (fused)
        hipLaunchKernelGGL((features_variance_kernel<true>), grid, dim3(kFeatVarLanes), 0, st, rows, dim, select, m, out_mean, out_var);
    else
        hipLaunchKernelGGL((features_variance_kernel<false>), grid, dim3(kFeatVarLanes), 0, st, rows, dim, select, m, out_mean, out_var);
    return hipGetLastError();
}

hipError_t launch_features_row_nsq(hipStream_t st, const float* dense, uint64_t n, uint32_t dim, const uint32_t* kept, const float* kept_w,
                                   uint32_t kc, double* nsq) {
    if (n == 0 || kc == 0) return hipSuccess;
    const dim3 grid(feat_blocks(n, kFeatThreads));
    if (kept)
        hipLaunchKernelGGL(features_row_nsq_gather_kernel, grid, dim3(kFeatThreads), 0, st, dense, n, dim, kept, kept_w, kc, nsq);
    else
        hipLaunchKernelGGL(features_row_nsq_kernel, grid, dim3(kRowThreads), 0, st, dense, n, dim, row_vec4_loads(dense, dim), nsq);
    return hipGetLastError();
}

hipError_t launch_features_compose_store(hipStream_t st, const FeatComposeArgs& a) {
    if (a.n == 0) return hipSuccess;
    const uint32_t gy = a.out_stride ? feat_blocks(a.out_stride, kFeatThreads) : 1u;
    hipLaunchKernelGGL(features_compose_store_kernel, dim3(static_cast<uint32_t>(a.n), gy), dim3(kFeatThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_features_compose_sketch(hipStream_t st, const FeatComposeArgs& a) {
    if (a.n == 0 || !a.sig || !a.sig_len || !a.sketch_dim) return hipSuccess;
    hipLaunchKernelGGL(features_compose_sketch_kernel, dim3(static_cast<uint32_t>(a.n)), dim3(kFeatThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace yams_accel
