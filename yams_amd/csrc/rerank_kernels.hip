// rerank_kernels.hip — gfx950 kernels of the late-interaction rerank (ColBERT MaxSim) and of the token pooling.
//
// Reference semantics being reproduced (paths relative to the reference checkout; the contract is restated in
// include/yams_mi355x_accel.h):
//   plugins/onnx/onnx_colbert_session.cpp:286-293   dot: sum = 0.0f; sum += a[i] * b[i] in element order — a separate multiply
//                                                   and add, or one fmaf, as the host's compiler made it
//   plugins/onnx/onnx_colbert_session.cpp:247-259   computeMaxSim: per query token maxSim = -inf, replaced only when
//                                                   sim > maxSim; score += maxSim in query order
//   plugins/onnx/onnx_colbert_session.cpp:214-230   maxPoolEmbeddings: std::max per dimension, non-finite -> 0.0f
//   plugins/onnx/onnx_colbert_session.cpp:232-245   normalizeEmbedding: one fp64 chain of squares, sqrt, v / norm in fp64
//
// Launches:
//   rerank_rowmax_kernel<FUSED, MFMA>   grid (document, tile of 32 query tokens), 256 threads.  The document is walked in
//                                       passes of 256 tokens; per pass the dimensions are staged through LDS 32 at a time,
//                                       TRANSPOSED ([k][token]) so that neither path meets a bank conflict.  Every (query
//                                       token, document token) pair is ONE chain walked in i order in ONE accumulator:
//       VALU  a lane holds a 4 x 8 register tile of chains; per i one b128 read of the query tile and two of the document
//             tile feed 32 steps: v_mul_f32 + v_add_f32 (separate) or v_fma_f32 (fused)
//       MFMA  (fused only) v_mfma_f32_32x32x2_f32 with C = +0.0f and k ascending: A = 32 document tokens, B = the 32 query
//             tokens, two independent accumulators per wave (64 document tokens), four waves per pass.  The result column is
//             the lane's query token, the 16 registers are document tokens: the row maximum is a per-lane scan.
//       Epilogue: every lane folds its finished chains into (maximum, token index) with the reference's `sim > maxSim` in
//       ascending token order; the partial winners of a query token (32 lanes on the VALU path, 8 on the MFMA path) meet in
//       LDS, where the larger value wins and equal values — zeros of both signs included — go to the EARLIER token: the first
//       in document order stays, as in the reference.  No float atomics.
//   rerank_score_kernel                 the per-document score chain, one lane per document, in query order, over the finished
//                                       row maxima: a second small launch rather than a per-document completion count, which
//                                       would need a zeroed counter array, a device-scope fence per workgroup and a last-block
//                                       tail that runs the chain while the other tiles' CUs wait anyway.
//   rerank_maxpool_kernel               one workgroup per document: one max chain per dimension (a lane each), then ONE fp64
//                                       chain of squares in one lane, then the divides.
//   rerank_check_kernel                 the offsets: from 0, never decreasing, ending at the total; no document too long.
//
// A dimension count that is no multiple of the k step is padded with query = -0.0f and document = +0.0f: the product is
// -0.0f, and sum + (-0.0f) == sum for every sum, -0.0f included (a fused chain can hold one: a negative product that
// underflows).  Float steps are spelled __fmul_rn / __fadd_rn / __fmaf_rn; the library is built with -ffp-contract=off and keeps
// f32 denormals.
#include "common.h"
#include "form_step.h"
#include "l2_normalize.h"
#include "rerank_launch.h"

namespace yams_accel {

namespace {

constexpr int kQStride = kRerankQTile;               // s_q[k][query token]; 32: the two k of an MFMA step sit 32 banks apart
constexpr int kDStride = kRerankDTile + 32;          // s_d[k][document token]; 288 = 32 mod 64: likewise
constexpr int kLdsFloats = kRerankKChunk * kQStride + kRerankKChunk * kDStride;
constexpr int kCandMax = 32;                         // partial winners per query token
static_assert(kRerankThreads == kRerankDTile, "one document token per thread when a pass is staged");
static_assert(2 * kCandMax * kRerankQTile <= kRerankKChunk * kDStride, "the partial winners reuse the document tile");

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the reference's `if (sim > maxSim) maxSim = sim;` — a NaN never wins
__device__ __forceinline__ void rerank_take(float& bv, uint32_t& bi, float v, uint32_t i) {
    if (v > bv) { bv = v; bi = i; }
}
// two partial winners over disjoint token sets: the larger value; equal values (zeros of both signs are equal): the earlier
// token.  kRerankNone (nothing won, the value is the initial -inf) is later than every token.
__device__ __forceinline__ void rerank_merge(float& bv, uint32_t& bi, float v, uint32_t i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

} // namespace

template <bool FUSED, bool MFMA>
__global__ __launch_bounds__(kRerankThreads) void rerank_rowmax_kernel(const float* __restrict__ query, uint32_t tq, uint32_t dim,
                                                                       const float* __restrict__ rows, const uint64_t* __restrict__ off,
                                                                       float* __restrict__ rowmax, uint32_t* __restrict__ rowarg) {
    static_assert(FUSED || !MFMA, "the matrix cores fuse");
    __shared__ __attribute__((aligned(16))) float s_mem[kLdsFloats];
    float* s_q = s_mem;
    float* s_d = s_mem + kRerankKChunk * kQStride;
    const int t = threadIdx.x;
    const uint32_t doc = blockIdx.x;
    const uint32_t q0 = blockIdx.y * kRerankQTile;
    const uint64_t lo = off[doc];
    const uint32_t len = static_cast<uint32_t>(off[doc + 1] - lo);
    const float* drows = rows + lo * dim;
    const bool vec4 = (dim & 3u) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15u) == 0;

    // VALU: query tokens 4 tq .. +3, document tokens 8 td .. +7 of the pass.  MFMA: lane's query token and k half.
    const int tq4 = (t & 7) * 4, td8 = (t >> 3) * 8;
    const int lane = t & 63, wave = t >> 6, col = lane & 31, half = lane >> 5;
    constexpr int kOwn = MFMA ? 1 : 4;
    float best_v[kOwn];
    uint32_t best_i[kOwn];
#pragma unroll
    for (int a = 0; a < kOwn; ++a) { best_v[a] = -INFINITY; best_i[a] = kRerankNone; }

    for (uint32_t d0 = 0; d0 < len; d0 += kRerankDTile) {
        float acc[4][8];
        f32x16 c0, c1;
        if constexpr (MFMA) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { c0[r] = 0.0f; c1[r] = 0.0f; }
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] = 0.0f;
        }
        for (uint32_t k0 = 0; k0 < dim; k0 += kRerankKChunk) {
            const uint32_t cl = dim - k0 < static_cast<uint32_t>(kRerankKChunk) ? dim - k0 : static_cast<uint32_t>(kRerankKChunk);
            // ---- stage: the query tile (thread = query token, 4 of the 32 k each) and the pass (thread = document token) ----
            {
                const uint32_t q = q0 + (t & 31);
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const uint32_t k = (t >> 5) + 8 * it;
                    s_q[k * kQStride + (t & 31)] = (q < tq && k < cl) ? query[static_cast<uint64_t>(q) * dim + k0 + k] : -0.0f;
                }
                const uint32_t d = d0 + t;
                const float* src = drows + static_cast<uint64_t>(d) * dim + k0;
                float v[kRerankKChunk];
                if (d < len && vec4) {      // dim % 4 == 0: cl % 4 == 0 too
#pragma unroll
                    for (int j = 0; j < kRerankKChunk / 4; ++j) {
                        float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (static_cast<uint32_t>(4 * j) < cl) x = *reinterpret_cast<const float4*>(src + 4 * j);
                        v[4 * j] = x.x; v[4 * j + 1] = x.y; v[4 * j + 2] = x.z; v[4 * j + 3] = x.w;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < kRerankKChunk; ++k) v[k] = (d < len && static_cast<uint32_t>(k) < cl) ? src[k] : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < kRerankKChunk; ++k) s_d[k * kDStride + t] = v[k];
            }
            __syncthreads();
            // ---- the chains, i ascending ----
            if constexpr (MFMA) {
                const float* pb = s_q + half * kQStride + col;
                const float* pa = s_d + half * kDStride + wave * 64 + col;
                const uint32_t steps = (cl + 1) >> 1;
                for (uint32_t s = 0; s < steps; ++s) {
                    const float b = pb[2 * s * kQStride];
                    const float a0 = pa[2 * s * kDStride], a1 = pa[2 * s * kDStride + 32];
                    c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, c0, 0, 0, 0);
                    c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, c1, 0, 0, 0);
                }
            } else {
                for (uint32_t i = 0; i < cl; ++i) {
                    const float4 qv = *reinterpret_cast<const float4*>(s_q + i * kQStride + tq4);
                    const float4 da = *reinterpret_cast<const float4*>(s_d + i * kDStride + td8);
                    const float4 db = *reinterpret_cast<const float4*>(s_d + i * kDStride + td8 + 4);
                    const float qa[4] = {qv.x, qv.y, qv.z, qv.w};
                    const float dv[8] = {da.x, da.y, da.z, da.w, db.x, db.y, db.z, db.w};
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 8; ++b) acc[a][b] = form_mul_add<FUSED>(qa[a], dv[b], acc[a][b]);
                }
            }
            __syncthreads();
        }
        // ---- fold the finished chains of this pass, ascending token order ----
        if constexpr (MFMA) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {      // C/D: row = (r & 3) + 8 (r >> 2) + 4 half
                const uint32_t d = d0 + wave * 64 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (d < len) rerank_take(best_v[0], best_i[0], c0[r], d);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t d = d0 + wave * 64 + 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (d < len) rerank_take(best_v[0], best_i[0], c1[r], d);
            }
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const uint32_t d = d0 + td8 + b;
                    if (d < len) rerank_take(best_v[a], best_i[a], acc[a][b], d);
                }
        }
    }
    // ---- the partial winners of each query token meet in LDS (the document tile is free: the loop ended on a barrier) ----
    float* s_bv = s_d;
    uint32_t* s_bi = reinterpret_cast<uint32_t*>(s_d) + kCandMax * kRerankQTile;
    constexpr int kCand = MFMA ? 8 : 32;
    if constexpr (MFMA) {
        const int cand = wave * 2 + half;
        s_bv[cand * kRerankQTile + col] = best_v[0];
        s_bi[cand * kRerankQTile + col] = best_i[0];
    } else {
        const int cand = t >> 3;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            s_bv[cand * kRerankQTile + tq4 + a] = best_v[a];
            s_bi[cand * kRerankQTile + tq4 + a] = best_i[a];
        }
    }
    __syncthreads();
    if (t < kRerankQTile && q0 + t < tq) {
        float bv = -INFINITY;
        uint32_t bi = kRerankNone;
        for (int c = 0; c < kCand; ++c) rerank_merge(bv, bi, s_bv[c * kRerankQTile + t], s_bi[c * kRerankQTile + t]);
        const uint64_t at = static_cast<uint64_t>(doc) * tq + q0 + t;
        rowmax[at] = bv;
        if (rowarg) rowarg[at] = bi;
    }
}

// One lane per document: score = 0.0f; score += maxSim in query order.
__global__ __launch_bounds__(64) void rerank_score_kernel(const float* __restrict__ rowmax, uint32_t tq, uint32_t n_docs,
                                                          float* __restrict__ scores) {
    const uint32_t doc = blockIdx.x * 64 + threadIdx.x;
    if (doc >= n_docs) return;
    const float* m = rowmax + static_cast<uint64_t>(doc) * tq;
    float score = 0.0f;
#pragma unroll 4
    for (uint32_t q = 0; q < tq; ++q) score = __fadd_rn(score, m[q]);
    scores[doc] = score;
}

// Grid: x = the document.
__global__ __launch_bounds__(kRerankThreads) void rerank_maxpool_kernel(const float* __restrict__ rows, uint32_t dim,
                                                                        const uint64_t* __restrict__ off, float* __restrict__ out) {
    __shared__ float s_p[kRerankMaxDim];
    __shared__ double s_norm;
    const int t = threadIdx.x;
    const uint32_t doc = blockIdx.x;
    const uint64_t lo = off[doc];
    const uint32_t len = static_cast<uint32_t>(off[doc + 1] - lo);
    const float* drows = rows + lo * dim;
    for (uint32_t d = t; d < dim; d += kRerankThreads) {
        float p = -INFINITY;
#pragma unroll 4
        for (uint32_t i = 0; i < len; ++i) {
            const float v = drows[static_cast<uint64_t>(i) * dim + d];
            if (p < v) p = v;                                   // :222 — std::max(pooled, token): a NaN never enters
        }
        if (p == INFINITY || p == -INFINITY) p = 0.0f;          // :226-227 — p is no NaN; an empty document: zeros (:216-219)
        s_p[d] = p;
    }
    __syncthreads();
    if (t == 0) s_norm = l2_norm(l2_chain(0.0, s_p, dim));      // l2_normalize.h: one lane, element order
    __syncthreads();
    const double norm = s_norm;
    for (uint32_t d = t; d < dim; d += kRerankThreads) out[static_cast<uint64_t>(doc) * dim + d] = l2_quotient(s_p[d], norm);
}

__global__ __launch_bounds__(256) void rerank_check_kernel(const uint64_t* __restrict__ off, uint64_t n_docs, uint64_t total,
                                                           uint32_t max_len, uint32_t* __restrict__ flags) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i > n_docs) return;
    uint32_t f = 0;
    if (i == 0 && off[0] != 0) f |= 1u;
    if (i == n_docs) {
        if (off[i] != total) f |= 1u;
    } else {
        if (off[i + 1] < off[i]) f |= 1u;
        else if (off[i + 1] - off[i] > max_len) f |= 2u;
    }
    if (f) atomicOr(flags, f);
}

hipError_t launch_rerank_check(hipStream_t st, const uint64_t* off, uint64_t n_docs, uint64_t total, uint32_t max_len, uint32_t* flags) {
    hipLaunchKernelGGL(rerank_check_kernel, dim3(static_cast<uint32_t>((n_docs + 256) / 256)), dim3(256), 0, st, off, n_docs, total, max_len,
                       flags);
    return hipGetLastError();
}

hipError_t launch_rerank_rowmax(hipStream_t st, const float* query, uint32_t tq, uint32_t dim, const float* rows, const uint64_t* off,
                                uint32_t n_docs, bool fused, RerankPath path, float* rowmax, uint32_t* rowarg) {
    if (n_docs == 0 || tq == 0) return hipSuccess;
    if (path == kRerankMfma && !fused) return hipErrorInvalidValue;
    const dim3 grid(n_docs, (tq + kRerankQTile - 1) / kRerankQTile), block(kRerankThreads);
    if (!fused)
        hipLaunchKernelGGL((rerank_rowmax_kernel<false, false>), grid, block, 0, st, query, tq, dim, rows, off, rowmax, rowarg);
    else if (path == kRerankMfma)
        hipLaunchKernelGGL((rerank_rowmax_kernel<true, true>), grid, block, 0, st, query, tq, dim, rows, off, rowmax, rowarg);
    else
        hipLaunchKernelGGL((rerank_rowmax_kernel<true, false>), grid, block, 0, st, query, tq, dim, rows, off, rowmax, rowarg);
    return hipGetLastError();
}

hipError_t launch_rerank_score(hipStream_t st, const float* rowmax, uint32_t tq, uint32_t n_docs, float* scores) {
    if (n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(rerank_score_kernel, dim3((n_docs + 63) / 64), dim3(64), 0, st, rowmax, tq, n_docs, scores);
    return hipGetLastError();
}

hipError_t launch_rerank_maxpool(hipStream_t st, const float* rows, uint32_t dim, const uint64_t* off, uint32_t n_docs, float* out) {
    if (n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(rerank_maxpool_kernel, dim3(n_docs), dim3(kRerankThreads), 0, st, rows, dim, off, out);
    return hipGetLastError();
}

} // namespace yams_accel
