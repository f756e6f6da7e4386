// embed_kernels.hip — gfx950 kernels of the embedding model's pooling head: CLS, max or mean over the tokens of each text, then
// the L2 normalisation.
//
// Reference semantics being reproduced (paths relative to the reference checkout; the contract is restated in
// include/yams_mi355x_accel.h):
//   plugins/onnx/onnx_model_pool.cpp:1808-1839   per text: emb starts at +0.0f; CLS copies token 0; MAX is std::max over the tokens
//                                                whose mask is > 0, in token order; MEAN is total += w; emb[d] += x * w over the
//                                                tokens with w = float(mask) > 0, in token order, then emb[d] / total if total > 0
//   plugins/onnx/onnx_model_pool.cpp:1840-1853   the fp64 chain of squares, sqrt, v / norm in fp64 or zeros (l2_normalize.h)
//   plugins/onnx/onnx_model_pool.cpp:1935-1953   the rank-2 output: the same normalisation of a copied row
//
// Launches:
//   embed_check_kernel        one lane per considered mask value: ORs the refusal (a MEAN weight above 1) and adds the wave's
//                             count of active tokens (one integer atomic per wave).
//   embed_pool_kernel<MODE, VEC>   grid (text, slab of dimensions), ONE wave.  A lane owns VEC consecutive dimensions and walks
//                             ALL tokens of its text for them: one fp32 chain per (text, dimension) in token order, in one
//                             register.  The text's mask is compacted, kEmbedWindow tokens at a time, into a list of active token
//                             indices in LDS (ballot + prefix count: the list is in token order); the chain then walks the list,
//                             so a masked row costs no load and is never read — a NaN there cannot reach the output.  kEmbedAhead
//                             row loads are issued before the first dependent add: their addresses come from the list, not from
//                             the chain.  VEC = 4: one 16-byte load per lane and row; VEC = 1: scalar loads.  MEAN serves masks of
//                             0 and 1 only (the check kernel refuses others), so x * w is x and total is the count of active
//                             tokens, exact in fp32 below 2^24.  The MEAN kernel leaves the SUMS and the text's count; the divide
//                             is the next launch's, so that this one holds additions only and nothing in it can be contracted.
//   embed_finish_kernel       one workgroup per row: v / total where a count is given and above 0 (MEAN), then, when asked, the
//                             normalisation.  The row passes through LDS kEmbedNormChunk floats at a time; ONE lane carries the
//                             fp64 chain of squares across the chunks in element order; every lane then divides its own elements
//                             (v / total is formed once: kept in LDS, or parked in the output for rows longer than a chunk).
// Float steps are spelled __fadd_rn / __fdiv_rn; the library is built with -ffp-contract=off and keeps f32 denormals.  No
// scratch, no float atomics.
#include "common.h"
#include "embed_launch.h"
#include "l2_normalize.h"

namespace yams_accel {

namespace {

template <int VEC> struct EmbedVec;
template <> struct EmbedVec<4> {
    float v[4];
    __device__ __forceinline__ void load(const float* p) {
        const float4 x = *reinterpret_cast<const float4*>(p);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    }
};
template <> struct EmbedVec<1> {
    float v[1];
    __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
};

template <uint32_t MODE> __device__ __forceinline__ float embed_step(float acc, float x) {
    if constexpr (MODE == kEmbedMax) return acc < x ? x : acc;      // :1821 — std::max(emb, x): a NaN never enters
    else return __fadd_rn(acc, x);                                  // :1833 — emb += x * w with w == 1.0f: the product is x
}

} // namespace

__global__ __launch_bounds__(256) void embed_check_kernel(const int32_t* __restrict__ mask, uint64_t batch, uint32_t mask_len, uint32_t t_len,
                                                          uint32_t mean, uint32_t* __restrict__ flags) {
    const uint64_t at = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    int32_t v = 0;
    if (at < batch * t_len) v = mask[(at / t_len) * mask_len + at % t_len];
    if (mean && v > 1) atomicOr(flags, 1u);
    const unsigned long long active = __ballot(v > 0);
    if ((threadIdx.x & 63) == 0 && active) atomicAdd(flags + 1, static_cast<uint32_t>(__popcll(active)));
}

// Grid: x = the text, y = the slab of dimensions.
template <uint32_t MODE, int VEC>
__global__ __launch_bounds__(kEmbedThreads) void embed_pool_kernel(const float* __restrict__ hidden, uint32_t seq, uint32_t dim,
                                                                   const int32_t* __restrict__ mask, uint32_t mask_len, uint32_t t_len,
                                                                   uint32_t slab_dims, float* __restrict__ out, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_idx[kEmbedWindow];
    const uint32_t lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const uint32_t d0 = blockIdx.y * slab_dims + lane * VEC;
    const bool own = lane * VEC < slab_dims && d0 < dim;      // dim % VEC == 0: an owned group is whole
    const float* rows = hidden + b * seq * dim + (own ? d0 : 0u);
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.0f;

    if constexpr (MODE == kEmbedCls) {
        if (own) {
            EmbedVec<VEC> x;
            x.load(rows);                                      // :1812-1814 — token 0, whatever the mask says
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] = x.v[j];
        }
    } else {
        const int32_t* m = mask + b * mask_len;
        uint32_t total = 0;
        for (uint32_t w0 = 0; w0 < t_len; w0 += kEmbedWindow) {
            // ---- the window's active tokens, in token order ----
            uint32_t n = 0;
#pragma unroll
            for (int p = 0; p < kEmbedWindow / kEmbedThreads; ++p) {
                const uint32_t i = w0 + p * kEmbedThreads + lane;
                const bool on = i < t_len && m[i] > 0;
                const unsigned long long bal = __ballot(on);
                if (on) s_idx[n + __popcll(bal & ((1ull << lane) - 1ull))] = i;
                n += static_cast<uint32_t>(__popcll(bal));
            }
            __syncthreads();
            total += n;
            // ---- the chains over the list: kEmbedAhead loads, then their steps in order ----
            if (own) {
                uint32_t k = 0;
                for (; k + kEmbedAhead <= n; k += kEmbedAhead) {
                    EmbedVec<VEC> x[kEmbedAhead];
#pragma unroll
                    for (int u = 0; u < kEmbedAhead; ++u) x[u].load(rows + static_cast<uint64_t>(s_idx[k + u]) * dim);
#pragma unroll
                    for (int u = 0; u < kEmbedAhead; ++u)
#pragma unroll
                        for (int j = 0; j < VEC; ++j) acc[j] = embed_step<MODE>(acc[j], x[u].v[j]);
                }
                for (; k < n; ++k) {
                    EmbedVec<VEC> x;
                    x.load(rows + static_cast<uint64_t>(s_idx[k]) * dim);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) acc[j] = embed_step<MODE>(acc[j], x.v[j]);
                }
            }
            __syncthreads();
        }
        if constexpr (MODE == kEmbedMean) {
            if (blockIdx.y == 0 && lane == 0) counts[b] = total;      // :1830 — total += 1.0f per active token: the count
        }
    }
    if (own) {
        float* o = out + b * dim + d0;
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else o[0] = acc[0];
    }
}

// Grid: x = the row.  counts: nullable.  rows == out is served: a lane reads its element before it writes it, and the staged reads
// of every chunk come before the first write.
__global__ __launch_bounds__(256) void embed_finish_kernel(const float* rows, uint32_t dim, const uint32_t* __restrict__ counts,
                                                           uint32_t normalize, float* out) {
    __shared__ float s_p[kEmbedNormChunk];
    __shared__ double s_norm;
    const uint32_t t = threadIdx.x;
    const float* src = rows + static_cast<uint64_t>(blockIdx.x) * dim;
    float* dst = out + static_cast<uint64_t>(blockIdx.x) * dim;
    const uint32_t total = counts ? counts[blockIdx.x] : 0u;
    const float tf = static_cast<float>(total);      // exact below 2^24
    // :1835-1838 — if (total > 0) v = v / total
    const auto mean = [&](float v) { return total > 0 ? __fdiv_rn(v, tf) : v; };
    if (!normalize) {
        for (uint32_t d = t; d < dim; d += 256) dst[d] = mean(src[d]);
        return;
    }
    // The quotient is formed ONCE per element: a row of one chunk keeps it in LDS; a longer row whose elements are divided parks
    // it in `dst` (element e is staged and finished by the same lane: e % 256 == t in both loops).
    const bool one_chunk = dim <= static_cast<uint32_t>(kEmbedNormChunk), parked = !one_chunk && total > 0;
    double nsq = 0.0;      // lane 0's
    for (uint32_t c0 = 0; c0 < dim; c0 += kEmbedNormChunk) {
        const uint32_t cl = dim - c0 < static_cast<uint32_t>(kEmbedNormChunk) ? dim - c0 : static_cast<uint32_t>(kEmbedNormChunk);
        for (uint32_t d = t; d < cl; d += 256) {
            const float v = mean(src[c0 + d]);
            s_p[d] = v;
            if (parked) dst[c0 + d] = v;
        }
        __syncthreads();
        if (t == 0) nsq = l2_chain(nsq, s_p, cl);
        __syncthreads();
    }
    if (t == 0) s_norm = l2_norm(nsq);
    __syncthreads();
    const double norm = s_norm;
    for (uint32_t d = t; d < dim; d += 256) dst[d] = l2_quotient(one_chunk ? s_p[d] : parked ? dst[d] : src[d], norm);
}

hipError_t launch_embed_check(hipStream_t st, const int32_t* mask, uint64_t batch, uint32_t mask_len, uint32_t t_len, bool mean,
                              uint32_t* flags) {
    const uint64_t n = batch * t_len;
    hipLaunchKernelGGL(embed_check_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, st, mask, batch, mask_len, t_len,
                       mean ? 1u : 0u, flags);
    return hipGetLastError();
}

namespace {
template <uint32_t MODE>
void embed_pool_go(hipStream_t st, dim3 grid, bool vec4, const float* hidden, uint32_t seq, uint32_t dim, const int32_t* mask, uint32_t mask_len,
                   uint32_t t_len, uint32_t slab_dims, float* out, uint32_t* counts) {
    if (vec4)
        hipLaunchKernelGGL((embed_pool_kernel<MODE, 4>), grid, dim3(kEmbedThreads), 0, st, hidden, seq, dim, mask, mask_len, t_len, slab_dims, out,
                           counts);
    else
        hipLaunchKernelGGL((embed_pool_kernel<MODE, 1>), grid, dim3(kEmbedThreads), 0, st, hidden, seq, dim, mask, mask_len, t_len, slab_dims, out,
                           counts);
}
} // namespace

hipError_t launch_embed_pool(hipStream_t st, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask,
                             uint32_t mask_len, uint32_t t_len, EmbedMode mode, uint32_t slab_dims, float* out, uint32_t* counts) {
    const bool vec4 = embed_vec4(hidden, out, dim);
    if (slab_dims == 0 || slab_dims > static_cast<uint32_t>(vec4 ? kEmbedSlabDims : kEmbedMinSlabDims) || (vec4 && (slab_dims & 3u)))
        return hipErrorInvalidValue;
    if (mode == kEmbedMean && !counts) return hipErrorInvalidValue;
    const dim3 grid(static_cast<uint32_t>(batch), (dim + slab_dims - 1) / slab_dims);
    if (mode == kEmbedCls) embed_pool_go<kEmbedCls>(st, grid, vec4, hidden, seq, dim, mask, mask_len, t_len, slab_dims, out, counts);
    else if (mode == kEmbedMax) embed_pool_go<kEmbedMax>(st, grid, vec4, hidden, seq, dim, mask, mask_len, t_len, slab_dims, out, counts);
    else embed_pool_go<kEmbedMean>(st, grid, vec4, hidden, seq, dim, mask, mask_len, t_len, slab_dims, out, counts);
    return hipGetLastError();
}

hipError_t launch_embed_finish(hipStream_t st, const float* rows, uint64_t batch, uint32_t dim, const uint32_t* counts, bool normalize, float* out) {
    hipLaunchKernelGGL(embed_finish_kernel, dim3(static_cast<uint32_t>(batch)), dim3(256), 0, st, rows, dim, counts, normalize ? 1u : 0u, out);
    return hipGetLastError();
}

} // namespace yams_accel
