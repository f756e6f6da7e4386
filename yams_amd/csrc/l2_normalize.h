// l2_normalize.h — the one L2 normalisation the reference's ONNX plugin applies to an embedding (onnx_colbert_session.cpp:232-245
// normalizeEmbedding; onnx_model_pool.cpp:1840-1853 and the rank-2 blocks): norm = sqrt of ONE fp64 chain of double(v) * double(v)
// in element order (exact products: form-free); norm > 1e-8: v = float(double(v) / norm), otherwise zeros — a NaN norm fails the
// comparison.  Device code of rerank_kernels.hip and embed_kernels.hip.
#pragma once
#include "common.h"

namespace yams_accel {

// ONE lane continues the chain of squares over v[0 .. n) in element order.
__device__ __forceinline__ double l2_chain(double nsq, const float* v, uint32_t n) {
    for (uint32_t d = 0; d < n; ++d) {
        const double x = static_cast<double>(v[d]);
        nsq = __dadd_rn(nsq, __dmul_rn(x, x));
    }
    return nsq;
}
__device__ __forceinline__ double l2_norm(double nsq) { return __dsqrt_rn(nsq); }
__device__ __forceinline__ float l2_quotient(float v, double norm) {
    return norm > 1e-8 ? static_cast<float>(__ddiv_rn(static_cast<double>(v), norm)) : 0.0f;
}

} // namespace yams_accel
