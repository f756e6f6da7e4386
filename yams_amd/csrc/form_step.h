// form_step.h — the one step `acc += a * b` whose product is NOT exact in the accumulator's format, in the two forms a host
// compiler may have given it.  Device code for the .hip files.
//
// The bits of such a chain depend on whether the host contracted the step: FUSED = one fma (one rounding), otherwise the
// product is rounded, then the sum.  Both are written with explicit intrinsics, which the compiler may neither contract nor
// split whatever the file's contraction setting.  Callers: the residual chains of artifact_kernels.hip, the variance pass of
// features_kernels.hip, the pair step of persistence_kernels.hip (double); the MaxSim dot of rerank_kernels.hip (float).
#pragma once
#include <hip/hip_runtime.h>

namespace yams_accel {

template <bool FUSED> __device__ __forceinline__ double form_mul_add(double a, double b, double acc) {
    return FUSED ? __fma_rn(a, b, acc) : __dadd_rn(acc, __dmul_rn(a, b));
}
template <bool FUSED> __device__ __forceinline__ float form_mul_add(float a, float b, float acc) {
    return FUSED ? __fmaf_rn(a, b, acc) : __fadd_rn(acc, __fmul_rn(a, b));
}

} // namespace yams_accel
