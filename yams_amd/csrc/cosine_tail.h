// cosine_tail.h — the tail of the topology code's cosineDistance, shared by kmeans_kernels.hip and artifact_kernels.hip
// (src/topology/topology_alternate_engines.cpp:300-304 and src/topology/topology_representatives.cpp:25-28 of the reference are
// the same three lines).  Device code for the .hip files.
#pragma once
#include "common.h"

namespace yams_accel {

// From the three fp64 sums; ra / rb = sqrt(na) / sqrt(nb).  std::clamp(v, lo, hi) is (v < lo) ? lo : (hi < v) ? hi : v: a NaN
// passes through.
__device__ __forceinline__ double km_distance(double dot, double na, double ra, double nb, double rb) {
    if (na <= 0.0 || nb <= 0.0) return 2.0;
    const double c = dot / (ra * rb);
    const double cl = (c < -1.0) ? -1.0 : ((1.0 < c) ? 1.0 : c);
    return 1.0 - cl;
}

} // namespace yams_accel
