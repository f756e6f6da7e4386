// sgc_launch.h — what sgc_kernels.hip and sgc_api.cpp share: the launchers of applySGCSmoothing.
#pragma once
#include "common.h"

namespace yams_accel {

// The checks and the degrees.  small: 8 zeroed words ([0] flags [1] hub rows [2..3] nnz [4] max degree [6..7] zero-scale edges);
// hub_rows: [n] uint32.
hipError_t launch_sgc_check(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const uint64_t* off, const uint32_t* cols,
                            const float* w, double* inv, uint32_t* hub_rows, uint32_t* small);
hipError_t launch_sgc_scale(hipStream_t st, uint64_t n, const uint64_t* off, const uint32_t* cols, const float* w, const double* inv,
                            double* scale, uint32_t* small);
// The number of workgroups of the main launch of one hop (the caller refuses a grid beyond the launch limit).
uint64_t sgc_hop_blocks(uint64_t n, uint32_t dim);
bool sgc_vec_loads(uint32_t dim, const float* a, const float* b, const float* c);
// One hop x -> y.  vec: sgc_vec_loads over every buffer the hops of this call touch.
hipError_t launch_sgc_hop(hipStream_t st, const float* x, float* y, uint64_t n, uint32_t dim, const uint64_t* off, const uint32_t* cols,
                          const double* scale, const double* inv, const uint32_t* hub_rows, uint32_t n_hubs, bool vec);

} // namespace yams_accel
