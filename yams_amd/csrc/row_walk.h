// row_walk.h — one row per thread, 16 elements of 256 rows per LDS stage: the walk of kmeans_norm_kernel,
// kmeans_rowdist_kernel and semgraph_norm_kernel (workgroups of 256 threads).  Device code for the .hip files.
#pragma once
#include "common.h"

namespace yams_accel {

constexpr int kRwRows = 256;
constexpr int kRwChunk = 16;
constexpr int kRwLds = kRwChunk + 1;     // padded stride (floats): thread t walks row t conflict-free
using RowWalkTile = float[kRwRows][kRwLds];

// Stages elements [d0, d0 + 16) of rows [base, base + 256) into tile (zero-filled past n / dim): 16 lanes read the 64
// contiguous bytes of one row.  The caller puts a barrier before and after.
__device__ __forceinline__ void rw_stage_rows(const float* __restrict__ x, uint64_t n, uint32_t dim, uint64_t base, uint32_t d0,
                                              RowWalkTile& tile) {
    const int t = threadIdx.x, dc = t & 15;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = (t >> 4) + 16 * i;
        const uint64_t row = base + r;
        tile[r][dc] = (row < n && d0 + dc < dim) ? x[row * dim + d0 + dc] : 0.0f;
    }
}

// s + the squares of this thread's 16 staged elements, one fp64 chain in element order (the +0.0f fill adds nothing:
// fp64_tile.h has the argument).
__device__ __forceinline__ double rw_add_squares(const RowWalkTile& tile, double s) {
#pragma unroll
    for (int e = 0; e < kRwChunk; ++e) { const double a = static_cast<double>(tile[threadIdx.x][e]); s = fma(a, a, s); }
    return s;
}

} // namespace yams_accel
