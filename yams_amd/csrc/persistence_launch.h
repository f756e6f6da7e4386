// persistence_launch.h — what persistence_kernels.hip and persistence_api.cpp share: the launchers of computePersistenceH0.
#pragma once
#include "common.h"

namespace yams_accel {

constexpr uint32_t kPersistMaxPoints = 16384u;      // YAMS_QUALITY_MAX_POINTS: an m x m fp64 matrix of 2 GiB
constexpr uint32_t kPersistSelectPasses = 8u;       // the radix select: 8 bits of the 64-bit pattern per pass, high bits first
constexpr uint32_t kPersistSelectStateWords = 4u;   // uint64: [0] the prefix found so far, [1] the rank left inside it
constexpr uint32_t kPersistFlagRange = 1u, kPersistFlagNonFinite = 2u;

// flags |= kPersistFlagRange if a select entry is >= n; |= kPersistFlagNonFinite if a selected row holds a non-finite element
// (a row out of range is never read).  select nullable = the rows 0 .. m-1.
hipError_t launch_persist_check(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint32_t m,
                                uint32_t* flags);
// dist[i * m + j] = sqrt(chain of (a[k] - b[k])^2 over k in element order) for the points i, j = rows select[i], select[j]; the
// diagonal is +0.0.  Tiles that touch the upper triangle are computed, every value is stored at (i, j) and at (j, i).
hipError_t launch_persist_pairs(hipStream_t st, const float* rows, uint32_t dim, const uint32_t* select, uint32_t m, bool fused,
                                double* dist);
// state[0] = the 64-bit pattern of the order statistic `index` (0-based) of the m (m - 1) / 2 values dist[i][j], i < j.
// hist: kPersistSelectPasses * 256 uint32 of scratch; state: kPersistSelectStateWords uint64.
hipError_t launch_persist_select(hipStream_t st, const double* dist, uint32_t m, uint64_t index, uint32_t* hist, uint64_t* state);
// weights[0 .. m-2] = the edge weights of a minimum spanning tree of the complete graph over dist, in no particular order.
// Boruvka, ceil(log2 m) rounds.  scratch: persist_tree_scratch_bytes(m) bytes, 8-byte aligned.
size_t persist_tree_scratch_bytes(uint32_t m);
hipError_t launch_persist_tree(hipStream_t st, const double* dist, uint32_t m, double* weights, void* scratch);

} // namespace yams_accel
