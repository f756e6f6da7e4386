// route_launch.h — what route_kernels.hip and route_api.cpp share: the launchers of the cluster router's dense signal.
#pragma once
#include "common.h"

namespace yams_accel {

constexpr uint16_t kRouteCentroid = 0xffffu;   // position[] of a centroid row inside the resident index
constexpr uint32_t kRouteMaxQueries = 1024u;   // queries per call
constexpr uint32_t kRouteRowsFormMax = 8u;     // up to here the row-chain form serves a slice, beyond it the fp64 tile

// norms[r] = float(sqrt(fp64 chain of squares of row r)), element order
hipError_t launch_route_norms(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, float* norms);
// pair[q * n_rows + r] for every query q < nq of the slice and every row of the index: the mapped cosine of an evaluated
// (query, row), kRouteSkipped (-1.0f) where the reference evaluates nothing.  cand: the slice's bitset rows, nullable.
hipError_t launch_route_score(hipStream_t st, const float* vectors, const float* vnorm, const uint32_t* owner, const uint16_t* position,
                              uint32_t n_rows, uint32_t dim, const float* queries, const float* qnorm, uint32_t nq, uint32_t pos_limit,
                              const uint32_t* cand, uint32_t cand_words, float* pair);
// the fold of every (query, cluster) of the slice
hipError_t launch_route_fold(hipStream_t st, const float* pair, const uint32_t* offsets, const uint16_t* position, uint32_t n_rows,
                             uint32_t n_clusters, uint32_t nq, const uint32_t* cand, uint32_t cand_words, float* out_dense,
                             uint8_t* out_observed, uint32_t* out_evals);

} // namespace yams_accel
