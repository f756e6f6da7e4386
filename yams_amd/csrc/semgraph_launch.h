// semgraph_launch.h — what semgraph_kernels.hip and semgraph_api.cpp share: the launchers of the semantic-neighbour self-join.
#pragma once
#include "common.h"

namespace yams_accel {

hipError_t launch_semgraph_norm(hipStream_t st, const float* x, uint64_t n, uint32_t dim, float* inv, uint32_t* flags);
hipError_t launch_semgraph_check(hipStream_t st, uint64_t n, const uint32_t* tie_rank, const uint32_t* source_rows, uint64_t n_sources,
                                 uint32_t* row_of_rank, uint32_t* flags);
// The geometry of the pairs grid: source tiles of 128, candidate tiles of 64 dealt to stripes.
void semgraph_geometry(uint64_t n, uint64_t n_sources, uint32_t* source_tiles, uint32_t* stripes, uint32_t* tiles_per_stripe);
hipError_t launch_semgraph_pairs(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const float* inv, const uint32_t* tie_rank,
                                 const uint32_t* source_rows, uint64_t n_sources, uint32_t K, bool explicit_threshold, float threshold,
                                 uint32_t source_tiles, uint32_t stripes, uint32_t tiles_per_stripe, uint64_t* part,
                                 unsigned long long* counts);
hipError_t launch_semgraph_merge(hipStream_t st, const uint64_t* part, uint32_t stripes, uint32_t K, uint64_t n_sources, const float* x,
                                 uint32_t dim, const float* inv, const uint32_t* source_rows, const uint32_t* row_of_rank,
                                 uint32_t* out_rows, float* out_sims, uint32_t* out_counts);

} // namespace yams_accel
