// kmeans_launch.h — what kmeans_kernels.hip shares with kmeans_api.cpp and artifact_api.cpp: the launchers of runKMeans and
// nearestCentroid.
#pragma once
#include "common.h"

namespace yams_accel {

// norms[r] = (na, sqrt(na)) of row r; *nonfinite (nullable) becomes non-zero when a row holds a non-finite value
hipError_t launch_kmeans_norm(hipStream_t st, const float* x, uint64_t n, uint32_t dim, double2* norms, uint32_t* nonfinite);
hipError_t launch_kmeans_init_dist(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const double2* row_norm, const float* cents,
                                   const double2* cent_norm, uint32_t centroid, const uint8_t* selected, double* min_dist,
                                   double* part_val, uint32_t* part_idx);
hipError_t launch_kmeans_own_dist(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const double2* row_norm, const float* cents,
                                  const double2* cent_norm, const uint32_t* membership, double* out_dist);
hipError_t launch_kmeans_pick(hipStream_t st, const double* part_val, const uint32_t* part_idx, uint32_t n_parts, uint32_t explicit_index,
                              const float* x, uint32_t dim, uint8_t* selected, float* cents, double2* cent_norm, uint32_t slot);
hipError_t launch_kmeans_assign(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const double2* row_norm, const float* cents,
                                const double2* cent_norm, uint32_t k, const uint8_t* skip, uint32_t* membership, uint32_t* changed,
                                uint32_t* out_assign, double* out_dist);
// counts / offsets / members of the current membership (counts must be zero on entry)
hipError_t launch_kmeans_group(hipStream_t st, const uint32_t* membership, uint64_t n, uint32_t k, uint32_t* counts, uint32_t* offsets,
                               uint32_t* members);
hipError_t launch_kmeans_centroids(hipStream_t st, const float* x, uint32_t dim, const uint32_t* members, const uint32_t* offsets,
                                   const uint32_t* counts, uint32_t k, int only, float* cents, double2* cent_norm);

} // namespace yams_accel
