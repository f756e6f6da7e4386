// artifact_launch.h — what artifact_kernels.hip shares with artifact_api.cpp and features_api.cpp: the launchers of the cluster
// artifacts (centroids, representatives, residual chains) and the list checks.
#pragma once
#include "common.h"

namespace yams_accel {

// flags |= 1 for offsets that do not start at 0, decrease or pass `total`; |= 2 for an index >= limit
hipError_t launch_artifact_check(hipStream_t st, const uint64_t* off, uint64_t lists, uint64_t total, const uint32_t* idx, uint32_t limit,
                                 uint32_t* flags);
hipError_t launch_artifact_check_primary(hipStream_t st, const uint32_t* primary, uint64_t n, uint32_t c, uint32_t* flags);
hipError_t launch_artifact_owner(hipStream_t st, const uint64_t* off, uint32_t lists, uint64_t total, uint32_t* owner);
hipError_t launch_artifact_centroids(hipStream_t st, const float* x, uint32_t dim, const uint64_t* off, const uint32_t* members, uint32_t c,
                                     float* out, uint32_t* out_counts);
hipError_t launch_artifact_rep_init(hipStream_t st, const uint64_t* off, uint32_t c, const uint8_t* centroid_empty, uint32_t n_extra,
                                    uint32_t* limit, uint32_t* last);
// one pass of the selection: the distances of every unused candidate, then every cluster's winner
hipError_t launch_artifact_rep_pass(hipStream_t st, const float* x, uint32_t dim, const double2* row_norm, const uint64_t* off,
                                    const uint32_t* cand, const uint32_t* owner, uint64_t total, uint32_t c, const float* cents,
                                    const double2* cent_norm, const uint32_t* limit, uint32_t* last, uint32_t s, uint32_t n_extra,
                                    uint8_t* used, double* min_dist, uint32_t* out_selected);
hipError_t launch_artifact_residual_dense(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const float* cents, uint32_t c,
                                          const uint32_t* primary, bool fused, double* out_norm, double* out_dot);
hipError_t launch_artifact_residual_list(hipStream_t st, const float* x, uint32_t dim, const float* cents, const uint32_t* primary,
                                         const uint32_t* doc_of, const uint32_t* cand, uint64_t total, bool fused, double* out_norm,
                                         double* out_dot);
hipError_t launch_artifact_primary_norm(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const float* cents, const uint32_t* primary,
                                        bool fused, double* out_norm);

} // namespace yams_accel
