// features_launch.h — what features_kernels.hip and features_api.cpp share: the launchers of the topology build's input
// features (aggregateEmbedding, computeVarianceWeights' two passes, composeFeatureVector).
#pragma once
#include "common.h"

namespace yams_accel {

constexpr uint32_t kFeatMaxDim = 4096u;         // YAMS_FEATURES_MAX_DIM: dim, K and sketch_dim
constexpr uint32_t kFeatMaxSigLen = 65536u;     // YAMS_FEATURES_MAX_SIG_LEN: float(count) == the `+= 1.0F` chain below 2^24
constexpr int kFeatVarLanes = 64;               // dimensions per workgroup of the variance chains (one wave)
constexpr int kFeatVarRows = 8;                 // sample rows whose loads are in flight per lane

// out[d][:] = rows[records[off[d]]] (+ the later records, in list order) (/ float(count) when count > 1); zeros for an empty
// list.  out_counts[d] = the list's length.  One chain per (document, dimension), one lane each.
hipError_t launch_features_aggregate(hipStream_t st, const float* rows, uint32_t dim, const uint64_t* doc_offsets, const uint32_t* records,
                                     uint32_t n_docs, float* out, uint32_t* out_counts);
// out_mean[d], out_var[d] over the m sample rows select[0 .. m) (the rows 0 .. m-1 without select): two fp64 chains per
// dimension in sample order, one lane each.  m >= 1.
hipError_t launch_features_variance(hipStream_t st, const float* rows, uint32_t dim, const uint32_t* select, uint32_t m, bool fused,
                                    double* out_mean, double* out_var);
// nsq[i] = the fp64 chain of squares of row i's dense view in element order: the row itself (kept == null, kc == dim) or
// dense[i][kept[j]] * kept_w[j] (an fp32 multiply), j = 0 .. kc-1.  kc >= 1.
hipError_t launch_features_row_nsq(hipStream_t st, const float* dense, uint64_t n, uint32_t dim, const uint32_t* kept, const float* kept_w,
                                   uint32_t kc, double* nsq);
struct FeatComposeArgs {
    const float* dense; uint64_t n; uint32_t dim;
    const uint32_t* kept; const float* kept_w; uint32_t kc;      // the dense view's length is kc (== dim without weights)
    const double* nsq;                                           // [n] (unused when kc == 0)
    const float* entity; uint32_t k; const uint8_t* entity_on;   // entity null or k == 0: the part is off everywhere
    const uint32_t* sig; uint32_t sig_len; const uint8_t* sketch_on; uint32_t sketch_dim;      // sig null, sig_len or sketch_dim 0: off
    float alpha_e, alpha_m;
    float* out; uint32_t out_stride; uint32_t* out_dims;
};
// Everything of out but the sketch part of the rows that have one; out_dims.
hipError_t launch_features_compose_store(hipStream_t st, const FeatComposeArgs& a);
// The sketch part of the rows that have one: bucket counts, their norm, the scale by aM.
hipError_t launch_features_compose_sketch(hipStream_t st, const FeatComposeArgs& a);

} // namespace yams_accel
