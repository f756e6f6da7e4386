// entity_launch.h — host-visible launch descriptors for entity_kernels.hip (entity-vector search).  The gather of
// the admitted ordinals is launch_compact_rows of scan_launch.h.
#pragma once
#include "common.h"

namespace yams_accel {

hipError_t launch_entity_qnorm(hipStream_t st, const float* queries, uint32_t nq, uint32_t dim, double* qnorm);
// keys[slot][item] for every item < n_items (0 = not kept); visited / matching[q0 + slot] += the rows admitted / kept
hipError_t launch_entity_score(hipStream_t st, const float* rows, uint64_t n_rows, uint32_t dim, const float* queries,
                               const double* qnorm, const yams_scan_entity_filter_t* filters, uint32_t q0, uint32_t n_slots,
                               const yams_scan_entities_t& cols, const uint32_t* rows_sel, const unsigned long long* n_sel_dev,
                               uint64_t n_items, float threshold, unsigned long long* keys, unsigned long long* visited,
                               unsigned long long* matching);
hipError_t launch_entity_emit(hipStream_t st, const unsigned long long* res, uint64_t res_stride, const float* rows, uint32_t dim,
                              const float* queries, const double* qnorm, int64_t row_base, uint32_t q0, uint32_t n_slots,
                              uint32_t k, float* out_scores, int64_t* out_rows, uint32_t* out_counts);

} // namespace yams_accel
