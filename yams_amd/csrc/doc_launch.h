// doc_launch.h — host-visible launch descriptors for doc_kernels.hip (document-level selection).
#pragma once
#include "common.h"

namespace yams_accel {

// doc_key[slot][doc] = the best key of the document's allowed rows (atomicMax; zeroed by the caller), matching[q0 + slot] +=
// the rows that got a key; bit 0 of *bad_doc when row_doc holds an ordinal >= n_docs
hipError_t launch_doc_score(hipStream_t st, const float* rows, uint64_t n_rows, uint32_t dim, const float* queries,
                            const double* qnorm, uint32_t q0, uint32_t n_slots, const uint32_t* tie_rank,
                            const uint32_t* row_mask, const uint32_t* rows_sel, const unsigned long long* n_sel_dev,
                            uint64_t n_items, const uint32_t* row_doc, uint32_t n_docs, float threshold,
                            unsigned long long* doc_key, unsigned long long* matching, uint32_t* bad_doc);
hipError_t launch_doc_sel_keys(hipStream_t st, const unsigned long long* doc_key, const uint32_t* doc_rank, uint32_t n_docs,
                               uint32_t n_slots, unsigned long long* sel);
// inv[doc_rank[d]] = d; bit 1 of *bad unless doc_rank is a permutation of 0 .. n_docs - 1
hipError_t launch_doc_rank_inverse(hipStream_t st, const uint32_t* doc_rank, uint32_t n_docs, uint32_t* inv, uint32_t* bad);
hipError_t launch_doc_emit(hipStream_t st, const unsigned long long* res, uint64_t res_stride, const unsigned long long* doc_key,
                           uint32_t n_docs, const float* rows, uint32_t dim, const float* queries, const double* qnorm,
                           const uint32_t* rank_inv, const uint32_t* rank_row, int64_t row_base, uint32_t q0,
                           uint32_t n_slots, uint32_t k, float* out_scores, int64_t* out_rows, uint32_t* out_docs,
                           uint32_t* out_counts);

} // namespace yams_accel
