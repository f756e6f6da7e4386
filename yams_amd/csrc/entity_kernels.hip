// entity_kernels.hip — gfx950 kernels of the entity-vector search (IEntityStore::searchEntities).
//
// Reference semantics being reproduced (paths relative to the reference checkout):
//   src/vector/sqlite_vec_backend.cpp:2801-2887   searchEntities: entity_vectors WHERE [embedding_type = ?] [AND node_type = ?]
//                                                 [AND document_hash = ?] in table order, similarity = float(cosine),
//                                                 kept iff similarity >= threshold, std::sort by similarity desc, first k
//   src/vector/vector_database.cpp:1786-1810      computeCosineSimilarity: dot, norm_a, norm_b summed in fp64, element by
//                                                 element; 0.0 if either norm == 0.0 (tested BEFORE the division); no
//                                                 finiteness test, no small-norm drop, no query validation
// std::sort has one key and is not stable: the order inside a run of equal similarities (-0.0f == +0.0f) is left open by the
// reference; the rule served here is (similarity desc, row ordinal asc) — what a stable sort of the table order gives.
//
// Launches per call:
//   entity_qnorm_kernel     sqrt of the fp64 sum of squares of every query, in element order
//   compact_rows_kernel     (scan_kernels.hip) only when a row_mask or the filters restrict the rows: the ordinals some
//                           query admits
//   per slice of queries:
//   entity_score_kernel     every admitted row is read from HBM once per group of QG queries (row_chains.h: 128-byte row
//                           chunks staged through LDS with 16-byte loads, the next chunk's loads in flight while this one is summed),
//                           scored, counted, and its key pack_key(similarity with -0.0 -> +0.0, row) written
//   topk_multilevel + entity_emit_kernel   the k best keys of each query and their rows; a winner whose similarity is a
//                           zero is scored again for the sign of its zero (the key holds the canonical one)
#include <algorithm>

#include "common.h"
#include "entity_launch.h"
#include "row_chains.h"

namespace yams_accel {

// qnorm[q] = sqrt(sum of squares), fp64, element by element (norm_a of :1798,1802).  One thread per query.
__global__ __launch_bounds__(64) void entity_qnorm_kernel(const float* __restrict__ queries, uint32_t nq, uint32_t dim,
                                                          double* __restrict__ qnorm) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float* x = queries + static_cast<uint64_t>(q) * dim;
    double s = 0.0;
    for (uint32_t i = 0; i < dim; ++i) {
        const double v = static_cast<double>(x[i]);
        s = fma(v, v, s);
    }
    qnorm[q] = sqrt(s);
}

// One thread per item (rows_sel: the compacted ordinals, bounded by *n_sel_dev; else item == row), QG queries per workgroup
// (blockIdx.y * QG + j of the slice).  keys[slot][item] for every item < n_items: 0 = not kept.
template <int QG>
__global__ __launch_bounds__(kRowThreads) void entity_score_kernel(
    const float* __restrict__ rows, uint64_t n_rows, uint32_t dim, int vec4, const float* __restrict__ queries,
    const double* __restrict__ qnorm, const yams_scan_entity_filter_t* __restrict__ filters, uint32_t q0, uint32_t n_slots,
    const uint8_t* __restrict__ row_type, const uint32_t* __restrict__ row_node_type, const uint32_t* __restrict__ row_doc,
    const uint32_t* __restrict__ rows_sel, const unsigned long long* n_sel_dev, uint64_t n_items, float threshold,
    unsigned long long* __restrict__ keys, unsigned long long* visited, unsigned long long* matching) {
    __shared__ RowLdsRows s_rows;
    __shared__ RowLdsQueries<QG> s_q;
    __shared__ RowLdsOrdinals s_row;
    __shared__ uint32_t s_count[2][QG];
    const int t = threadIdx.x, lane = t & 63;
    const uint32_t slot0 = blockIdx.y * QG;
    const uint64_t item = static_cast<uint64_t>(blockIdx.x) * kRowThreads + t;
    const uint64_t n_valid = rows_sel ? (*n_sel_dev < n_items ? *n_sel_dev : n_items) : n_items;
    if (static_cast<uint64_t>(blockIdx.x) * kRowThreads >= n_valid) { // (a compacted list shorter than its bound: empty keys)
        if (item < n_items) {
#pragma unroll
            for (int j = 0; j < QG; ++j)
                if (slot0 + j < n_slots) keys[static_cast<uint64_t>(slot0 + j) * n_items + item] = 0ull;
        }
        return;
    }
    uint64_t row = 0;
    bool in = item < n_valid;
    if (in) {
        row = rows_sel ? rows_sel[item] : item;
        if (row >= n_rows) in = false;
    }
    // which queries of the group admit the row (the row_mask has been applied by the compaction)
    uint32_t adm = 0;
#pragma unroll
    for (int j = 0; j < QG; ++j) {
        const uint32_t slot = slot0 + j;
        if (in && slot < n_slots && (!filters || entity_admits(filters[q0 + slot], row_type, row_node_type, row_doc, row))) adm |= 1u << j;
    }
    const bool on = adm != 0; // a row that no query of the group admits is never read
    if (t < 2 * QG) s_count[t / QG][t % QG] = 0;
    // the reference's sums (:1796-1800), one sequential chain each
    double nsq, dot[QG];
    row_chains<QG>(s_rows, s_q, s_row, on ? static_cast<uint32_t>(row) : kRowNone, rows, dim, vec4, queries, q0, slot0, n_slots,
                   on, nsq, dot);

#pragma unroll
    for (int j = 0; j < QG; ++j) {
        const uint32_t slot = slot0 + j;
        unsigned long long key = 0;
        const bool a = (adm >> j) & 1u;
        if (a) {
            const float sim = compute_cosine_similarity(dot[j], nsq, qnorm[q0 + slot]);
            // float compare (:2862): a NaN similarity or threshold keeps nothing; -0.0f and +0.0f are one score
            if (sim >= threshold) key = pack_key(sim == 0.0f ? 0.0f : sim, static_cast<uint32_t>(row));
        }
        if (slot < n_slots && item < n_items) keys[static_cast<uint64_t>(slot) * n_items + item] = key;
        const unsigned long long ball_a = __ballot(a), ball_k = __ballot(key != 0);
        if (lane == 0 && ball_a) atomicAdd(&s_count[0][j], static_cast<uint32_t>(__popcll(ball_a)));
        if (lane == 0 && ball_k) atomicAdd(&s_count[1][j], static_cast<uint32_t>(__popcll(ball_k)));
    }
    __syncthreads();
    if (t < QG && slot0 + t < n_slots) {
        if (s_count[0][t]) atomicAdd(visited + q0 + slot0 + t, static_cast<unsigned long long>(s_count[0][t]));
        if (s_count[1][t]) atomicAdd(matching + q0 + slot0 + t, static_cast<unsigned long long>(s_count[1][t]));
    }
}

// The k winners of every slot: score, row (row_base + ordinal), count; unused slots -inf / -1.  The key of a winner whose
// similarity is a zero holds +0.0: its own bits (the reference returns -0.0f where the quotient underflows from below) come
// from scoring the row again with the same chains.
__global__ __launch_bounds__(256) void entity_emit_kernel(const unsigned long long* res, uint64_t res_stride,
                                                          const float* __restrict__ rows, uint32_t dim,
                                                          const float* __restrict__ queries, const double* __restrict__ qnorm,
                                                          int64_t row_base, uint32_t q0, uint32_t k, float* out_scores,
                                                          int64_t* out_rows, uint32_t* out_counts) {
    const uint32_t slot = blockIdx.x;
    const uint32_t q = q0 + slot;
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) {
        const uint64_t o = static_cast<uint64_t>(q) * k + i;
        const unsigned long long s = res ? res[static_cast<uint64_t>(slot) * res_stride + i] : 0ull;
        if (s) {
            const uint32_t r = key_idx(s);
            float sim = key_score(s);
            if (sim == 0.0f) {
                double nsq, dot;
                row_sums(rows + static_cast<uint64_t>(r) * dim, queries + static_cast<uint64_t>(q) * dim, dim, &nsq, &dot);
                sim = compute_cosine_similarity(dot, nsq, qnorm[q]);
            }
            out_scores[o] = sim;
            out_rows[o] = global_row_id(row_base, 0, 0, 0, r);
            atomicAdd(&s_n, 1u);
        } else {
            write_empty_slot(o, out_scores, out_rows, nullptr, nullptr, nullptr);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) out_counts[q] = s_n; // (the winners are a prefix: keys are sorted, 0-padded)
}

hipError_t launch_entity_qnorm(hipStream_t st, const float* queries, uint32_t nq, uint32_t dim, double* qnorm) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(entity_qnorm_kernel, dim3((nq + 63) / 64), dim3(64), 0, st, queries, nq, dim, qnorm);
    return hipGetLastError();
}

hipError_t launch_entity_score(hipStream_t st, const float* rows, uint64_t n_rows, uint32_t dim, const float* queries,
                               const double* qnorm, const yams_scan_entity_filter_t* filters, uint32_t q0, uint32_t n_slots,
                               const yams_scan_entities_t& cols, const uint32_t* rows_sel, const unsigned long long* n_sel_dev,
                               uint64_t n_items, float threshold, unsigned long long* keys, unsigned long long* visited,
                               unsigned long long* matching) {
    if (n_items == 0 || n_slots == 0) return hipSuccess;
    const int vec4 = row_vec4_loads(rows, dim);
    row_chains_dispatch(n_items, n_slots, [&](auto qg, dim3 grid) {
        hipLaunchKernelGGL((entity_score_kernel<decltype(qg)::value>), grid, dim3(kRowThreads), 0, st, rows, n_rows, dim, vec4, queries, qnorm,
                           filters, q0, n_slots, cols.row_type, cols.row_node_type, cols.row_doc, rows_sel, n_sel_dev, n_items,
                           threshold, keys, visited, matching);
    });
    return hipGetLastError();
}

hipError_t launch_entity_emit(hipStream_t st, const unsigned long long* res, uint64_t res_stride, const float* rows, uint32_t dim,
                              const float* queries, const double* qnorm, int64_t row_base, uint32_t q0, uint32_t n_slots,
                              uint32_t k, float* out_scores, int64_t* out_rows, uint32_t* out_counts) {
    if (n_slots == 0) return hipSuccess;
    hipLaunchKernelGGL(entity_emit_kernel, dim3(n_slots), dim3(256), 0, st, res, res_stride, rows, dim, queries, qnorm, row_base,
                       q0, k, out_scores, out_rows, out_counts);
    return hipGetLastError();
}

} // namespace yams_accel
