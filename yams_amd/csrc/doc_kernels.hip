// doc_kernels.hip — gfx950 kernels of document-level selection (CandidateFilterMode::DocumentTopK).
//
// Reference semantics being reproduced (paths relative to the reference checkout):
//   src/vector/sqlite_vec_backend.cpp:1508-1518   the exact arm: every matching row of the candidate documents, then
//   src/vector/sqlite_vec_backend.cpp:86-125      retainBestRecordPerDocument: rows without a document_hash are dropped,
//                                                 the best row per document by (score desc, chunk_id asc), the documents
//                                                 sorted by (score desc, document_hash asc, chunk_id asc), cut to k
//   src/vector/sqlite_vec_backend.cpp:4253-4279   the fp64 cosine of every row (the fast path of the exact scan)
//
// Two launches per slice of queries:
//   doc_score_kernel   every allowed row is read from HBM once per group of QG queries (row_chains.h: 128-byte row chunks
//                      staged through LDS with 16-byte loads, the next chunk's loads in flight while this one is summed),
//                      scored in fp64 in the reference's element order, counted, and its key
//                      pack_cosine_key(sim, tie rank) reduced per document: a segmented max over the runs of equal documents
//                      inside a wave, then one atomicMax per run into doc_key[slot][doc]
//   doc_sel_keys_kernel + topk_multilevel + doc_emit_kernel
//                      the best k documents by (score desc, doc_rank asc) and their rows
#include <algorithm>

#include "common.h"
#include "doc_launch.h"
#include "row_chains.h"

namespace yams_accel {

namespace {

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int off) {
    const uint32_t lo = __shfl_up(static_cast<uint32_t>(v), off, 64);
    const uint32_t hi = __shfl_up(static_cast<uint32_t>(v >> 32), off, 64);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

} // namespace

// One thread per allowed row (rows_sel: the compacted ordinals of a sparse allow-mask, bounded by *n_sel_dev; else every
// row, skipping the clear bits of row_mask), QG queries per workgroup (blockIdx.y * QG + j of the slice).
template <int QG>
__global__ __launch_bounds__(kRowThreads) void doc_score_kernel(
    const float* __restrict__ rows, uint64_t n_rows, uint32_t dim, int vec4, const float* __restrict__ queries,
    const double* __restrict__ qnorm, uint32_t q0, uint32_t n_slots, const uint32_t* __restrict__ tie_rank,
    const uint32_t* __restrict__ row_mask, const uint32_t* __restrict__ rows_sel, const unsigned long long* n_sel_dev,
    uint64_t n_items, const uint32_t* __restrict__ row_doc, uint32_t n_docs, float threshold,
    unsigned long long* doc_key, unsigned long long* matching, uint32_t* bad_doc) {
    __shared__ RowLdsRows s_rows;
    __shared__ RowLdsQueries<QG> s_q;
    __shared__ RowLdsOrdinals s_row;
    __shared__ uint32_t s_count[QG];
    const int t = threadIdx.x, lane = t & 63;
    const uint32_t slot0 = blockIdx.y * QG;
    const uint64_t item = static_cast<uint64_t>(blockIdx.x) * kRowThreads + t;
    const uint64_t n_valid = rows_sel ? (*n_sel_dev < n_items ? *n_sel_dev : n_items) : n_items;
    bool on = item < n_valid;
    uint64_t row = 0;
    if (on) {
        row = rows_sel ? rows_sel[item] : item;
        if (row >= n_rows) on = false;
        else if (!rows_sel && row_mask && !row_allowed(row_mask, row)) on = false;
    }
    if (t < QG) s_count[t] = 0;
    // the reference's sums (:4253-4266), one sequential chain each
    double nsq, dot[QG];
    row_chains<QG>(s_rows, s_q, s_row, on ? static_cast<uint32_t>(row) : kRowNone, rows, dim, vec4, queries, q0, slot0, n_slots,
                   on, nsq, dot);

    // scores and keys: the fast path's rule (never the record path here)
    uint64_t key[QG];
    const uint32_t kidx = on ? (tie_rank ? tie_rank[row] : static_cast<uint32_t>(row)) : 0u;
#pragma unroll
    for (int j = 0; j < QG; ++j) {
        const uint32_t slot = slot0 + j;
        key[j] = (on && slot < n_slots) ? fast_cosine_key(dot[j], nsq, qnorm[q0 + slot], false, threshold, kidx) : 0;
    }
    // matching rows per query (documents or not: the reference counts them before the reduction)
#pragma unroll
    for (int j = 0; j < QG; ++j) {
        const unsigned long long ball = __ballot(key[j] != 0);
        if (lane == 0 && ball) atomicAdd(&s_count[j], static_cast<uint32_t>(__popcll(ball)));
    }
    // the document of the row; an ordinal out of range is the caller's error (reported, never written)
    uint32_t d = YAMS_SCAN_NO_DOC;
    if (on) {
        d = row_doc[row];
        if (d != YAMS_SCAN_NO_DOC && d >= n_docs) { atomicOr(bad_doc, 1u); d = YAMS_SCAN_NO_DOC; }
    }
    // segmented max over the runs of equal documents in the wave (contiguous documents: one or two runs per wave); the
    // last lane of a run holds the run's maximum.  Any layout is exact: an interleaved one only makes more runs.
    const uint32_t d_prev = __shfl_up(d, 1, 64), d_next = __shfl_down(d, 1, 64);
    int seg = (lane == 0 || d_prev != d) ? 1 : 0;
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        const int seg_l = __shfl_up(seg, off, 64);
#pragma unroll
        for (int j = 0; j < QG; ++j) {
            const uint64_t kl = shfl_up_u64(key[j], off);
            if (lane >= off && !seg && kl > key[j]) key[j] = kl;
        }
        if (lane >= off) seg |= seg_l;
    }
    const bool tail = lane == 63 || d_next != d;
    if (tail && d != YAMS_SCAN_NO_DOC) {
#pragma unroll
        for (int j = 0; j < QG; ++j)
            if (key[j]) atomicMax(doc_key + static_cast<uint64_t>(slot0 + j) * n_docs + d, static_cast<unsigned long long>(key[j]));
    }
    __syncthreads();
    if (t < QG && slot0 + t < n_slots && s_count[t]) atomicAdd(matching + q0 + slot0 + t, static_cast<unsigned long long>(s_count[t]));
}

// Selection keys: (score, doc_rank) of every document that has a row, 0 for the others.
__global__ __launch_bounds__(256) void doc_sel_keys_kernel(const unsigned long long* doc_key, const uint32_t* doc_rank,
                                                           uint32_t n_docs, uint32_t n_slots, unsigned long long* sel) {
    const uint64_t total = static_cast<uint64_t>(n_slots) * n_docs;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const unsigned long long k = doc_key[i];
        const uint32_t d = static_cast<uint32_t>(i % n_docs);
        const uint32_t r = doc_rank ? doc_rank[d] : d;
        sel[i] = k ? ((k & 0xffffffff00000000ull) | (0xffffffffull - r)) : 0ull;
    }
}

// inv[doc_rank[d]] = d; any rank out of range or repeated sets *bad (checked by doc_rank_check_kernel).
__global__ __launch_bounds__(256) void doc_rank_inverse_kernel(const uint32_t* doc_rank, uint32_t n_docs, uint32_t* inv, uint32_t* bad) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_docs) return;
    const uint32_t r = doc_rank[d];
    if (r >= n_docs) { atomicOr(bad, 2u); return; }
    inv[r] = d;
}
__global__ __launch_bounds__(256) void doc_rank_check_kernel(const uint32_t* doc_rank, uint32_t n_docs, const uint32_t* inv, uint32_t* bad) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_docs) return;
    const uint32_t r = doc_rank[d];
    if (r < n_docs && inv[r] != d) atomicOr(bad, 2u);
}

// The k winners of every slot: score, row (row_base + ordinal), document ordinal, count; unused slots -inf / -1 / NO_DOC.
// A key holds the canonical zero (-0.0f and +0.0f are one score to the reference's compares, :100-120): a winner whose
// similarity is a zero is scored again with the same chains for the sign of ITS zero.
__global__ __launch_bounds__(256) void doc_emit_kernel(const unsigned long long* res, uint64_t res_stride,
                                                       const unsigned long long* doc_key, uint32_t n_docs,
                                                       const float* __restrict__ rows, uint32_t dim,
                                                       const float* __restrict__ queries, const double* __restrict__ qnorm,
                                                       const uint32_t* rank_inv, const uint32_t* rank_row, int64_t row_base,
                                                       uint32_t q0, uint32_t k, float* out_scores, int64_t* out_rows,
                                                       uint32_t* out_docs, uint32_t* out_counts) {
    const uint32_t slot = blockIdx.x;
    const uint32_t q = q0 + slot;
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) {
        const uint64_t o = static_cast<uint64_t>(q) * k + i;
        const unsigned long long s = res ? res[static_cast<uint64_t>(slot) * res_stride + i] : 0ull;
        const uint32_t r = 0xffffffffu - static_cast<uint32_t>(s);
        // (a doc_rank that is not a permutation fails the call afterwards; nothing is read out of range meanwhile)
        const uint32_t d = (s && r < n_docs) ? (rank_inv ? rank_inv[r] : r) : YAMS_SCAN_NO_DOC;
        if (d < n_docs) {
            const unsigned long long dk = doc_key[static_cast<uint64_t>(slot) * n_docs + d];
            const uint32_t kidx = key_idx(dk);
            const uint32_t row = rank_row ? rank_row[kidx] : kidx;
            float sim = key_score(dk);
            if (sim == 0.0f) sim = exact_cosine_again(rows + static_cast<uint64_t>(row) * dim, queries + static_cast<uint64_t>(q) * dim, dim, qnorm[q]);
            out_scores[o] = sim;
            out_rows[o] = global_row_id(row_base, 0, 0, 0, row);
            if (out_docs) out_docs[o] = d;
            atomicAdd(&s_n, 1u);
        } else {
            write_empty_slot(o, out_scores, out_rows, nullptr, nullptr, out_docs);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) out_counts[q] = s_n; // (the winners are a prefix: keys are sorted, 0-padded)
}

hipError_t launch_doc_score(hipStream_t st, const float* rows, uint64_t n_rows, uint32_t dim, const float* queries,
                            const double* qnorm, uint32_t q0, uint32_t n_slots, const uint32_t* tie_rank,
                            const uint32_t* row_mask, const uint32_t* rows_sel, const unsigned long long* n_sel_dev,
                            uint64_t n_items, const uint32_t* row_doc, uint32_t n_docs, float threshold,
                            unsigned long long* doc_key, unsigned long long* matching, uint32_t* bad_doc) {
    if (n_items == 0 || n_slots == 0) return hipSuccess;
    const int vec4 = row_vec4_loads(rows, dim);
    row_chains_dispatch(n_items, n_slots, [&](auto qg, dim3 grid) {
        hipLaunchKernelGGL((doc_score_kernel<decltype(qg)::value>), grid, dim3(kRowThreads), 0, st, rows, n_rows, dim, vec4, queries,
                           qnorm, q0, n_slots, tie_rank, row_mask, rows_sel, n_sel_dev, n_items, row_doc, n_docs, threshold, doc_key,
                           matching, bad_doc);
    });
    return hipGetLastError();
}

hipError_t launch_doc_sel_keys(hipStream_t st, const unsigned long long* doc_key, const uint32_t* doc_rank, uint32_t n_docs,
                               uint32_t n_slots, unsigned long long* sel) {
    const uint64_t total = static_cast<uint64_t>(n_slots) * n_docs;
    if (total == 0) return hipSuccess;
    const uint32_t gx = static_cast<uint32_t>(std::min<uint64_t>((total + 255) / 256, 65536));
    hipLaunchKernelGGL(doc_sel_keys_kernel, dim3(gx), dim3(256), 0, st, doc_key, doc_rank, n_docs, n_slots, sel);
    return hipGetLastError();
}

hipError_t launch_doc_rank_inverse(hipStream_t st, const uint32_t* doc_rank, uint32_t n_docs, uint32_t* inv, uint32_t* bad) {
    if (n_docs == 0) return hipSuccess;
    const uint32_t gx = (n_docs + 255) / 256;
    hipLaunchKernelGGL(doc_rank_inverse_kernel, dim3(gx), dim3(256), 0, st, doc_rank, n_docs, inv, bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(doc_rank_check_kernel, dim3(gx), dim3(256), 0, st, doc_rank, n_docs, inv, bad);
    return hipGetLastError();
}

hipError_t launch_doc_emit(hipStream_t st, const unsigned long long* res, uint64_t res_stride, const unsigned long long* doc_key,
                           uint32_t n_docs, const float* rows, uint32_t dim, const float* queries, const double* qnorm,
                           const uint32_t* rank_inv, const uint32_t* rank_row, int64_t row_base, uint32_t q0,
                           uint32_t n_slots, uint32_t k, float* out_scores, int64_t* out_rows, uint32_t* out_docs,
                           uint32_t* out_counts) {
    if (n_slots == 0) return hipSuccess;
    hipLaunchKernelGGL(doc_emit_kernel, dim3(n_slots), dim3(256), 0, st, res, res_stride, doc_key, n_docs, rows, dim, queries,
                       qnorm, rank_inv, rank_row, row_base, q0, k, out_scores, out_rows, out_docs, out_counts);
    return hipGetLastError();
}

} // namespace yams_accel
