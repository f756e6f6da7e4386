// row_chains.h — the row-staged fp64 scorer of doc_score_kernel and entity_score_kernel: one thread owns one row and carries
// its sum of squares and its dot products with QG queries; 256 rows go through LDS in 128-byte chunks.  Device code for the
// .hip files, plus what their launchers share (the 16-byte-load predicate, the QG choice, the launch geometry).
//
// Exactness (the bit-for-bit claim of both entries lives here): the product of two floats is exact in fp64, so
// fma(a, b, acc) == acc + a * b bit for bit; every chain walks the dimension in element order in ONE lane and is never split,
// so it is the reference's scalar loop (sqlite_vec_backend.cpp:4253-4266, vector_database.cpp:1796-1800).  What lies past
// `dim` in the last chunk, a row that is not read and the tile of a slot past `n_slots` are filled with +0.0f.  No chain that
// is looked at sums any of it (the chains stop at the chunk's length, and a dead slot's dot is the caller's to ignore), and
// the fill adds nothing where it is summed: a chain that starts at +0.0 can never hold -0.0 (x + y is -0.0 only when both
// are), so adding the exact product +0.0 leaves every finite value as it was.
//
// Operand order of the dot product's fma: (query, row).  The product is commutative, so no finite sum, no infinity and no
// "is it a NaN" depends on the order; only WHICH NaN's payload survives could.  No NaN reaches an output of either entry:
// fast_cosine_key drops the row unless nsq and the quotient are finite (fast_row_scored, fast_quotient), and the entity rule
// keeps a row only if `sim >= threshold`, false for a NaN; a dropped row is key 0, and the counts count keys.  The emit
// kernels score a zero winner again with row_sums, chains of their own.
//
// Shape: 8 lanes per row, 16 bytes per lane, so a wave loads 8 rows x 128 contiguous bytes per instruction and the workgroup
// takes 8 passes per chunk.  The next chunk's global loads are issued into registers before this chunk's chains run and are
// stored to LDS after them; two barriers per chunk (one buffer).  The LDS row stride is padded to 33 floats: thread t reads
// row t, conflict-free.
#pragma once
#include <type_traits>

#include "common.h"

namespace yams_accel {

constexpr int kRowThreads = 256;            // rows per workgroup (one per thread)
constexpr int kRowChunk = 32;               // elements of a row per LDS stage (128 bytes)
constexpr int kRowLds = kRowChunk + 1;      // padded LDS row stride (floats)
constexpr int kRowLoads = kRowChunk / 4;    // 16-byte loads per thread and stage: 8 lanes per row, 32 rows per pass, 8 passes
constexpr uint32_t kRowNone = 0xffffffffu;  // "this thread's row is not read"
using RowLdsRows = float[kRowThreads * kRowLds];    // the kernels declare these three __shared__
template <int QG> using RowLdsQueries = float[QG][kRowChunk];
using RowLdsOrdinals = uint32_t[kRowThreads];     // (tests/test_kernel_resources_cpu.py holds the kernels' static LDS to these)

// 16-byte loads: whole float4s are inside a row, and aligned, when dim % 4 == 0 and the base is 16-byte aligned
inline int row_vec4_loads(const float* rows, uint32_t dim) {
    return ((reinterpret_cast<uintptr_t>(rows) & 15u) == 0 && (dim & 3u) == 0) ? 1 : 0;
}
// The score kernels exist for QG = 1, 4 and 8 queries per workgroup: 1 when one slot, 4 up to four, else 8.
// launch(std::integral_constant<int, QG>, grid) starts <QG>: x = one workgroup per 256 items, y = one per group of QG slots.
template <typename Launch>
inline void row_chains_dispatch(uint64_t n_items, uint32_t n_slots, Launch&& launch) {
    const uint32_t gx = static_cast<uint32_t>((n_items + kRowThreads - 1) / kRowThreads);
    const auto go = [&](auto qg) { launch(qg, dim3(gx, (n_slots + qg.value - 1) / qg.value)); };
    if (n_slots == 1) go(std::integral_constant<int, 1>{});
    else if (n_slots <= 4) go(std::integral_constant<int, 4>{});
    else go(std::integral_constant<int, 8>{});
}

// up to four consecutive floats of a row (zero-filled past `left`), as one 16-byte load when the layout allows it
__device__ __forceinline__ float4 row_load4(const float* src, uint32_t left, int vec4) {
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec4 && left >= 4) {
        x = *reinterpret_cast<const float4*>(src);
    } else {
        if (left > 0) x.x = src[0];
        if (left > 1) x.y = src[1];
        if (left > 2) x.z = src[2];
        if (left > 3) x.w = src[3];
    }
    return x;
}

// nsq = the chain of squares of this thread's row, dot[j] = its chain with query q0 + slot0 + j, over [0, dim); both only
// where `on` (else 0.0).  ordinal: the row this thread owns, kRowNone when it is not to be read — a row that no query of
// the group admits is never read.  Called by the whole workgroup; its first barrier also publishes what the caller wrote to
// LDS before the call, and it ends with one.
template <int QG>
__device__ __forceinline__ void row_chains(RowLdsRows& s_rows, RowLdsQueries<QG>& s_q, RowLdsOrdinals& s_row, uint32_t ordinal,
                                           const float* __restrict__ rows, uint32_t dim, int vec4,
                                           const float* __restrict__ queries, uint32_t q0, uint32_t slot0, uint32_t n_slots,
                                           bool on, double& nsq, double (&dot)[QG]) {
    const int t = threadIdx.x;
    s_row[t] = ordinal;
    __syncthreads();

    // stage geometry: lane t loads floats v .. v + 3 of the chunk of rows (t >> 3) + 32 * it
    const int v = (t & 7) * 4;
    const float* src[kRowLoads];
#pragma unroll
    for (int it = 0; it < kRowLoads; ++it) {
        const uint32_t r = s_row[it * (kRowThreads / 8) + (t >> 3)];
        src[it] = r != kRowNone ? rows + static_cast<uint64_t>(r) * dim + v : nullptr;
    }
    float4 pre[kRowLoads];
    auto fetch = [&](uint32_t c0) {
        const uint32_t cl = dim - c0 < static_cast<uint32_t>(kRowChunk) ? dim - c0 : static_cast<uint32_t>(kRowChunk);
        const uint32_t left = static_cast<uint32_t>(v) < cl ? cl - v : 0u;
#pragma unroll
        for (int it = 0; it < kRowLoads; ++it)
            pre[it] = (src[it] && left) ? row_load4(src[it] + c0, left, vec4) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    fetch(0);

    nsq = 0.0;
#pragma unroll
    for (int j = 0; j < QG; ++j) dot[j] = 0.0;
    for (uint32_t c0 = 0; c0 < dim; c0 += kRowChunk) {
        const uint32_t cl = dim - c0 < static_cast<uint32_t>(kRowChunk) ? dim - c0 : static_cast<uint32_t>(kRowChunk);
#pragma unroll
        for (int it = 0; it < kRowLoads; ++it) {
            float* dst = s_rows + (it * (kRowThreads / 8) + (t >> 3)) * kRowLds + v;
            dst[0] = pre[it].x; dst[1] = pre[it].y; dst[2] = pre[it].z; dst[3] = pre[it].w;
        }
        for (int i = t; i < QG * kRowChunk; i += kRowThreads) {
            const int j = i / kRowChunk, e = i % kRowChunk;
            const uint32_t slot = slot0 + j;
            s_q[j][e] = (slot < n_slots && static_cast<uint32_t>(e) < cl)
                            ? queries[static_cast<uint64_t>(q0 + slot) * dim + c0 + e] : 0.f;
        }
        __syncthreads();
        // the next chunk's loads are issued before this chunk's fp64 chains and land in registers while they run
        if (c0 + kRowChunk < dim) fetch(c0 + kRowChunk);
        if (on) {
            const float* x = s_rows + t * kRowLds;
#pragma unroll 4
            for (uint32_t i = 0; i < cl; ++i) {
                const double sv = static_cast<double>(x[i]);
                nsq = fma(sv, sv, nsq);
#pragma unroll
                for (int j = 0; j < QG; ++j) dot[j] = fma(static_cast<double>(s_q[j][i]), sv, dot[j]);
            }
        }
        __syncthreads();
    }
}

} // namespace yams_accel
