// sgc_kernels.hip — gfx950 kernels of SGC smoothing: `hops` rounds of X <- D^-1/2 (A + I) D^-1/2 X over a neighbour list
// whose ORDER is an input (every output element is one fp32 chain over the row's edges in list order).
//
// Reference semantics being reproduced (src/topology/topology_sgc.cpp of the reference checkout, applySGCSmoothing):
//   :114-121  degree: deg[i] = 1.0 + the fp64 chain of double(w) over the row's edges in list order
//   :122-125  inv[i] = deg > 0 ? 1.0 / sqrt(deg) : 0.0 — a correctly rounded square root, then a correctly rounded divide
//   :144-147  self term: acc = float((inv[i] * inv[i]) * double(x[i][d]))
//   :148-153  per edge: scale = (double(w) * inv[i]) * inv[to]; an edge with scale == 0.0 is SKIPPED, not added
//   :154-157  acc = acc +f32 float(scale * double(x[to][d])): fp64 product, round to nearest even, fp32 add, denormals kept
//   :160      hop h + 1 reads the output of hop h (ping-pong buffers)
//
// Exactness: a chain (one output element) lives in ONE lane from the self term to the last edge and is never split; the
// dimension is split freely, every d being its own chain.  No atomics touch a sum, no LDS reduction exists.  The build has
// -ffp-contract=off: the fp32 add is never fused with anything.
//
// Kernels:
//   sgc_offsets_kernel   row_offsets[0] == 0, no offset decreases, nnz = row_offsets[n] < 2^32
//   sgc_degree_kernel    one lane per row, after the offsets are known good: columns < n, weights finite and >= 0, the fp64
//                        degree chain, inv[i]; the maximum degree; the list of hub rows (degree >= kSgcHubDegree)
//   sgc_finite_kernel    every element of rows is finite
//   sgc_scale_kernel     scale[e] of every edge, once (one wave per row); counts the edges of zero scale
//   sgc_hop_kernel       THE HOT PATH: a lane owns W consecutive dimensions of one row and walks the row's edges in order,
//                        the loads of kSgcDepth edges in flight before their adds run in order.  W = 4 (float4 loads when
//                        dim % 4 == 0 and the bases are aligned, element loads otherwise); hub rows are served by a second
//                        launch with W = 1 over the hub list: four times as many waves share a hub row's walk
#include <cfloat>

#include "common.h"
#include "sgc_launch.h"

namespace yams_accel {

namespace {

constexpr int kSgcThreads = 256;
constexpr int kSgcDepth = 4;                 // edges whose loads are issued before the first of their adds
constexpr uint32_t kSgcFlagOffsets = 1u, kSgcFlagColumn = 2u, kSgcFlagWeight = 4u, kSgcFlagRows = 8u, kSgcFlagNnz = 16u;

// the words of the small device block: [0] flags, [1] hub rows, [2..3] nnz, [4] max degree, [6..7] edges of zero scale
constexpr int kSgcWordFlags = 0, kSgcWordHubs = 1, kSgcWordNnz = 2, kSgcWordMaxDeg = 4, kSgcWordSkipped = 6;

} // namespace

__global__ __launch_bounds__(kSgcThreads) void sgc_offsets_kernel(const uint64_t* __restrict__ off, uint64_t n, uint32_t* __restrict__ small) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSgcThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = off[i], b = off[i + 1];
    uint32_t f = 0;
    if (b < a) f |= kSgcFlagOffsets;
    if (i == 0 && a != 0) f |= kSgcFlagOffsets;
    if (i == n - 1) {
        if (b >= (1ull << 32)) f |= kSgcFlagNnz;
        small[kSgcWordNnz] = static_cast<uint32_t>(b);
        small[kSgcWordNnz + 1] = static_cast<uint32_t>(b >> 32);
    }
    if (f) atomicOr(small + kSgcWordFlags, f);
}

// Runs after sgc_offsets_kernel on the same stream: with a flag already up the offsets cannot be trusted and nothing is walked.
__global__ __launch_bounds__(kSgcThreads) void sgc_degree_kernel(const uint64_t* __restrict__ off, const uint32_t* __restrict__ cols,
                                                                 const float* __restrict__ w, uint64_t n, double* __restrict__ inv,
                                                                 uint32_t* __restrict__ hub_rows, uint32_t* __restrict__ small) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSgcThreads + threadIdx.x;
    if (i >= n || (small[kSgcWordFlags] & (kSgcFlagOffsets | kSgcFlagNnz))) return;
    const uint64_t beg = off[i], end = off[i + 1];
    if (end > beg && (!cols || !w)) { atomicOr(small + kSgcWordFlags, kSgcFlagColumn); return; }
    double sum = 1.0;
    uint32_t f = 0;
    for (uint64_t e = beg; e < end; ++e) {
        const float we = w[e];
        if (cols[e] >= n) f |= kSgcFlagColumn;
        if (!(we >= 0.0f) || !(we <= FLT_MAX)) f |= kSgcFlagWeight;
        sum += static_cast<double>(we);
    }
    inv[i] = sum > 0.0 ? 1.0 / sqrt(sum) : 0.0;
    if (f) atomicOr(small + kSgcWordFlags, f);
    const uint32_t deg = static_cast<uint32_t>(end - beg);        // (nnz < 2^32)
    if (deg) atomicMax(small + kSgcWordMaxDeg, deg);
    if (deg >= YAMS_SGC_HUB_DEGREE) hub_rows[atomicAdd(small + kSgcWordHubs, 1u)] = static_cast<uint32_t>(i);
}

__global__ __launch_bounds__(kSgcThreads) void sgc_finite_kernel(const float* __restrict__ x, uint64_t total, uint32_t* __restrict__ small) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kSgcThreads;
    bool bad = false;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSgcThreads + threadIdx.x; i < total; i += stride)
        bad |= !(fabsf(x[i]) <= FLT_MAX);
    if (bad) atomicOr(small + kSgcWordFlags, kSgcFlagRows);
}

// One wave per row: scale[e] = (double(w) * inv[i]) * inv[to], in that operand order.
__global__ __launch_bounds__(kSgcThreads) void sgc_scale_kernel(const uint64_t* __restrict__ off, const uint32_t* __restrict__ cols,
                                                                const float* __restrict__ w, uint64_t n, const double* __restrict__ inv,
                                                                double* __restrict__ scale, uint32_t* __restrict__ small) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * (kSgcThreads / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint64_t beg = off[i], end = off[i + 1];
    const double inv_i = inv[i];
    unsigned long long skipped = 0;
    for (uint64_t e = beg + (threadIdx.x & 63); e < end; e += 64) {
        const double s = (static_cast<double>(w[e]) * inv_i) * inv[cols[e]];
        scale[e] = s;
        skipped += s == 0.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) skipped += __shfl_xor(skipped, o);
    if ((threadIdx.x & 63) == 0 && skipped) atomicAdd(reinterpret_cast<unsigned long long*>(small + kSgcWordSkipped), skipped);
}

// The launch deals (row, W consecutive dimensions) to threads with 32-bit arithmetic only; cpr = ceil(dim / W) threads serve
// a row.  cpr <= 256: a workgroup serves 256 / cpr whole rows (thread t: row t / cpr of the group).  cpr > 256: a row takes
// ceil(cpr / 256) workgroups.  sgc_hop_grid (below) is the matching count of workgroups.
// HUB == false: the rows are [0, n); a hub row (degree >= YAMS_SGC_HUB_DEGREE) is left to the other launch.
// HUB == true: the rows are hub_rows[0 .. n_hubs).  VEC (W == 4 only): float4 loads and stores.
template <int W, bool VEC, bool HUB>
__global__ __launch_bounds__(kSgcThreads) void sgc_hop_kernel(const float* __restrict__ x, float* __restrict__ y, uint64_t n, uint32_t dim,
                                                              const uint64_t* __restrict__ off, const uint32_t* __restrict__ cols,
                                                              const double* __restrict__ scale, const double* __restrict__ inv,
                                                              const uint32_t* __restrict__ hub_rows, uint32_t n_hubs) {
    static_assert(!VEC || W == 4, "the vector form is four floats wide");
    const uint32_t cpr = (dim + W - 1) / W;
    const uint32_t t = threadIdx.x;
    uint64_t r;
    uint32_t c;
    if (cpr <= kSgcThreads) {
        const uint32_t rpb = kSgcThreads / cpr, lr = t / cpr;
        if (lr >= rpb) return;
        r = static_cast<uint64_t>(blockIdx.x) * rpb + lr;
        c = t - lr * cpr;
    } else {
        const uint32_t bpr = (cpr + kSgcThreads - 1) / kSgcThreads, rb = blockIdx.x / bpr;
        r = rb;
        c = (blockIdx.x - rb * bpr) * kSgcThreads + t;
        if (c >= cpr) return;
    }
    const uint32_t d0 = c * W;
    uint64_t row;
    if (HUB) {
        if (r >= n_hubs) return;
        row = hub_rows[r];
    } else {
        if (r >= n) return;
        row = r;
    }
    const uint64_t beg = off[row], end = off[row + 1];
    if (!HUB && end - beg >= YAMS_SGC_HUB_DEGREE) return;

    auto load = [&](uint64_t src_row, float (&v)[W]) {
        const float* p = x + src_row * dim + d0;
        if (VEC) {
            const float4 q = *reinterpret_cast<const float4*>(p);
            v[0] = q.x; v[W > 1 ? 1 : 0] = q.y; v[W > 2 ? 2 : 0] = q.z; v[W > 3 ? 3 : 0] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = d0 + j < dim ? p[j] : 0.0f;
        }
    };

    float acc[W];
    {
        const double inv_i = inv[row];
        const double self = inv_i * inv_i;
        float v[W];
        load(row, v);
#pragma unroll
        for (int j = 0; j < W; ++j) acc[j] = static_cast<float>(self * static_cast<double>(v[j]));
    }
    uint64_t e = beg;
    for (; e + kSgcDepth <= end; e += kSgcDepth) {
        double s[kSgcDepth];
        float v[kSgcDepth][W];
#pragma unroll
        for (int k = 0; k < kSgcDepth; ++k) {
            s[k] = scale[e + k];
            load(cols[e + k], v[k]);
        }
#pragma unroll
        for (int k = 0; k < kSgcDepth; ++k) {
            if (s[k] == 0.0) continue;
#pragma unroll
            for (int j = 0; j < W; ++j) acc[j] = acc[j] + static_cast<float>(s[k] * static_cast<double>(v[k][j]));
        }
    }
    for (; e < end; ++e) {
        const double s = scale[e];
        float v[W];
        load(cols[e], v);
        if (s == 0.0) continue;
#pragma unroll
        for (int j = 0; j < W; ++j) acc[j] = acc[j] + static_cast<float>(s * static_cast<double>(v[j]));
    }
    float* q = y + row * dim + d0;
    if (VEC) {
        *reinterpret_cast<float4*>(q) = make_float4(acc[0], acc[W > 1 ? 1 : 0], acc[W > 2 ? 2 : 0], acc[W > 3 ? 3 : 0]);
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (d0 + j < dim) q[j] = acc[j];
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static inline uint32_t sgc_blocks(uint64_t n, uint32_t per) { return static_cast<uint32_t>((n + per - 1) / per); }

hipError_t launch_sgc_check(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const uint64_t* off, const uint32_t* cols,
                            const float* w, double* inv, uint32_t* hub_rows, uint32_t* small) {
    sgc_offsets_kernel<<<sgc_blocks(n, kSgcThreads), kSgcThreads, 0, st>>>(off, n, small);
    sgc_degree_kernel<<<sgc_blocks(n, kSgcThreads), kSgcThreads, 0, st>>>(off, cols, w, n, inv, hub_rows, small);
    const uint64_t total = n * dim;
    const uint64_t want = (total + kSgcThreads * 8ull - 1) / (kSgcThreads * 8ull);
    sgc_finite_kernel<<<static_cast<uint32_t>(want < 65536 ? want : 65536), kSgcThreads, 0, st>>>(x, total, small);
    return hipGetLastError();
}

hipError_t launch_sgc_scale(hipStream_t st, uint64_t n, const uint64_t* off, const uint32_t* cols, const float* w, const double* inv,
                            double* scale, uint32_t* small) {
    sgc_scale_kernel<<<sgc_blocks(n, kSgcThreads / 64), kSgcThreads, 0, st>>>(off, cols, w, n, inv, scale, small);
    return hipGetLastError();
}

// The number of workgroups that deal `rows` rows of cpr threads each (the rule of sgc_hop_kernel).
static uint64_t sgc_hop_grid(uint64_t rows, uint32_t cpr) {
    if (cpr <= static_cast<uint32_t>(kSgcThreads)) {
        const uint32_t rpb = kSgcThreads / cpr;
        return (rows + rpb - 1) / rpb;
    }
    return rows * ((cpr + kSgcThreads - 1) / kSgcThreads);
}

uint64_t sgc_hop_blocks(uint64_t n, uint32_t dim) { return sgc_hop_grid(n, (dim + 3) / 4); }

bool sgc_vec_loads(uint32_t dim, const float* a, const float* b, const float* c) {
    return dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

hipError_t launch_sgc_hop(hipStream_t st, const float* x, float* y, uint64_t n, uint32_t dim, const uint64_t* off, const uint32_t* cols,
                          const double* scale, const double* inv, const uint32_t* hub_rows, uint32_t n_hubs, bool vec) {
    const uint32_t blocks = static_cast<uint32_t>(sgc_hop_blocks(n, dim));
    if (vec)
        sgc_hop_kernel<4, true, false><<<blocks, kSgcThreads, 0, st>>>(x, y, n, dim, off, cols, scale, inv, nullptr, 0);
    else
        sgc_hop_kernel<4, false, false><<<blocks, kSgcThreads, 0, st>>>(x, y, n, dim, off, cols, scale, inv, nullptr, 0);
    if (n_hubs)
        sgc_hop_kernel<1, false, true><<<static_cast<uint32_t>(sgc_hop_grid(n_hubs, dim)), kSgcThreads, 0, st>>>(
            x, y, n, dim, off, cols, scale, inv, hub_rows, n_hubs);
    return hipGetLastError();
}

} // namespace yams_accel
