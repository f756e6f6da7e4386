// persistence_kernels.hip — gfx950 kernels of computePersistenceH0 over a point cloud (the centroid cloud of a topology build).
//
// Reference semantics being reproduced (paths relative to the reference checkout; the contract is restated line by line in
// include/yams_mi355x_accel.h):
//   src/search/topological_quality.cpp:51-61    pairwiseDistance: d = double(a[k]) - double(b[k]); acc += d * d in element
//                                               order; sqrt(acc)
//   src/search/topological_quality.cpp:63-71    percentile: nth_element at a host-computed index
//   src/search/topological_quality.cpp:97-126   Kruskal over the edges ascending, m - 2 merges
//
// Launches per call:
//   persist_check_kernel        a select entry >= n, a non-finite element of a selected row: found before anything is written
//   persist_pairs_kernel        THE HOT PATH: tile_chains of fp64_tile.h (the 128 x 64 tile, its staging and its 8 x 4 chains
//                               per lane, each chain in ONE lane in element order) with this file's step, PairStep, in place of
//                               the default fma: d = a - b, then acc (+)= d * d.  d * d is NOT exact in fp64 (d carries up to 53
//                               bits), so fp64_tile.h's exactness argument does not cover it and the bits depend on whether the
//                               host contracted the step into an fma: form_mul_add (form_step.h) has both forms.  What is argued
//                               here instead: a - b is one correctly rounded subtraction in either form;
//                               (-d)^2 == d^2 bit for bit, so the matrix is symmetric: only tiles that touch the upper triangle
//                               are computed (about half the work at large m), every value is stored at (i, j) and, eight
//                               consecutive doubles per lane, at (j, i).  Each (i < j) lies in exactly one computed tile, so no
//                               element is written twice.  A chunk past `dim` is filled with +0.0f on both sides: d = +0.0,
//                               d * d = +0.0, and acc (>= +0.0, never -0.0) is left as it was.
//   persist_select_hist_kernel  } x 8: an exact radix select over the 64-bit patterns of the distances i < j (non-negative
//   persist_select_pick_kernel  }      finite doubles order as their bits), 8 bits per pass from the top; equal keys share every
//                                      bin, so an index inside a plateau ends on the plateau's key
//   persist_boruvka_*_kernel    the spanning tree: Boruvka over the whole device, ceil(log2 m) rounds of four launches, each
//                               reading the matrix once.  (Prim in one workgroup, the first form, is one latency-bound step
//                               per vertex: measured 1.2 us per step at 232 points and 4.4 us at 8192, 36 ms of a 42 ms call.)
//                               The tree's m - 1 weights come out in no particular order and the host sorts them:
//                               the sorted weights of ANY minimum spanning tree are those of the reference's Kruskal (for every
//                               threshold the number of tree edges at or below it is m minus the components of the graph of
//                               such edges).
#include "common.h"
#include "form_step.h"
#include "fp64_tile.h"
#include "persistence_launch.h"

namespace yams_accel {

__global__ __launch_bounds__(256) void persist_check_kernel(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                            const uint32_t* __restrict__ select, uint32_t m,
                                                            uint32_t* __restrict__ flags) {
    const uint32_t p = blockIdx.x;
    if (p >= m) return;
    const uint64_t row = select ? select[p] : p;
    if (row >= n) {
        if (threadIdx.x == 0) atomicOr(flags, kPersistFlagRange);
        return;
    }
    const float* x = rows + row * dim;
    bool bad = false;
    for (uint32_t k = threadIdx.x; k < dim; k += 256) bad = bad || !isfinite(x[k]);
    if (bad) atomicOr(flags, kPersistFlagNonFinite);
}

// The step of pairwiseDistance for tile_chains (fp64_tile.h): d = a - b, then acc (+)= d * d in the host's form.
template <bool FUSED> struct PairStep {
    static __device__ __forceinline__ double step(double a, double b, double acc) {
        const double d = __dsub_rn(a, b);
        return form_mul_add<FUSED>(d, d, acc);
    }
};

// Grid: x = one workgroup per 128 points (the rows i of the tile), y = one per 64 points (the columns j).  A tile wholly below
// the diagonal leaves at once (before any barrier).
template <bool VEC, bool FUSED>
__global__ __launch_bounds__(kTileThreads, 2) void persist_pairs_kernel(const float* __restrict__ rows, uint32_t dim,
                                                                        const uint32_t* __restrict__ select, uint32_t m,
                                                                        double* __restrict__ dist) {
    __shared__ __attribute__((aligned(16))) TileLdsA sa;
    __shared__ __attribute__((aligned(16))) TileLdsB sb;
    const uint32_t row0 = blockIdx.x * kTileA, col0 = blockIdx.y * kTileB;
    if (row0 > col0 + (kTileB - 1)) return;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const uint32_t a_pt = row0 + tile_a_row(t), b_pt = col0 + tile_b_row(t);
    const bool a_live = a_pt < m, b_live = b_pt < m;
    const uint64_t a_row = a_live ? (select ? select[a_pt] : a_pt) : 0u, b_row = b_live ? (select ? select[b_pt] : b_pt) : 0u;
    double acc[kTileRB][kTileCB];
    tile_chains<VEC, PairStep<FUSED>>(sa, sb, rows + a_row * dim, a_live, rows + b_row * dim, b_live, dim, acc);
#pragma unroll
    for (int i = 0; i < kTileRB; ++i) {
        const uint32_t r = row0 + ty * kTileRB + i;
#pragma unroll
        for (int j = 0; j < kTileCB; ++j) {
            const uint32_t c = col0 + tx * kTileCB + j;
            acc[i][j] = __dsqrt_rn(acc[i][j]);
            if (r < m && c < m) {
                if (r < c) dist[static_cast<uint64_t>(r) * m + c] = acc[i][j];
                else if (r == c) dist[static_cast<uint64_t>(r) * m + c] = 0.0;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kTileCB; ++j) {
        const uint32_t c = col0 + tx * kTileCB + j;
#pragma unroll
        for (int i = 0; i < kTileRB; ++i) {
            const uint32_t r = row0 + ty * kTileRB + i;
            if (r < c && c < m) dist[static_cast<uint64_t>(c) * m + r] = acc[i][j];      // (r < c < m)
        }
    }
}

// One pass of the radix select: the histogram of byte `7 - pass` of the keys whose higher bytes equal the prefix found so far.
// A workgroup walks whole rows of the upper triangle (row b, b + grid, ...).
__global__ __launch_bounds__(256) void persist_select_hist_kernel(const double* __restrict__ dist, uint32_t m, uint32_t pass,
                                                                  const uint64_t* __restrict__ state, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    const uint32_t t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const uint64_t prefix = pass ? state[0] : 0u;
    const uint32_t shift = 56u - 8u * pass;
    for (uint32_t row = blockIdx.x; row + 1 < m; row += gridDim.x) {
        const uint64_t* p = reinterpret_cast<const uint64_t*>(dist) + static_cast<uint64_t>(row) * m;
        for (uint32_t j = row + 1 + t; j < m; j += 256) {
            const uint64_t key = p[j];
            if (pass == 0 || ((key >> shift) >> 8) == prefix) atomicAdd(&h[(key >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    if (h[t]) atomicAdd(&hist[pass * 256u + t], h[t]);
}

// The bin that holds the rank: prefix = prefix * 256 + bin, rank -= what lies below the bin.
__global__ __launch_bounds__(64) void persist_select_pick_kernel(const uint32_t* __restrict__ hist, uint32_t pass, uint64_t index,
                                                                 uint64_t* __restrict__ state) {
    if (threadIdx.x != 0) return;
    const uint64_t prefix = pass ? state[0] : 0u;
    uint64_t k = pass ? state[1] : index, below = 0;
    for (uint32_t b = 0; b < 256; ++b) {
        const uint64_t c = hist[pass * 256u + b];
        if (k < below + c) {
            state[0] = (prefix << 8) | b;
            state[1] = k - below;
            return;
        }
        below += c;
    }
}

constexpr uint64_t kNoEdge = ~0ull;      // above every weight and edge id: the pattern of a finite non-negative double is below 0x7ff0...

// The spanning tree: Boruvka over the whole device, ceil(log2 m) rounds of four launches.  Edges are ordered by
// (weight pattern, edge id), edge id = min(u, v) * m + max(u, v): a strict total order, so the edges the components choose
// form no cycle except the pair of components that choose the SAME edge, of which the lower label stays a root.  A component is
// named by one of its vertices (its root).  Per round:
//   vertex   one workgroup per vertex: the least edge of its row that leaves its component -> vw / ve, and the least weight
//            per component by a 64-bit atomicMin (an integer minimum: the order of arrival is free)
//   edge     among the vertices that hold their component's least weight, the least edge id
//   hook     every root hangs itself under the other end's component and hands the edge's weight out (slot by atomicAdd: the
//            host sorts the weights)
//   jump     every vertex follows the hooks to its new root (a forest: the walk is bounded by m all the same) and the
//            per-component minima are reset for the next round
// A round at least halves the number of components; rounds after the last merge find no leaving edge and change nothing.
struct BoruvkaState {
    uint64_t* vw; uint64_t* ve;              // [m] per vertex: its least leaving edge
    uint64_t* best_w; uint64_t* best_e;      // [m] per component (indexed by the root): the component's least leaving edge
    uint32_t* comp; uint32_t* parent;        // [m] the root of every vertex; the hook of every root
    uint32_t* count;                         // weights handed out so far
};

__global__ __launch_bounds__(256) void persist_boruvka_init_kernel(BoruvkaState s, uint32_t m) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u < m) { s.comp[u] = u; s.parent[u] = u; s.best_w[u] = kNoEdge; s.best_e[u] = kNoEdge; }
    if (u == 0) *s.count = 0;
}

__global__ __launch_bounds__(256) void persist_boruvka_vertex_kernel(const double* __restrict__ dist, uint32_t m, BoruvkaState s) {
    __shared__ uint64_t s_w[4], s_e[4];
    const uint32_t u = blockIdx.x, t = threadIdx.x;
    const uint32_t cu = s.comp[u];
    const uint64_t* row = reinterpret_cast<const uint64_t*>(dist) + static_cast<uint64_t>(u) * m;
    uint64_t bw = kNoEdge, be = kNoEdge;
    for (uint32_t v = t; v < m; v += 256) {
        if (s.comp[v] == cu) continue;
        const uint64_t w = row[v];
        const uint64_t e = u < v ? static_cast<uint64_t>(u) * m + v : static_cast<uint64_t>(v) * m + u;
        if (w < bw || (w == bw && e < be)) { bw = w; be = e; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t ow = __shfl_xor(static_cast<unsigned long long>(bw), o);
        const uint64_t oe = __shfl_xor(static_cast<unsigned long long>(be), o);
        if (ow < bw || (ow == bw && oe < be)) { bw = ow; be = oe; }
    }
    if ((t & 63u) == 0) { s_w[t >> 6] = bw; s_e[t >> 6] = be; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (s_w[w] < bw || (s_w[w] == bw && s_e[w] < be)) { bw = s_w[w]; be = s_e[w]; }
        s.vw[u] = bw; s.ve[u] = be;
        if (be != kNoEdge) atomicMin(reinterpret_cast<unsigned long long*>(s.best_w + cu), static_cast<unsigned long long>(bw));
    }
}

__global__ __launch_bounds__(256) void persist_boruvka_edge_kernel(uint32_t m, BoruvkaState s) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= m || s.ve[u] == kNoEdge) return;
    const uint32_t cu = s.comp[u];
    if (s.vw[u] == s.best_w[cu]) atomicMin(reinterpret_cast<unsigned long long*>(s.best_e + cu), static_cast<unsigned long long>(s.ve[u]));
}

__global__ __launch_bounds__(256) void persist_boruvka_hook_kernel(uint32_t m, BoruvkaState s, double* __restrict__ weights) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= m || s.comp[c] != c) return;      // roots only
    const uint64_t e = s.best_e[c];
    if (e == kNoEdge) return;                  // no leaving edge: the tree is complete
    const uint32_t a = static_cast<uint32_t>(e / m), b = static_cast<uint32_t>(e % m);      // (e < m * m: both are vertices)
    const uint32_t ca = s.comp[a], other = ca == c ? s.comp[b] : ca;
    if (s.best_e[other] == e && c < other) return;      // both chose this edge: the higher label hooks, this one stays a root
    s.parent[c] = other;
    const uint32_t slot = atomicAdd(s.count, 1u);
    if (slot + 1 < m) weights[slot] = __longlong_as_double(static_cast<long long>(s.best_w[c]));      // (m - 1 merges in all)
}

__global__ __launch_bounds__(256) void persist_boruvka_jump_kernel(uint32_t m, BoruvkaState s) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= m) return;
    uint32_t x = s.comp[u];
    for (uint32_t i = 0; i < m && s.parent[x] != x; ++i) x = s.parent[x];      // only roots' hooks are read: nobody writes them here
    s.comp[u] = x;      // (read by nobody else in this launch)
    s.best_w[u] = kNoEdge; s.best_e[u] = kNoEdge;
}

hipError_t launch_persist_check(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint32_t m,
                                uint32_t* flags) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(persist_check_kernel, dim3(m), dim3(256), 0, st, rows, n, dim, select, m, flags);
    return hipGetLastError();
}

hipError_t launch_persist_pairs(hipStream_t st, const float* rows, uint32_t dim, const uint32_t* select, uint32_t m, bool fused,
                                double* dist) {
    if (m == 0) return hipSuccess;
    const dim3 grid((m + kTileA - 1) / kTileA, (m + kTileB - 1) / kTileB);
    const bool vec = tile_vec_loads(dim, rows, rows);
    if (vec && fused) hipLaunchKernelGGL((persist_pairs_kernel<true, true>), grid, dim3(kTileThreads), 0, st, rows, dim, select, m, dist);
    else if (vec) hipLaunchKernelGGL((persist_pairs_kernel<true, false>), grid, dim3(kTileThreads), 0, st, rows, dim, select, m, dist);
    else if (fused) hipLaunchKernelGGL((persist_pairs_kernel<false, true>), grid, dim3(kTileThreads), 0, st, rows, dim, select, m, dist);
    else hipLaunchKernelGGL((persist_pairs_kernel<false, false>), grid, dim3(kTileThreads), 0, st, rows, dim, select, m, dist);
    return hipGetLastError();
}

hipError_t launch_persist_select(hipStream_t st, const double* dist, uint32_t m, uint64_t index, uint32_t* hist, uint64_t* state) {
    if (m < 2) return hipSuccess;
    hipError_t e = hipMemsetAsync(hist, 0, kPersistSelectPasses * 256u * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const uint32_t grid = m - 1 < 1024u ? m - 1 : 1024u;
    for (uint32_t pass = 0; pass < kPersistSelectPasses; ++pass) {
        hipLaunchKernelGGL(persist_select_hist_kernel, dim3(grid), dim3(256), 0, st, dist, m, pass, state, hist);
        hipLaunchKernelGGL(persist_select_pick_kernel, dim3(1), dim3(64), 0, st, hist, pass, index, state);
    }
    return hipGetLastError();
}

size_t persist_tree_scratch_bytes(uint32_t m) { return static_cast<size_t>(m) * (4 * 8 + 2 * 4) + 16; }

hipError_t launch_persist_tree(hipStream_t st, const double* dist, uint32_t m, double* weights, void* scratch) {
    if (m < 2) return hipSuccess;
    if (m > kPersistMaxPoints) return hipErrorInvalidValue;
    BoruvkaState s;
    s.vw = static_cast<uint64_t*>(scratch); s.ve = s.vw + m; s.best_w = s.ve + m; s.best_e = s.best_w + m;
    s.comp = reinterpret_cast<uint32_t*>(s.best_e + m); s.parent = s.comp + m; s.count = s.parent + m;
    const dim3 per_vertex((m + 255) / 256);
    hipLaunchKernelGGL(persist_boruvka_init_kernel, per_vertex, dim3(256), 0, st, s, m);
    uint32_t rounds = 0;
    while ((1u << rounds) < m) ++rounds;
    for (uint32_t r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(persist_boruvka_vertex_kernel, dim3(m), dim3(256), 0, st, dist, m, s);
        hipLaunchKernelGGL(persist_boruvka_edge_kernel, per_vertex, dim3(256), 0, st, m, s);
        hipLaunchKernelGGL(persist_boruvka_hook_kernel, per_vertex, dim3(256), 0, st, m, s, weights);
        hipLaunchKernelGGL(persist_boruvka_jump_kernel, per_vertex, dim3(256), 0, st, m, s);
    }
    return hipGetLastError();
}

} // namespace yams_accel
