// kmeans_kernels.hip — gfx950 kernels of the spherical k-means of the topology build (engine "kmeans_v1").
//
// Reference semantics being reproduced (paths relative to the reference checkout):
//   src/topology/topology_alternate_engines.cpp:288-305   cosineDistance: dot, na, nb summed in fp64 element by element; 2.0 if
//                                                         na <= 0 || nb <= 0, else 1 - std::clamp(dot / (sqrt(na) * sqrt(nb)), -1, 1)
//   :307-319                                              normalized: norm^2 in fp64, inv = float(1.0 / sqrt(norm)), x *= inv in fp32;
//                                                         a zero vector stays as it is
//   :321-336                                              nearestCentroid: strict <, lowest index wins, empty centroids skipped
//   :341-478                                              runKMeans: farthest-first initialisation, Lloyd iterations, empty-cluster repair
//   src/topology/topology_build_utils.h:27-56             meanEmbedding: fp32 running sum over the members in list order, / float(count)
//
// Exactness: every chain walks its elements in the reference's order (the dimension for a distance — fp64_tile.h has the
// argument — and the member list for a mean) and is never split.
// na / nb are per-row / per-centroid: computed once by the same chain, kept as (sum, sqrt(sum)).
//
// Kernels:
//   kmeans_norm_kernel       (na, sqrt(na)) of every row of a matrix; flags a non-finite sum (= a non-finite element: the sum of
//                            dim <= 4096 finite squares cannot overflow fp64)
//   kmeans_rowdist_kernel    one distance per row, to one centroid (initialisation: updates minDist, block arg-max of it) or to the
//                            row's own centroid (the repair path)
//   kmeans_pick_kernel       finishes the arg-max (largest value, smallest index), writes normalized(row[index]) as a centroid
//   kmeans_assign_kernel     THE HOT PATH: rows x centroids distances in register blocks of fp64 chains, running nearest centroid
//   kmeans_hist / _scan / _group   stable grouping of the rows by membership (ascending row order inside a cluster)
//   kmeans_centroid_kernel   one fp32 chain per (cluster, dimension) in member order, the IEEE divide, normalized
#include <cfloat>

#include "common.h"
#include "cosine_tail.h"
#include "fp64_tile.h"
#include "kmeans_launch.h"
#include "row_walk.h"

namespace yams_accel {

namespace {

constexpr int kKmThreads = 256;
constexpr int kKmMaxDim = 4096;          // YAMS_CLUSTER_MAX_DIM: one centroid fits the 16 KiB LDS stage of pick / centroid
static_assert(kKmThreads == kRwRows && kKmThreads == kTileThreads, "the row walk and the tile are built for this workgroup");

// (cosineDistance's tail (:300-304), km_distance, is in cosine_tail.h)

// normalized (:307-319) of the `dim` floats in v (LDS), written to out (global) and back to v; then (nb, sqrt(nb)) of the
// result.  Both chains are one thread's, in element order.  Called by a whole workgroup.
__device__ __forceinline__ void km_normalize_store(float* v, uint32_t dim, float* __restrict__ out, double2* __restrict__ out_norm) {
    __shared__ float s_inv;
    __shared__ int s_scale;
    __syncthreads();
    if (threadIdx.x == 0) {
        double norm = 0.0;
        for (uint32_t i = 0; i < dim; ++i) { const double a = static_cast<double>(v[i]); norm = fma(a, a, norm); }
        s_scale = norm > 0.0;
        s_inv = s_scale ? static_cast<float>(1.0 / sqrt(norm)) : 1.0f;
    }
    __syncthreads();
    const float inv = s_inv;
    const bool scale = s_scale != 0;
    for (uint32_t i = threadIdx.x; i < dim; i += blockDim.x) {
        const float y = scale ? v[i] * inv : v[i];
        v[i] = y; out[i] = y;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double nb = 0.0;
        for (uint32_t i = 0; i < dim; ++i) { const double a = static_cast<double>(v[i]); nb = fma(a, a, nb); }
        *out_norm = make_double2(nb, sqrt(nb));
    }
}

} // namespace

// norms[r] = (sum of squares, its sqrt), fp64, element by element.  *nonfinite |= 1 when a sum is not finite.
__global__ __launch_bounds__(kKmThreads) void kmeans_norm_kernel(const float* __restrict__ x, uint64_t n, uint32_t dim,
                                                                 double2* __restrict__ norms, uint32_t* __restrict__ nonfinite) {
    __shared__ RowWalkTile tile;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kKmThreads;
    const int t = threadIdx.x;
    double s = 0.0;
    for (uint32_t d0 = 0; d0 < dim; d0 += kRwChunk) {
        __syncthreads();
        rw_stage_rows(x, n, dim, base, d0, tile);
        __syncthreads();
        s = rw_add_squares(tile, s);
    }
    if (base + t < n) {
        norms[base + t] = make_double2(s, sqrt(s));
        if (nonfinite && !(fabs(s) <= DBL_MAX)) *nonfinite = 1u;
    }
}

// d = cosineDistance(row u, centroid c(u)) for every row.  c(u) = which ? which[u] : fixed.
// INIT (:382-394): rows with selected[u] are skipped; minDist[u] = min(minDist[u], d); the block's (largest minDist, smallest
// u) goes to part_val / part_idx[blockIdx.x] (value -1.0, index 0xffffffff when every row of the block is selected).
// !INIT: out_dist[u] = d.
template <bool INIT>
__global__ __launch_bounds__(kKmThreads) void kmeans_rowdist_kernel(const float* __restrict__ x, uint64_t n, uint32_t dim,
                                                                    const double2* __restrict__ row_norm, const float* __restrict__ cents,
                                                                    const double2* __restrict__ cent_norm, const uint32_t* __restrict__ which,
                                                                    uint32_t fixed, const uint8_t* __restrict__ selected,
                                                                    double* __restrict__ min_dist, double* __restrict__ part_val,
                                                                    uint32_t* __restrict__ part_idx, double* __restrict__ out_dist) {
    __shared__ RowWalkTile tile;
    __shared__ double r_val[kKmThreads / 64];
    __shared__ uint32_t r_idx[kKmThreads / 64];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kKmThreads;
    const int t = threadIdx.x;
    const uint64_t u = base + t;
    const bool live = u < n;
    const uint32_t c = live ? (which ? which[u] : fixed) : fixed;
    const float* cv = cents + static_cast<uint64_t>(c) * dim;
    double dot = 0.0;
    for (uint32_t d0 = 0; d0 < dim; d0 += kRwChunk) {
        __syncthreads();
        rw_stage_rows(x, n, dim, base, d0, tile);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kRwChunk; ++e) {
            const float b = (d0 + e < dim) ? cv[d0 + e] : 0.0f;
            dot = fma(static_cast<double>(tile[t][e]), static_cast<double>(b), dot);
        }
    }
    double d = 2.0;
    if (live) {
        const double2 na = row_norm[u], nb = cent_norm[c];
        d = km_distance(dot, na.x, na.y, nb.x, nb.y);
    }
    if (!INIT) {
        if (live) out_dist[u] = d;
        return;
    }
    double val = -1.0;
    uint32_t idx = 0xffffffffu;
    if (live && !selected[u]) {
        double m = min_dist[u];
        if (d < m) { m = d; min_dist[u] = m; }
        val = m; idx = static_cast<uint32_t>(u);      // (m is never NaN: a NaN d does not pass `d < m`)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(val, o);
        const uint32_t oi = __shfl_xor(idx, o);
        if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
    }
    if ((t & 63) == 0) { r_val[t >> 6] = val; r_idx[t >> 6] = idx; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kKmThreads / 64; ++w)
            if (r_val[w] > val || (r_val[w] == val && r_idx[w] < idx)) { val = r_val[w]; idx = r_idx[w]; }
        part_val[blockIdx.x] = val; part_idx[blockIdx.x] = idx;
    }
}

// One workgroup.  index = n_parts ? the arg-max of the partials (largest value, smallest index: "the first u with the strictly
// largest minDist", :390-393) : *explicit_index.  selected[index] = 1 (when selected is given); cents[slot] =
// normalized(row[index]); cent_norm[slot] = its (nb, sqrt(nb)).  An arg-max without a candidate (every row selected; cannot
// happen while slot < n) leaves everything as it is.
__global__ __launch_bounds__(kKmThreads) void kmeans_pick_kernel(const double* __restrict__ part_val, const uint32_t* __restrict__ part_idx,
                                                                 uint32_t n_parts, uint32_t explicit_index, const float* __restrict__ x,
                                                                 uint32_t dim, uint8_t* __restrict__ selected, float* __restrict__ cents,
                                                                 double2* __restrict__ cent_norm, uint32_t slot) {
    __shared__ float vec[kKmMaxDim];
    __shared__ double r_val[kKmThreads];
    __shared__ uint32_t r_idx[kKmThreads];
    const int t = threadIdx.x;
    uint32_t index = explicit_index;
    if (n_parts) {
        double val = -1.0;
        uint32_t idx = 0xffffffffu;
        for (uint32_t i = t; i < n_parts; i += kKmThreads) {
            const double ov = part_val[i];
            const uint32_t oi = part_idx[i];
            if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
        }
        r_val[t] = val; r_idx[t] = idx;
        __syncthreads();
        for (int s = kKmThreads / 2; s > 0; s >>= 1) {
            if (t < s && (r_val[t + s] > r_val[t] || (r_val[t + s] == r_val[t] && r_idx[t + s] < r_idx[t]))) {
                r_val[t] = r_val[t + s]; r_idx[t] = r_idx[t + s];
            }
            __syncthreads();
        }
        index = r_idx[0];
        if (index == 0xffffffffu) return;
    }
    if (selected && t == 0) selected[index] = 1;
    const float* row = x + static_cast<uint64_t>(index) * dim;
    for (uint32_t i = t; i < dim; i += kKmThreads) vec[i] = row[i];
    km_normalize_store(vec, dim, cents + static_cast<uint64_t>(slot) * dim, cent_norm + slot);
}

// nearestCentroid (:321-336) of every row.  Grid: one workgroup per 128 rows; it walks the centroid tiles in ascending order.
// Lane (ty, tx) of 16 x 16 owns rows ty*8 .. +7 and, in each tile, centroids tx*4 .. +3: the 32 chains of tile_chains
// (fp64_tile.h), A = the rows, B = the tile's centroids.
// best = (distance, index) with "first strictly smaller wins": inside a lane the centroids come in ascending order; across
// the 16 lanes of a row the reduction is lexicographic (smaller distance, then smaller index), which picks the lowest index
// among the minima exactly as the sequential loop does.  A NaN distance never passes `<`; a row no centroid wins keeps
// (DBL_MAX, 0).  skip[c] != 0 leaves centroid c out (:326-328).  membership != nullptr: *changed = 1 when a row's answer
// differs from membership[u], which is then updated (:416-422).
template <bool VEC>
__global__ __launch_bounds__(kKmThreads, 2) void kmeans_assign_kernel(const float* __restrict__ x, uint64_t n, uint32_t dim,
                                                                   const double2* __restrict__ row_norm, const float* __restrict__ cents,
                                                                   const double2* __restrict__ cent_norm, uint32_t k,
                                                                   const uint8_t* __restrict__ skip, uint32_t* __restrict__ membership,
                                                                   uint32_t* __restrict__ changed, uint32_t* __restrict__ out_assign,
                                                                   double* __restrict__ out_dist) {
    __shared__ __attribute__((aligned(16))) TileLdsA sa;
    __shared__ __attribute__((aligned(16))) TileLdsB sb;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const uint64_t row0 = static_cast<uint64_t>(blockIdx.x) * kTileA;
    const uint64_t a_row = row0 + tile_a_row(t);
    const bool a_live = a_row < n;
    const float* a_src = x + (a_live ? a_row : 0) * dim;

    double best_d[kTileRB];
    uint32_t best_c[kTileRB];
#pragma unroll
    for (int i = 0; i < kTileRB; ++i) { best_d[i] = DBL_MAX; best_c[i] = 0; }

    for (uint32_t c0 = 0; c0 < k; c0 += kTileB) {
        const uint32_t b_cent = c0 + tile_b_row(t);
        const bool b_live = b_cent < k;
        const float* b_src = cents + static_cast<uint64_t>(b_live ? b_cent : 0) * dim;
        double acc[kTileRB][kTileCB];
        tile_chains<VEC>(sa, sb, a_src, a_live, b_src, b_live, dim, acc);
        // the distance formula and the running minimum, centroids of the lane in ascending order
#pragma unroll
        for (int j = 0; j < kTileCB; ++j) {
            const uint32_t c = c0 + tx * kTileCB + j;
            if (c >= k || (skip && skip[c])) continue;
            const double2 nb = cent_norm[c];
#pragma unroll
            for (int i = 0; i < kTileRB; ++i) {
                const uint64_t r = row0 + ty * kTileRB + i;
                const double2 na = row_norm[r < n ? r : n - 1];     // (re-read per tile: 16 registers the chains keep)
                const double d = km_distance(acc[i][j], na.x, na.y, nb.x, nb.y);
                if (d < best_d[i]) { best_d[i] = d; best_c[i] = c; }
            }
        }
    }
    // the 16 lanes of a row: lexicographic (distance, index) minimum
#pragma unroll
    for (int i = 0; i < kTileRB; ++i) {
        double d = best_d[i];
        uint32_t c = best_c[i];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            const double od = __shfl_xor(d, o);
            const uint32_t oc = __shfl_xor(c, o);
            if (od < d || (od == d && oc < c)) { d = od; c = oc; }
        }
        const uint64_t r = row0 + ty * kTileRB + i;
        if (tx == 0 && r < n) {
            if (membership) {
                if (membership[r] != c) { membership[r] = c; *changed = 1u; }
            }
            if (out_assign) out_assign[r] = c;
            if (out_dist) out_dist[r] = d;
        }
    }
}

// counts[membership[u]] += 1
__global__ __launch_bounds__(kKmThreads) void kmeans_hist_kernel(const uint32_t* __restrict__ membership, uint64_t n,
                                                                 uint32_t* __restrict__ counts) {
    const uint64_t u = static_cast<uint64_t>(blockIdx.x) * kKmThreads + threadIdx.x;
    if (u < n) atomicAdd(&counts[membership[u]], 1u);
}

// offsets[c] = counts[0] + ... + counts[c - 1], c in [0, k].  One workgroup.
__global__ __launch_bounds__(kKmThreads) void kmeans_scan_kernel(const uint32_t* __restrict__ counts, uint32_t k,
                                                                 uint32_t* __restrict__ offsets) {
    __shared__ uint32_t seg[kKmThreads];
    const int t = threadIdx.x;
    const uint32_t per = (k + kKmThreads - 1) / kKmThreads;
    const uint32_t lo = min(k, static_cast<uint32_t>(t) * per), hi = min(k, lo + per);
    uint32_t s = 0;
    for (uint32_t c = lo; c < hi; ++c) s += counts[c];
    seg[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int i = 0; i < kKmThreads; ++i) { const uint32_t v = seg[i]; seg[i] = run; run += v; }
        offsets[k] = run;
    }
    __syncthreads();
    uint32_t run = seg[t];
    for (uint32_t c = lo; c < hi; ++c) { offsets[c] = run; run += counts[c]; }
}

// members[offsets[c] ..] = the rows of cluster c in ascending order.  One workgroup per cluster walks the membership array
// (4 bytes per row and cluster: 1/dim of what the assignment pass reads per pair).
__global__ __launch_bounds__(kKmThreads) void kmeans_group_kernel(const uint32_t* __restrict__ membership, uint64_t n,
                                                                  const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                                  uint32_t* __restrict__ members) {
    __shared__ uint32_t wave_cnt[kKmThreads / 64];
    const uint32_t c = blockIdx.x;
    const uint32_t want = counts[c];
    if (want == 0) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t run = offsets[c];
    const uint32_t end = run + want;
    for (uint64_t base = 0; base < n && run < end; base += kKmThreads) {
        const uint64_t u = base + t;
        const bool mine = u < n && membership[u] == c;
        const unsigned long long bal = __ballot(mine);
        if (lane == 0) wave_cnt[w] = __popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < kKmThreads / 64; ++i) { const uint32_t v = wave_cnt[i]; if (i < w) before += v; total += v; }
        if (mine) members[run + before + __popcll(bal & ((1ull << lane) - 1ull))] = static_cast<uint32_t>(u);
        run += total;
        __syncthreads();
    }
}

// centroidOf (:403-410) of cluster c = only >= 0 ? only : blockIdx.x: per dimension an fp32 chain 0.0f + row[m0] + row[m1] + ...
// over the members in list order (meanEmbedding :43-45), / float(count) (:52-54, the IEEE divide), then normalized.  A
// cluster without members keeps its centroid (:429).
__global__ __launch_bounds__(kKmThreads) void kmeans_centroid_kernel(const float* __restrict__ x, uint32_t dim,
                                                                     const uint32_t* __restrict__ members, const uint32_t* __restrict__ offsets,
                                                                     const uint32_t* __restrict__ counts, int only, float* __restrict__ cents,
                                                                     double2* __restrict__ cent_norm) {
    __shared__ float vec[kKmMaxDim];
    const uint32_t c = only >= 0 ? static_cast<uint32_t>(only) : blockIdx.x;
    const uint32_t cnt = counts[c];
    if (cnt == 0) return;
    const uint32_t* list = members + offsets[c];
    const float fcnt = static_cast<float>(cnt);
    for (uint32_t d = threadIdx.x; d < dim; d += kKmThreads) {
        float s = 0.0f;
        for (uint32_t m = 0; m < cnt; ++m) s += x[static_cast<uint64_t>(list[m]) * dim + d];
        vec[d] = s / fcnt;
    }
    km_normalize_store(vec, dim, cents + static_cast<uint64_t>(c) * dim, cent_norm + c);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static inline uint32_t km_blocks(uint64_t n, uint32_t per) { return static_cast<uint32_t>((n + per - 1) / per); }

hipError_t launch_kmeans_norm(hipStream_t st, const float* x, uint64_t n, uint32_t dim, double2* norms, uint32_t* nonfinite) {
    if (n == 0) return hipSuccess;
    kmeans_norm_kernel<<<km_blocks(n, kKmThreads), kKmThreads, 0, st>>>(x, n, dim, norms, nonfinite);
    return hipGetLastError();
}

hipError_t launch_kmeans_init_dist(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const double2* row_norm, const float* cents,
                                   const double2* cent_norm, uint32_t centroid, const uint8_t* selected, double* min_dist,
                                   double* part_val, uint32_t* part_idx) {
    kmeans_rowdist_kernel<true><<<km_blocks(n, kKmThreads), kKmThreads, 0, st>>>(x, n, dim, row_norm, cents, cent_norm, nullptr, centroid,
                                                                                 selected, min_dist, part_val, part_idx, nullptr);
    return hipGetLastError();
}

hipError_t launch_kmeans_own_dist(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const double2* row_norm, const float* cents,
                                  const double2* cent_norm, const uint32_t* membership, double* out_dist) {
    kmeans_rowdist_kernel<false><<<km_blocks(n, kKmThreads), kKmThreads, 0, st>>>(x, n, dim, row_norm, cents, cent_norm, membership, 0,
                                                                                  nullptr, nullptr, nullptr, nullptr, out_dist);
    return hipGetLastError();
}

hipError_t launch_kmeans_pick(hipStream_t st, const double* part_val, const uint32_t* part_idx, uint32_t n_parts, uint32_t explicit_index,
                              const float* x, uint32_t dim, uint8_t* selected, float* cents, double2* cent_norm, uint32_t slot) {
    kmeans_pick_kernel<<<1, kKmThreads, 0, st>>>(part_val, part_idx, n_parts, explicit_index, x, dim, selected, cents, cent_norm, slot);
    return hipGetLastError();
}

hipError_t launch_kmeans_assign(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const double2* row_norm, const float* cents,
                                const double2* cent_norm, uint32_t k, const uint8_t* skip, uint32_t* membership, uint32_t* changed,
                                uint32_t* out_assign, double* out_dist) {
    if (n == 0) return hipSuccess;
    if (tile_vec_loads(dim, x, cents))
        kmeans_assign_kernel<true><<<km_blocks(n, kTileA), kKmThreads, 0, st>>>(x, n, dim, row_norm, cents, cent_norm, k, skip, membership,
                                                                                changed, out_assign, out_dist);
    else
        kmeans_assign_kernel<false><<<km_blocks(n, kTileA), kKmThreads, 0, st>>>(x, n, dim, row_norm, cents, cent_norm, k, skip, membership,
                                                                                 changed, out_assign, out_dist);
    return hipGetLastError();
}

hipError_t launch_kmeans_group(hipStream_t st, const uint32_t* membership, uint64_t n, uint32_t k, uint32_t* counts, uint32_t* offsets,
                               uint32_t* members) {
    kmeans_hist_kernel<<<km_blocks(n, kKmThreads), kKmThreads, 0, st>>>(membership, n, counts);
    kmeans_scan_kernel<<<1, kKmThreads, 0, st>>>(counts, k, offsets);
    kmeans_group_kernel<<<k, kKmThreads, 0, st>>>(membership, n, counts, offsets, members);
    return hipGetLastError();
}

hipError_t launch_kmeans_centroids(hipStream_t st, const float* x, uint32_t dim, const uint32_t* members, const uint32_t* offsets,
                                   const uint32_t* counts, uint32_t k, int only, float* cents, double2* cent_norm) {
    kmeans_centroid_kernel<<<only >= 0 ? 1u : k, kKmThreads, 0, st>>>(x, dim, members, offsets, counts, only, cents, cent_norm);
    return hipGetLastError();
}

} // namespace yams_accel
