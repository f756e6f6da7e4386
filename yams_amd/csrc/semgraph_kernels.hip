// semgraph_kernels.hip — gfx950 kernels of the semantic-neighbour graph: for every source document the best K other
// document-level embeddings (an exact top-K self-join).
//
// Reference semantics being reproduced (src/daemon/components/EmbeddingService.cpp of the reference checkout,
// updateSemanticNeighborGraphUnlocked; the rules themselves are contract_rules.h graph_*):
//   :405-415    inverseNorm: norm = fp64 chain of x * x in element order; inv = norm <= 0 ? 0.0f : float(1.0 / sqrt(norm))
//   :417-431    cosineSimilarity: dot = fp64 chain of double(a[i]) * double(b[i]) in element order;
//               sim = float((dot * double(invSource)) * double(invNeighbour))
//   :876-878    a row with inv <= 0 is not part of the corpus: never a candidate, and as a source it has no neighbours
//   :985        the source never lists itself
//   :991-997    admission: explicit threshold drops sim < threshold, otherwise sim <= 0.0f is dropped   (:626-632 streaming)
//   :949-954    order: similarity descending by the float compare, then document hash ascending        (:464-470 streaming)
//   :1001-1017  the min-replacement loop keeps the best K under that strict total order; they are returned sorted
//
// Exactness: every dot is one fp64 chain over the dimension in element order, never split (fp64_tile.h has the argument).
//
// The order is strict and total (a candidate's tie rank is unique), so "the best K" does not depend on the order in which
// candidates are offered: a source's list may be filled tile by tile, stripe by stripe, and merged.
//
// Kernels:
//   semgraph_norm_kernel     inv of every row; flags a non-finite sum (= a non-finite element) or an infinite inverse
//   semgraph_check_kernel    source indices < n; tie_rank -> row table (and, in a second launch, that tie_rank is a permutation)
//   semgraph_pairs_kernel    THE HOT PATH: 128 sources x 64 candidates per tile, 8 x 4 fp64 chains per lane, operands staged
//                            in LDS (double-buffered); the epilogue scores, admits, packs pack_cosine_key(sim, tie rank) and
//                            offers the key to the source's best-K list in LDS; one list per (source, candidate stripe)
//   semgraph_merge_kernel    the K best of a source's stripe lists, sorted; rows, similarities (sign of a zero restored), count
#include <cfloat>

#include "common.h"
#include "fp64_tile.h"
#include "row_walk.h"
#include "semgraph_launch.h"

namespace yams_accel {

namespace {

constexpr int kSgThreads = 256;
constexpr int kSgMergeThreads = 64;      // one wave per source
static_assert(kSgThreads == kRwRows && kSgThreads == kTileThreads, "the row walk and the tile are built for this workgroup");

constexpr uint32_t kSgFlagNonFinite = 1u, kSgFlagSource = 2u, kSgFlagRank = 4u;

// Offers the (at most four per lane) pending keys of the 16 lanes that share a source to that source's list of K keys.
// Empty slots hold 0, which is below every key, so "replace the minimum while the best pending key beats it" fills the list
// first and is the reference's min-replacement loop afterwards.  All 16 lanes run the loop together (its conditions are
// uniform over them); they sit in one wave, so the LDS accesses need no barrier, only their program order.
__device__ __forceinline__ void sg_offer(uint64_t* list, uint32_t K, uint64_t (&pend)[kTileCB], int tx, uint64_t* gate) {
    for (;;) {
        uint64_t mn = ~0ull;
        uint32_t slot = 0;
        for (uint32_t s = tx; s < K; s += 16) {
            const uint64_t v = list[s];
            if (v < mn) { mn = v; slot = s; }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            const uint64_t ov = __shfl_xor(mn, o);
            const uint32_t os = __shfl_xor(slot, o);
            if (ov < mn || (ov == mn && os < slot)) { mn = ov; slot = os; }
        }
        uint64_t m = 0;
#pragma unroll
        for (int j = 0; j < kTileCB; ++j) m = pend[j] > m ? pend[j] : m;
        const uint64_t mine = m;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            const uint64_t ov = __shfl_xor(m, o);
            m = ov > m ? ov : m;
        }
        if (m <= mn) {
            if (tx == 0) *gate = mn;
            break;
        }
        if (mine == m) {           // keys of one source are unique: exactly one lane, one slot
            list[slot] = m;
#pragma unroll
            for (int j = 0; j < kTileCB; ++j) pend[j] = pend[j] == m ? 0 : pend[j];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

} // namespace

// inv[r] = graph_inverse_norm(fp64 chain of x * x).  *flags |= 1 when a sum is not finite (dim <= 4096 finite squares cannot
// overflow fp64, so that is a non-finite element) or the float inverse is +inf (every element a denormal).
__global__ __launch_bounds__(kSgThreads) void semgraph_norm_kernel(const float* __restrict__ x, uint64_t n, uint32_t dim,
                                                                   float* __restrict__ inv, uint32_t* __restrict__ flags) {
    __shared__ RowWalkTile tile;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSgThreads;
    const int t = threadIdx.x;
    double s = 0.0;
    for (uint32_t d0 = 0; d0 < dim; d0 += kRwChunk) {
        __syncthreads();
        rw_stage_rows(x, n, dim, base, d0, tile);
        __syncthreads();
        s = rw_add_squares(tile, s);
    }
    if (base + t < n) {
        const float v = graph_inverse_norm(s);
        inv[base + t] = v;
        if (!(fabs(s) <= DBL_MAX) || !(v <= FLT_MAX)) atomicOr(flags, kSgFlagNonFinite);
    }
}

// VERIFY == false: *flags |= 2 for a source index >= n; row_of_rank[tie_rank[r]] = r (*flags |= 4 for a rank >= n).
// VERIFY == true (a second launch): *flags |= 4 unless row_of_rank[tie_rank[r]] == r, i.e. unless the ranks are distinct.
template <bool VERIFY>
__global__ __launch_bounds__(kSgThreads) void semgraph_check_kernel(uint64_t n, const uint32_t* __restrict__ tie_rank,
                                                                    const uint32_t* __restrict__ source_rows, uint64_t n_sources,
                                                                    uint32_t* __restrict__ row_of_rank, uint32_t* __restrict__ flags) {
    const uint64_t u = static_cast<uint64_t>(blockIdx.x) * kSgThreads + threadIdx.x;
    if (!VERIFY && source_rows && u < n_sources && source_rows[u] >= n) atomicOr(flags, kSgFlagSource);
    if (tie_rank && u < n) {
        const uint32_t rk = tie_rank[u];
        if (rk >= n) { if (!VERIFY) atomicOr(flags, kSgFlagRank); }
        else if (!VERIFY) row_of_rank[rk] = static_cast<uint32_t>(u);
        else if (row_of_rank[rk] != static_cast<uint32_t>(u)) atomicOr(flags, kSgFlagRank);
    }
}

// Grid (source tiles, candidate stripes).  Workgroup (bx, by) scores sources [bx * 128, +128) against the candidates of
// tiles [by * tiles_per_stripe, +tiles_per_stripe) in ascending order.  Lane (ty, tx) of 16 x 16 owns sources ty*8 .. +7
// and, in each tile, candidates tx*4 .. +3: the 32 chains of tile_chains (fp64_tile.h), A = the sources, B = the tile's
// candidates.
// Dynamic LDS: lists [128][K] keys, then gates [128] (a list's current minimum: a key not above it is never offered).
// part[(source * gridDim.y + by) * K ..] receives the list; counts[0] += pairs scored, counts[1] += pairs admitted.
template <bool VEC>
__global__ __launch_bounds__(kSgThreads, 2) void semgraph_pairs_kernel(const float* __restrict__ x, uint64_t n, uint32_t dim,
                                                                     const float* __restrict__ inv, const uint32_t* __restrict__ tie_rank,
                                                                     const uint32_t* __restrict__ source_rows, uint64_t n_sources,
                                                                     uint32_t K, uint32_t explicit_threshold, float threshold,
                                                                     uint32_t tiles_per_stripe, uint64_t* __restrict__ part,
                                                                     unsigned long long* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) TileLdsA sa;
    __shared__ __attribute__((aligned(16))) TileLdsB sb;
    __shared__ unsigned long long s_cnt[2][kSgThreads / 64];
    extern __shared__ __attribute__((aligned(16))) uint64_t sg_dyn[];
    uint64_t* lists = sg_dyn;
    uint64_t* gates = sg_dyn + static_cast<size_t>(kTileA) * K;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const uint64_t src0 = static_cast<uint64_t>(blockIdx.x) * kTileA;
    for (uint32_t i = t; i < kTileA * K + kTileA; i += kSgThreads) sg_dyn[i] = 0;

    const int ar = tile_a_row(t);
    const bool a_live = src0 + ar < n_sources;
    const uint64_t a_row = a_live ? (source_rows ? source_rows[src0 + ar] : src0 + ar) : 0;
    const float* a_src = x + a_row * dim;
    const uint64_t n_tiles = (n + kTileB - 1) / kTileB;
    const uint64_t tile_lo = static_cast<uint64_t>(blockIdx.y) * tiles_per_stripe;
    const uint64_t tile_hi = tile_lo + tiles_per_stripe < n_tiles ? tile_lo + tiles_per_stripe : n_tiles;
    const bool expl = explicit_threshold != 0;
    uint32_t scored = 0, admitted = 0;

    for (uint64_t tile = tile_lo; tile < tile_hi; ++tile) {
        const uint64_t c0 = tile * kTileB;
        const uint64_t b_row = c0 + tile_b_row(t);
        const bool b_live = b_row < n;
        const float* b_src = x + (b_live ? b_row : 0) * dim;
        double acc[kTileRB][kTileCB];
        // (its leading barrier: the previous tile's last chunk has been read by every lane; first tile: the lists are zeroed)
        tile_chains<VEC>(sa, sb, a_src, a_live, b_src, b_live, dim, acc);

        // the epilogue: similarity in the reference's operand order, self, admission, key, the source's best-K
        float inv_c[kTileCB];
        uint32_t rank_c[kTileCB];
#pragma unroll
        for (int j = 0; j < kTileCB; ++j) {
            const uint64_t c = c0 + tx * kTileCB + j;
            inv_c[j] = c < n ? inv[c] : 0.0f;
            rank_c[j] = c < n ? (tie_rank ? tie_rank[c] : static_cast<uint32_t>(c)) : 0u;
        }
#pragma unroll
        for (int i = 0; i < kTileRB; ++i) {
            const int sl = ty * kTileRB + i;
            const uint64_t s = src0 + sl;
            const bool s_live = s < n_sources;
            const uint64_t s_row = s_live ? (source_rows ? source_rows[s] : s) : 0;
            const float inv_s = s_live ? inv[s_row] : 0.0f;
            const uint64_t gate = gates[sl];
            uint64_t pend[kTileCB];
            bool want = false;
#pragma unroll
            for (int j = 0; j < kTileCB; ++j) {
                const uint64_t c = c0 + tx * kTileCB + j;
                pend[j] = 0;
                if (!(inv_s > 0.0f) || !(inv_c[j] > 0.0f) || c == s_row) continue;     // (inv_c is 0 past n)
                ++scored;
                const float sim = graph_similarity(acc[i][j], inv_s, inv_c[j]);
                if (!graph_admits(sim, expl, threshold)) continue;
                ++admitted;
                const uint64_t key = pack_cosine_key(sim, rank_c[j]);
                if (key > gate) { pend[j] = key; want = true; }
            }
            const unsigned long long bal = __ballot(want);
            if ((bal >> ((t & 48))) & 0xffffull)          // any of the 16 lanes that share this source
                sg_offer(lists + static_cast<size_t>(sl) * K, K, pend, tx, gates + sl);
        }
    }

    // the two counts: wave reduction, then one atomic each per workgroup
    unsigned long long w_scored = scored, w_admitted = admitted;      // (a lane's count fits 32 bits, a wave's need not)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { w_scored += __shfl_xor(w_scored, o); w_admitted += __shfl_xor(w_admitted, o); }
    if ((t & 63) == 0) { s_cnt[0][t >> 6] = w_scored; s_cnt[1][t >> 6] = w_admitted; }
    __syncthreads();            // (also: every list is final)
    if (t < 2) {
        unsigned long long sum = 0;
        for (int w = 0; w < kSgThreads / 64; ++w) sum += s_cnt[t][w];
        if (sum) atomicAdd(counts + t, sum);
    }
    for (uint32_t i = t; i < kTileA * K; i += kSgThreads) {
        const uint64_t s = src0 + i / K;
        if (s < n_sources) part[(s * gridDim.y + blockIdx.y) * K + i % K] = lists[i];
    }
}

// One wave per source: the K largest of its stripes * K partial keys (0 = empty), in descending order — K rounds of "the
// largest key below the previous winner" (keys of one source are unique).  Then one lane per winner writes the row (through
// row_of_rank when the key carries a tie rank) and the similarity; a key that says "zero" carries the canonical zero, so
// the pair is scored again for the sign (graph_similarity over the same chain).  Unused slots: row 0xffffffff, -inf.
__global__ __launch_bounds__(kSgMergeThreads) void semgraph_merge_kernel(const uint64_t* __restrict__ part, uint32_t stripes, uint32_t K,
                                                                        const float* __restrict__ x, uint32_t dim, const float* __restrict__ inv,
                                                                        const uint32_t* __restrict__ source_rows,
                                                                        const uint32_t* __restrict__ row_of_rank, uint32_t* __restrict__ out_rows,
                                                                        float* __restrict__ out_sims, uint32_t* __restrict__ out_counts) {
    __shared__ uint64_t win[YAMS_GRAPH_MAX_K];
    const uint64_t s = blockIdx.x;
    const int t = threadIdx.x;
    const uint64_t* keys = part + s * stripes * K;
    const uint32_t m = stripes * K;
    uint64_t prev = ~0ull;
    uint32_t count = 0;
    for (uint32_t r = 0; r < K; ++r) {
        uint64_t best = 0;
        for (uint32_t i = t; i < m; i += kSgMergeThreads) {
            const uint64_t v = keys[i];
            if (v < prev && v > best) best = v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t ov = __shfl_xor(best, o);
            best = ov > best ? ov : best;
        }
        if (best == 0) break;
        if (t == 0) win[r] = best;
        prev = best;
        ++count;
    }
    __syncthreads();
    if (t == 0) out_counts[s] = count;
    for (uint32_t r = t; r < K; r += kSgMergeThreads) {
        const uint64_t o = s * K + r;
        if (r >= count) {
            out_rows[o] = 0xffffffffu;
            out_sims[o] = -__builtin_inff();
            continue;
        }
        const uint64_t key = win[r];
        const uint32_t idx = key_idx(key);
        const uint32_t row = row_of_rank ? row_of_rank[idx] : idx;
        float sim = key_score(key);
        if (sim == 0.0f) {
            const uint64_t s_row = source_rows ? source_rows[s] : s;
            const float* a = x + s_row * dim;
            const float* b = x + static_cast<uint64_t>(row) * dim;
            double nsq, dot;
            row_sums(a, b, dim, &nsq, &dot);       // (nsq goes unused)
            sim = graph_similarity(dot, inv[s_row], inv[row]);
        }
        out_rows[o] = row;
        out_sims[o] = sim;
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static inline uint32_t sg_blocks(uint64_t n, uint32_t per) { return static_cast<uint32_t>((n + per - 1) / per); }

hipError_t launch_semgraph_norm(hipStream_t st, const float* x, uint64_t n, uint32_t dim, float* inv, uint32_t* flags) {
    semgraph_norm_kernel<<<sg_blocks(n, kSgThreads), kSgThreads, 0, st>>>(x, n, dim, inv, flags);
    return hipGetLastError();
}

hipError_t launch_semgraph_check(hipStream_t st, uint64_t n, const uint32_t* tie_rank, const uint32_t* source_rows, uint64_t n_sources,
                                 uint32_t* row_of_rank, uint32_t* flags) {
    if (!tie_rank && !source_rows) return hipSuccess;
    const uint64_t ranks = tie_rank ? n : 0, indices = source_rows ? n_sources : 0;
    const uint64_t span = ranks > indices ? ranks : indices;
    semgraph_check_kernel<false><<<sg_blocks(span, kSgThreads), kSgThreads, 0, st>>>(n, tie_rank, source_rows, n_sources, row_of_rank, flags);
    if (tie_rank)
        semgraph_check_kernel<true><<<sg_blocks(n, kSgThreads), kSgThreads, 0, st>>>(n, tie_rank, nullptr, 0, row_of_rank, flags);
    return hipGetLastError();
}

// The geometry of the pairs grid: source tiles of 128, candidate tiles of 64 dealt to stripes.  Stripes only where the source
// tiles alone leave CUs idle (two workgroups per CU, 256 CUs), and never fewer than four candidate tiles per stripe.
void semgraph_geometry(uint64_t n, uint64_t n_sources, uint32_t* source_tiles, uint32_t* stripes, uint32_t* tiles_per_stripe) {
    const uint64_t st = (n_sources + kTileA - 1) / kTileA, ct = (n + kTileB - 1) / kTileB;
    uint64_t want = st >= 512 ? 1 : (512 + st - 1) / st;
    const uint64_t most = ct / 4 > 0 ? ct / 4 : 1;
    if (want > most) want = most;
    const uint64_t per = (ct + want - 1) / want;
    *source_tiles = static_cast<uint32_t>(st);
    *tiles_per_stripe = static_cast<uint32_t>(per);
    *stripes = static_cast<uint32_t>((ct + per - 1) / per);
}

size_t semgraph_pairs_lds(uint32_t K) { return (static_cast<size_t>(kTileA) * K + kTileA) * sizeof(uint64_t); }

hipError_t launch_semgraph_pairs(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const float* inv, const uint32_t* tie_rank,
                                 const uint32_t* source_rows, uint64_t n_sources, uint32_t K, bool explicit_threshold, float threshold,
                                 uint32_t source_tiles, uint32_t stripes, uint32_t tiles_per_stripe, uint64_t* part,
                                 unsigned long long* counts) {
    const bool vec = tile_vec_loads(dim, x, x);
    const size_t lds = semgraph_pairs_lds(K);
    const dim3 grid(source_tiles, stripes);
    // static 25 KiB + lists: above 64 KiB from K = 39 on
    const void* fn = vec ? reinterpret_cast<const void*>(&semgraph_pairs_kernel<true>) : reinterpret_cast<const void*>(&semgraph_pairs_kernel<false>);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return e;
    if (vec)
        semgraph_pairs_kernel<true><<<grid, kSgThreads, lds, st>>>(x, n, dim, inv, tie_rank, source_rows, n_sources, K, explicit_threshold ? 1u : 0u,
                                                                   threshold, tiles_per_stripe, part, counts);
    else
        semgraph_pairs_kernel<false><<<grid, kSgThreads, lds, st>>>(x, n, dim, inv, tie_rank, source_rows, n_sources, K, explicit_threshold ? 1u : 0u,
                                                                    threshold, tiles_per_stripe, part, counts);
    return hipGetLastError();
}

hipError_t launch_semgraph_merge(hipStream_t st, const uint64_t* part, uint32_t stripes, uint32_t K, uint64_t n_sources, const float* x,
                                 uint32_t dim, const float* inv, const uint32_t* source_rows, const uint32_t* row_of_rank,
                                 uint32_t* out_rows, float* out_sims, uint32_t* out_counts) {
    semgraph_merge_kernel<<<static_cast<uint32_t>(n_sources), kSgMergeThreads, 0, st>>>(part, stripes, K, x, dim, inv, source_rows, row_of_rank,
                                                                                        out_rows, out_sims, out_counts);
    return hipGetLastError();
}

} // namespace yams_accel
