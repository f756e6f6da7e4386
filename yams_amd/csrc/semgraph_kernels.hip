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
// Exactness: the product of two floats is exact in fp64, so fma(a, b, acc) == acc + a * b bit for bit; every chain walks the
// dimension in element order and is never split.  A chunk that reaches past `dim` is filled with +0.0f, which leaves a chain
// that started at +0.0 as it was (kmeans_kernels.hip gives the argument in full).
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

namespace yams_accel {

namespace {

constexpr int kSgThreads = 256;
constexpr int kSgMergeThreads = 64;      // one wave per source
constexpr int kRwChunk = 16;             // norm kernel: one row per thread, 16 elements of 256 rows per LDS stage
constexpr int kRwLds = kRwChunk + 1;
// pairs kernel: the register block of kmeans_assign_kernel
constexpr int kSgSrc = 128, kSgCand = 64, kSgChunk = 8;
constexpr int kSgRB = 8, kSgCB = 4;      // sources x candidates per lane (16 x 16 lanes)
constexpr int kSgLdA = kSgSrc + 2;       // LDS strides in doubles (16-byte aligned rows, half-chunks on different banks)
constexpr int kSgLdB = kSgCand + 2;

constexpr uint32_t kSgFlagNonFinite = 1u, kSgFlagSource = 2u, kSgFlagRank = 4u;

// Offers the (at most four per lane) pending keys of the 16 lanes that share a source to that source's list of K keys.
// Empty slots hold 0, which is below every key, so "replace the minimum while the best pending key beats it" fills the list
// first and is the reference's min-replacement loop afterwards.  All 16 lanes run the loop together (its conditions are
// uniform over them); they sit in one wave, so the LDS accesses need no barrier, only their program order.
__device__ __forceinline__ void sg_offer(uint64_t* list, uint32_t K, uint64_t (&pend)[kSgCB], int tx, uint64_t* gate) {
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
        for (int j = 0; j < kSgCB; ++j) m = pend[j] > m ? pend[j] : m;
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
            for (int j = 0; j < kSgCB; ++j) pend[j] = pend[j] == m ? 0 : pend[j];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

} // namespace

// inv[r] = graph_inverse_norm(fp64 chain of x * x).  *flags |= 1 when a sum is not finite (dim <= 4096 finite squares cannot
// overflow fp64, so that is a non-finite element) or the float inverse is +inf (every element a denormal).
__global__ __launch_bounds__(kSgThreads) void semgraph_norm_kernel(const float* __restrict__ x, uint64_t n, uint32_t dim,
                                                                   float* __restrict__ inv, uint32_t* __restrict__ flags) {
    __shared__ float tile[kSgThreads][kRwLds];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSgThreads;
    const int t = threadIdx.x, dc = t & 15;
    double s = 0.0;
    for (uint32_t d0 = 0; d0 < dim; d0 += kRwChunk) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {      // 16 lanes read the 64 contiguous bytes of one row
            const int r = (t >> 4) + 16 * i;
            const uint64_t row = base + r;
            tile[r][dc] = (row < n && d0 + dc < dim) ? x[row * dim + d0 + dc] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kRwChunk; ++e) { const double a = static_cast<double>(tile[t][e]); s = fma(a, a, s); }
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
// and, in each tile, candidates tx*4 .. +3: 32 fp64 chains, each walking the dimension sequentially, operands from LDS as in
// kmeans_assign_kernel (the next chunk's global loads are issued before this chunk's chains run).
// Dynamic LDS: lists [128][K] keys, then gates [128] (a list's current minimum: a key not above it is never offered).
// part[(source * gridDim.y + by) * K ..] receives the list; counts[0] += pairs scored, counts[1] += pairs admitted.
template <bool VEC>
__global__ __launch_bounds__(kSgThreads, 2) void semgraph_pairs_kernel(const float* __restrict__ x, uint64_t n, uint32_t dim,
                                                                     const float* __restrict__ inv, const uint32_t* __restrict__ tie_rank,
                                                                     const uint32_t* __restrict__ source_rows, uint64_t n_sources,
                                                                     uint32_t K, uint32_t explicit_threshold, float threshold,
                                                                     uint32_t tiles_per_stripe, uint64_t* __restrict__ part,
                                                                     unsigned long long* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) double sa[2][kSgChunk][kSgLdA];
    __shared__ __attribute__((aligned(16))) double sb[2][kSgChunk][kSgLdB];
    __shared__ unsigned long long s_cnt[2][kSgThreads / 64];
    extern __shared__ __attribute__((aligned(16))) uint64_t sg_dyn[];
    uint64_t* lists = sg_dyn;
    uint64_t* gates = sg_dyn + static_cast<size_t>(kSgSrc) * K;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const uint64_t src0 = static_cast<uint64_t>(blockIdx.x) * kSgSrc;
    for (uint32_t i = t; i < kSgSrc * K + kSgSrc; i += kSgThreads) sg_dyn[i] = 0;

    // staging roles: A — source t/2, dimensions (t%2)*4 .. +3 of the chunk; B — candidate t/4, dimensions (t%4)*2 .. +1
    const int ar = t >> 1, ad = (t & 1) * 4, br = t >> 2, bd = (t & 3) * 2;
    const bool a_live = src0 + ar < n_sources;
    const uint64_t a_row = a_live ? (source_rows ? source_rows[src0 + ar] : src0 + ar) : 0;
    const float* a_src = x + a_row * dim;
    const uint32_t n_chunks = (dim + kSgChunk - 1) / kSgChunk;
    const uint64_t n_tiles = (n + kSgCand - 1) / kSgCand;
    const uint64_t tile_lo = static_cast<uint64_t>(blockIdx.y) * tiles_per_stripe;
    const uint64_t tile_hi = tile_lo + tiles_per_stripe < n_tiles ? tile_lo + tiles_per_stripe : n_tiles;
    const bool expl = explicit_threshold != 0;
    uint32_t scored = 0, admitted = 0;

    for (uint64_t tile = tile_lo; tile < tile_hi; ++tile) {
        const uint64_t c0 = tile * kSgCand;
        const uint64_t b_row = c0 + br;
        const bool b_live = b_row < n;
        const float* b_src = x + (b_live ? b_row : 0) * dim;
        float fa[4], fb[2];
        auto load = [&](uint32_t d0) {
            if (VEC) {   // dim % 4 == 0 and a 16-byte aligned base: whole vectors are inside the row
                const float4 v = (a_live && d0 + ad < dim) ? *reinterpret_cast<const float4*>(a_src + d0 + ad) : make_float4(0.f, 0.f, 0.f, 0.f);
                fa[0] = v.x; fa[1] = v.y; fa[2] = v.z; fa[3] = v.w;
                const float2 w = (b_live && d0 + bd < dim) ? *reinterpret_cast<const float2*>(b_src + d0 + bd) : make_float2(0.f, 0.f);
                fb[0] = w.x; fb[1] = w.y;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) fa[e] = (a_live && d0 + ad + e < dim) ? a_src[d0 + ad + e] : 0.0f;
#pragma unroll
                for (int e = 0; e < 2; ++e) fb[e] = (b_live && d0 + bd + e < dim) ? b_src[d0 + bd + e] : 0.0f;
            }
        };
        auto store = [&](int buf) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sa[buf][ad + e][ar] = static_cast<double>(fa[e]);
#pragma unroll
            for (int e = 0; e < 2; ++e) sb[buf][bd + e][br] = static_cast<double>(fb[e]);
        };
        double acc[kSgRB][kSgCB];
#pragma unroll
        for (int i = 0; i < kSgRB; ++i)
#pragma unroll
            for (int j = 0; j < kSgCB; ++j) acc[i][j] = 0.0;

        __syncthreads();          // the previous tile's last chunk has been read by every lane (first tile: the lists are zeroed)
        load(0);
        store(0);
        __syncthreads();
        for (uint32_t ch = 0; ch < n_chunks; ++ch) {
            const int buf = ch & 1;
            const bool more = ch + 1 < n_chunks;
            if (more) load((ch + 1) * kSgChunk);
#pragma unroll 2      // (a full unroll hoists every LDS read of the chunk and spills)
            for (int e = 0; e < kSgChunk; ++e) {
                double a[kSgRB], b[kSgCB];
#pragma unroll
                for (int i = 0; i < kSgRB; i += 2) {
                    const double2 v = *reinterpret_cast<const double2*>(&sa[buf][e][ty * kSgRB + i]);
                    a[i] = v.x; a[i + 1] = v.y;
                }
#pragma unroll
                for (int j = 0; j < kSgCB; j += 2) {
                    const double2 v = *reinterpret_cast<const double2*>(&sb[buf][e][tx * kSgCB + j]);
                    b[j] = v.x; b[j + 1] = v.y;
                }
#pragma unroll
                for (int i = 0; i < kSgRB; ++i)
#pragma unroll
                    for (int j = 0; j < kSgCB; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
            }
            if (more) store(buf ^ 1);
            __syncthreads();
        }

        // the epilogue: similarity in the reference's operand order, self, admission, key, the source's best-K
        float inv_c[kSgCB];
        uint32_t rank_c[kSgCB];
#pragma unroll
        for (int j = 0; j < kSgCB; ++j) {
            const uint64_t c = c0 + tx * kSgCB + j;
            inv_c[j] = c < n ? inv[c] : 0.0f;
            rank_c[j] = c < n ? (tie_rank ? tie_rank[c] : static_cast<uint32_t>(c)) : 0u;
        }
#pragma unroll
        for (int i = 0; i < kSgRB; ++i) {
            const int sl = ty * kSgRB + i;
            const uint64_t s = src0 + sl;
            const bool s_live = s < n_sources;
            const uint64_t s_row = s_live ? (source_rows ? source_rows[s] : s) : 0;
            const float inv_s = s_live ? inv[s_row] : 0.0f;
            const uint64_t gate = gates[sl];
            uint64_t pend[kSgCB];
            bool want = false;
#pragma unroll
            for (int j = 0; j < kSgCB; ++j) {
                const uint64_t c = c0 + tx * kSgCB + j;
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
    for (uint32_t i = t; i < kSgSrc * K; i += kSgThreads) {
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
            double dot = 0.0;
            for (uint32_t i = 0; i < dim; ++i) dot = fma(static_cast<double>(a[i]), static_cast<double>(b[i]), dot);
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
    const uint64_t st = (n_sources + kSgSrc - 1) / kSgSrc, ct = (n + kSgCand - 1) / kSgCand;
    uint64_t want = st >= 512 ? 1 : (512 + st - 1) / st;
    const uint64_t most = ct / 4 > 0 ? ct / 4 : 1;
    if (want > most) want = most;
    const uint64_t per = (ct + want - 1) / want;
    *source_tiles = static_cast<uint32_t>(st);
    *tiles_per_stripe = static_cast<uint32_t>(per);
    *stripes = static_cast<uint32_t>((ct + per - 1) / per);
}

size_t semgraph_pairs_lds(uint32_t K) { return (static_cast<size_t>(kSgSrc) * K + kSgSrc) * sizeof(uint64_t); }

hipError_t launch_semgraph_pairs(hipStream_t st, const float* x, uint64_t n, uint32_t dim, const float* inv, const uint32_t* tie_rank,
                                 const uint32_t* source_rows, uint64_t n_sources, uint32_t K, bool explicit_threshold, float threshold,
                                 uint32_t source_tiles, uint32_t stripes, uint32_t tiles_per_stripe, uint64_t* part,
                                 unsigned long long* counts) {
    const bool vec = dim % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
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
