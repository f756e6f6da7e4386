// fp64_tile.h — the fp64 tile of kmeans_assign_kernel, semgraph_pairs_kernel, route_score_tile_kernel and persist_pairs_kernel:
// 128 A rows x 64 B rows of float vectors, one fp64 chain per pair (a dot product unless the caller brings its own step).
// Device code for the .hip files, plus the launchers' predicate for the VEC form.
//
// Exactness of the default step (the bit-for-bit claim of the dot-product callers lives here): the product of two floats is exact in fp64, so
// fma(a, b, acc) == acc + a * b bit for bit; every pair's chain walks the dimension in element order in ONE lane and is never
// split, so it is the reference's scalar loop.  A chunk that reaches past `dim` (and a row that is not live) is filled with
// +0.0f: a chain that starts at +0.0 can never hold -0.0 (x + y is -0.0 only when both are), so adding the exact product +0.0
// leaves every value, NaN and infinities included, as it was.  fp64 MFMA is not used: its summation order is not documented.
//
// Shape: lane (ty, tx) of 16 x 16 owns A rows ty*8 .. +7 and B rows tx*4 .. +3 — 32 chains.  Both operand chunks (8
// dimensions, converted to fp64 on the way) sit in LDS, double-buffered: the next chunk's global loads are issued before this
// chunk's chains run and stored to the other buffer after them, one barrier per chunk.  Staging roles: thread t loads A row
// t/2, dimensions (t%2)*4 .. +3 of the chunk, and B row t/4, dimensions (t%4)*2 .. +1.
#pragma once
#include "common.h"

namespace yams_accel {

constexpr int kTileThreads = 256;
constexpr int kTileA = 128, kTileB = 64, kTileChunk = 8;
constexpr int kTileRB = 8, kTileCB = 4;  // register block: A rows x B rows per lane
constexpr int kTileLdA = kTileA + 2;     // LDS strides in doubles: rows stay 16-byte aligned, and the two half-chunks a wave
constexpr int kTileLdB = kTileB + 2;     // stores (four dimensions apart) fall on different banks
using TileLdsA = double[2][kTileChunk][kTileLdA];   // declare both __shared__ __attribute__((aligned(16)))
using TileLdsB = double[2][kTileChunk][kTileLdB];

// the rows of the tile that thread t stages
__device__ __forceinline__ int tile_a_row(int t) { return t >> 1; }
__device__ __forceinline__ int tile_b_row(int t) { return t >> 2; }

// The VEC form loads float4 / float2: whole vectors are inside a row when dim % 4 == 0 and the bases are aligned.
inline bool tile_vec_loads(uint32_t dim, const float* a_base, const float* b_base) {
    return dim % 4 == 0 && (reinterpret_cast<uintptr_t>(a_base) & 15) == 0 && (reinterpret_cast<uintptr_t>(b_base) & 7) == 0;
}

// The default step of a chain: the exact-product fma the exactness argument above is about.
struct TileFmaStep {
    static __device__ __forceinline__ double step(double a, double b, double acc) { return fma(a, b, acc); }
};

// acc[i][j] = the chain of A row ty*8 + i and B row tx*4 + j over [0, dim).  a_src / b_src: the rows tile_a_row(t) /
// tile_b_row(t) (never dereferenced unless a_live / b_live).  Called by the whole workgroup; begins with a barrier (every lane
// has read the previous call's last chunk) and ends with one.
//
// The accumulate step is a parameter: acc = Step::step(a, b, acc), once per element in element order.  The staging (zero fill
// past `dim`, one barrier per chunk, double buffering) and the one-lane-per-chain order are the same for every step.  The
// exactness argument at the top of this header covers the default step only.  A caller whose step has an inexact product owns
// its own argument — what its step makes of the +0.0 fill, which host form its bits follow — as persistence_kernels.hip does
// for d = a - b, acc (+)= d * d.
template <bool VEC, class Step = TileFmaStep>
__device__ __forceinline__ void tile_chains(TileLdsA& sa, TileLdsB& sb, const float* __restrict__ a_src, bool a_live,
                                            const float* __restrict__ b_src, bool b_live, uint32_t dim,
                                            double (&acc)[kTileRB][kTileCB]) {
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int ar = tile_a_row(t), ad = (t & 1) * 4, br = tile_b_row(t), bd = (t & 3) * 2;
    const uint32_t n_chunks = (dim + kTileChunk - 1) / kTileChunk;
    float fa[4], fb[2];
    auto load = [&](uint32_t d0) {
        if (VEC) {
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
#pragma unroll
    for (int i = 0; i < kTileRB; ++i)
#pragma unroll
        for (int j = 0; j < kTileCB; ++j) acc[i][j] = 0.0;

    __syncthreads();
    load(0);
    store(0);
    __syncthreads();
    for (uint32_t ch = 0; ch < n_chunks; ++ch) {
        const int buf = ch & 1;
        const bool more = ch + 1 < n_chunks;
        if (more) load((ch + 1) * kTileChunk);
#pragma unroll 2      // (a full unroll hoists every LDS read of the chunk: 330 registers, spills)
        for (int e = 0; e < kTileChunk; ++e) {
            double a[kTileRB], b[kTileCB];
#pragma unroll
            for (int i = 0; i < kTileRB; i += 2) {
                const double2 v = *reinterpret_cast<const double2*>(&sa[buf][e][ty * kTileRB + i]);
                a[i] = v.x; a[i + 1] = v.y;
            }
#pragma unroll
            for (int j = 0; j < kTileCB; j += 2) {
                const double2 v = *reinterpret_cast<const double2*>(&sb[buf][e][tx * kTileCB + j]);
                b[j] = v.x; b[j + 1] = v.y;
            }
#pragma unroll
            for (int i = 0; i < kTileRB; ++i)
#pragma unroll
                for (int j = 0; j < kTileCB; ++j) acc[i][j] = Step::step(a[i], b[j], acc[i][j]);
        }
        if (more) store(buf ^ 1);
        __syncthreads();
    }
}

} // namespace yams_accel
