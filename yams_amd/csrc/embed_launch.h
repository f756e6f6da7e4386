// embed_launch.h — what embed_kernels.hip and embed_api.cpp share: the launchers of the embedding model's pooling head (CLS, max
// or mean over the tokens of each text, then the L2 normalisation).
#pragma once
#include "common.h"

namespace yams_accel {

constexpr uint32_t kEmbedMaxDim = 8192u;                 // YAMS_EMBED_MAX_DIM
constexpr uint32_t kEmbedMaxSeq = 1u << 16;              // YAMS_EMBED_MAX_SEQ: below 2^24, so the float token count is exact
constexpr uint64_t kEmbedMaxRows = 1ull << 22;           // YAMS_EMBED_MAX_ROWS: batch * seq of one call (and the rows of a normalise)
constexpr int kEmbedThreads = 64;                        // one wave per workgroup: the skip of a masked row is wave-uniform
constexpr int kEmbedWindow = 128;                        // tokens whose active indices are compacted into LDS at a time
constexpr int kEmbedAhead = 8;                           // independent row loads issued in front of the dependent chain
constexpr int kEmbedSlabDims = 256;                      // the widest slab: 64 lanes x 4 dimensions (one 16-byte load each)
constexpr int kEmbedMinSlabDims = 64;                    // the narrowest; the only one of the scalar-load path (64 lanes x 1)
constexpr int kEmbedNormChunk = 1024;                    // floats of a row staged per step of the normalise kernel
constexpr uint32_t kEmbedCus = 256;                      // compute units of an MI355X: what a small batch's slabs are cut to cover

enum EmbedMode : uint32_t { kEmbedCls = 0u, kEmbedMax = 1u, kEmbedMean = 2u };

// The predicate of the 16-byte row loads (row_vec4_loads), of the input and of the output a lane stores its four dimensions to:
// every row of both then starts on a 16-byte boundary.
inline bool embed_vec4(const float* hidden, const float* out, uint32_t dim) {
    return (dim & 3u) == 0 && ((reinterpret_cast<uintptr_t>(hidden) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
}
// The slab of dimensions one workgroup owns: the widest of 256 / 128 / 64 (16-byte loads; 64 with scalar loads) at which
// batch * slabs still gives every compute unit two workgroups, else the narrowest.
inline uint32_t embed_slab_dims(uint64_t batch, uint32_t dim, bool vec4) {
    if (!vec4) return kEmbedMinSlabDims;
    for (uint32_t slab = kEmbedSlabDims; slab > static_cast<uint32_t>(kEmbedMinSlabDims); slab >>= 1)
        if (batch * ((dim + slab - 1) / slab) >= 2ull * kEmbedCus) return slab;
    return kEmbedMinSlabDims;
}

// flags[0] |= 1: a considered mask value above 1 (looked for when `mean`); flags[1] += the considered values above 0.
// considered: mask[b][i], i < t_len.  batch * t_len >= 1.
hipError_t launch_embed_check(hipStream_t st, const int32_t* mask, uint64_t batch, uint32_t mask_len, uint32_t t_len, bool mean,
                              uint32_t* flags);
// out[b][:] = the pooled row of text b: CLS and MAX finished, MEAN the SUM over the active tokens with counts[b] = their number
// (the divide is launch_embed_finish's).  mask: null only when t_len == 0 or mode == kEmbedCls.  counts: [batch], needed for
// kEmbedMean only.  slab_dims: of embed_slab_dims.  batch >= 1.
hipError_t launch_embed_pool(hipStream_t st, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask,
                             uint32_t mask_len, uint32_t t_len, EmbedMode mode, uint32_t slab_dims, float* out, uint32_t* counts);
// out[b][:] = rows[b][:], divided by counts[b] where counts is given and counts[b] > 0 (a correctly rounded fp32 divide), then
// L2-normalised when asked.  out == rows is served.
hipError_t launch_embed_finish(hipStream_t st, const float* rows, uint64_t batch, uint32_t dim, const uint32_t* counts, bool normalize, float* out);

} // namespace yams_accel
