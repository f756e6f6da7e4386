// rerank_launch.h — what rerank_kernels.hip and rerank_api.cpp share: the launchers of the late-interaction rerank (ColBERT
// MaxSim) and of the token pooling (max-pool + L2 normalisation).
#pragma once
#include "common.h"

namespace yams_accel {

constexpr uint32_t kRerankMaxDim = 1024u;                // YAMS_RERANK_MAX_DIM
constexpr uint32_t kRerankMaxDocTokens = 1u << 20;       // YAMS_RERANK_MAX_DOC_TOKENS: tokens of one document
constexpr uint32_t kRerankMaxQueryTokens = 1u << 16;     // YAMS_RERANK_MAX_QUERY_TOKENS
constexpr uint64_t kRerankMaxRows = 1ull << 28;          // YAMS_RERANK_MAX_ROWS: the row pool of one call
constexpr uint64_t kRerankMaxDocs = 1ull << 20;          // YAMS_RERANK_MAX_DOCS
constexpr uint64_t kRerankMaxRowMax = 1ull << 27;        // YAMS_RERANK_MAX_ROWMAX: n_docs * Tq, the row maxima of one call
constexpr int kRerankThreads = 256;
constexpr int kRerankQTile = 32;                         // query tokens per workgroup
constexpr int kRerankDTile = 256;                        // document tokens per pass of a workgroup
constexpr int kRerankKChunk = 32;                        // dimensions staged per pass
constexpr uint32_t kRerankNone = 0xffffffffu;            // no document token won (the row maximum is the initial -inf)

enum RerankPath : uint32_t { kRerankValu = 0u, kRerankMfma = 1u };
// Which path serves the fused form in the product.
constexpr RerankPath kRerankFusedPath = kRerankMfma;

// flags |= 1: offsets that do not start at 0, decrease or do not end at `total`; |= 2: a document longer than max_len.
hipError_t launch_rerank_check(hipStream_t st, const uint64_t* off, uint64_t n_docs, uint64_t total, uint32_t max_len, uint32_t* flags);
// rowmax[doc][q] = the row maximum of query token q over the document's tokens (-inf where none won); rowarg, nullable,
// [doc][q] = the winning token's index inside the document (kRerankNone where none won).  fused: fmaf chains, else multiply
// then add.  path: kRerankMfma only with fused.  tq, n_docs >= 1.
hipError_t launch_rerank_rowmax(hipStream_t st, const float* query, uint32_t tq, uint32_t dim, const float* rows, const uint64_t* off,
                                uint32_t n_docs, bool fused, RerankPath path, float* rowmax, uint32_t* rowarg);
// scores[doc] = the fp32 chain 0.0f + rowmax[doc][0] + rowmax[doc][1] + ... in query order, one lane per document.
hipError_t launch_rerank_score(hipStream_t st, const float* rowmax, uint32_t tq, uint32_t n_docs, float* scores);
// out[doc][:] = the max-pooled, L2-normalised token matrix of every document.
hipError_t launch_rerank_maxpool(hipStream_t st, const float* rows, uint32_t dim, const uint64_t* off, uint32_t n_docs, float* out);

} // namespace yams_accel
