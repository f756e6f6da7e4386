// contract_rules.h — the result contract's small rules, ONE definition each.
//
// Every returned row, order and score bit equals the reference's; that rests on the rules below, each taken from the
// reference lines cited at its definition (paths relative to the reference checkout: src/vector/sqlite_vec_backend.cpp
// unless a file is named).  Kernels call these functions and keep a comment only for what is particular to the site;
// DESIGN.md §3.10 lists rule -> function -> reference lines -> call sites.
//
// Plain inline functions of scalars and pointers, for host and device: the header compiles with g++ -std=c++17 and no ROCm
// include path (tests/cpp/contract_rules_test.cpp holds each rule to the CPU oracle), and on the device every function is
// inlined into its kernel — fma stays fma, nothing becomes a call.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/yams_mi355x_accel.h"

#if defined(__HIPCC__)
#define YAMS_RULE __host__ __device__ inline __attribute__((always_inline))
#else
#define YAMS_RULE inline
#endif

namespace yams_accel {

// ---- order-preserving float <-> uint32 keys ----------------------------------------------------
// Larger key == better (larger) score.  NaN maps to the top key so that a row whose fp32 filter
// score is not trustworthy is always kept as a candidate (it is then scored exactly in fp64).
// Key 0 is never produced and marks an empty slot.
YAMS_RULE uint32_t f2ord(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu; // NaN
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
YAMS_RULE float ord2f(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
YAMS_RULE uint64_t pack_key(float score, uint32_t idx) {
    return (static_cast<uint64_t>(f2ord(score)) << 32) | static_cast<uint64_t>(0xffffffffu - idx);
}
// The reference orders cosine results with a FLOAT compare (:4218-4223, :4296-4298, :100-120): -0.0f == +0.0f there, the
// two zeros are ONE score and the tie rank decides between them — while f2ord puts every +0.0f above every -0.0f.  A
// cosine key therefore carries the canonical zero; the score a caller is GIVEN keeps its own sign bit (the reference
// returns -0.0f where the fp64 quotient underflows from below), which a selection either keeps beside the key or recovers
// by scoring the winner again (exact_cosine_again).  L2 keys (-distance: always -0.0f at distance zero) have one zero only.
YAMS_RULE uint64_t pack_cosine_key(float sim, uint32_t idx) {
    return pack_key(sim == 0.0f ? 0.0f : sim, idx);
}
YAMS_RULE uint32_t key_idx(uint64_t k) {
    return 0xffffffffu - static_cast<uint32_t>(k);
}
YAMS_RULE float key_score(uint64_t k) {
    return ord2f(static_cast<uint32_t>(k >> 32));
}

// ---- the sums ----------------------------------------------------------------------------------
// One sequential fp64 chain per sum, element by element (:4253-4266; vector_database.cpp:1796-1800).  A product of two
// floats is exact in fp64, so fma == multiply then add.  For the sites whose loop is this and nothing else; the staged
// and vectorised walks of the kernels feed the same chains from LDS or registers.
YAMS_RULE void row_sums(const float* x, const float* q, uint32_t dim, double* nsq, double* dot) {
    double n = 0.0, d = 0.0;
    for (uint32_t i = 0; i < dim; ++i) {
        const double sv = static_cast<double>(x[i]);
        n = std::fma(sv, sv, n);
        d = std::fma(sv, static_cast<double>(q[i]), d);
    }
    *nsq = n;
    *dot = d;
}

// ---- query validity (:4127-4130) ---------------------------------------------------------------
// nsq = the query's fp64 sum of squares.  bit 0: a non-finite element (isFiniteEmbedding :229-236 — fp64 cannot
// overflow on fp32 squares, so "every element finite" <=> "the sum is finite"); bit 1: isZeroNormEmbedding, norm^2 <
// 1e-10 (:204-211).
YAMS_RULE uint32_t query_flags(double nsq) {
    uint32_t f = 0;
    if (!std::isfinite(nsq)) f |= 1u;
    if (!(nsq >= 1e-10)) f |= 2u;
    return f;
}

// ---- the fast path's cosine (:4258-4279) -------------------------------------------------------
// Which rows get a score: every element finite (<=> nsq finite) and norm^2 > 1e-12 (:4267-4269); the record path drops
// norm^2 < 1e-10 instead (isZeroNormEmbedding :204-211, :4365-4367).
YAMS_RULE bool fast_row_scored(double nsq, bool record_path) {
    return std::isfinite(nsq) && (record_path ? nsq >= 1e-10 : nsq > 1e-12);
}
// The quotient (:4271-4272) into *sd; false when it is not finite and the row is dropped (:4273-4275).
YAMS_RULE bool fast_quotient(double dot, double nsq, double qn, double* sd) {
    const double denom = std::sqrt(nsq) * qn;
    *sd = denom > 0.0 ? dot / denom : 0.0;
    return std::isfinite(*sd);
}
YAMS_RULE float fast_cast(double sd) { return static_cast<float>(sd); } // :4276
// :4277-4279: dropped iff sim < threshold — a NaN threshold keeps every row.
YAMS_RULE bool fast_kept(float sim, float threshold) { return !(sim < threshold); }
// The whole rule: the key of a row (the canonical zero: pack_cosine_key), 0 when the row is dropped.
YAMS_RULE uint64_t fast_cosine_key(double dot, double nsq, double qn, bool record_path, float threshold, uint32_t rank) {
    double sd;
    if (!fast_row_scored(nsq, record_path) || !fast_quotient(dot, nsq, qn, &sd)) return 0;
    const float sim = fast_cast(sd);
    return fast_kept(sim, threshold) ? pack_cosine_key(sim, rank) : 0;
}
// The score of one row again, for a winner whose key says "zero": only the sign of the zero is news, the row is known to
// be valid.
YAMS_RULE float exact_cosine_again(const float* x, const float* q, uint32_t dim, double qn) {
    double nsq, dot, sd;
    row_sums(x, q, dim, &nsq, &dot);
    fast_quotient(dot, nsq, qn, &sd);
    return fast_cast(sd);
}

// ---- VectorDatabase::computeCosineSimilarity (vector_database.cpp:1786-1810) ----------------------
// nsq_row = the row's sum of squares, qn = sqrt of the query's: each norm's own square root, 0 when either is zero —
// tested BEFORE the division — no finiteness test, no small-norm rule; the cast of the callers (:2859, :4023-4034,
// :4373-4374).  Each caller keeps its own admission rule around it.
YAMS_RULE float compute_cosine_similarity(double dot, double nsq_row, double qn) {
    const double rn = std::sqrt(nsq_row);
    return static_cast<float>((qn == 0.0 || rn == 0.0) ? 0.0 : dot / (qn * rn));
}

// ---- the semantic-neighbour graph (src/daemon/components/EmbeddingService.cpp) -------------------------------------
// inverseNorm (:405-415) from the row's fp64 sum of squares: 0 for a zero row, else the fp64 quotient rounded to FLOAT.
YAMS_RULE float graph_inverse_norm(double nsq) {
    return nsq <= 0.0 ? 0.0f : static_cast<float>(1.0 / std::sqrt(nsq));
}
// cosineSimilarity's tail (:430): (dot * invSource) * invNeighbour in fp64, in THAT order, then the cast.
YAMS_RULE float graph_similarity(double dot, float inv_source, float inv_neighbour) {
    return static_cast<float>((dot * static_cast<double>(inv_source)) * static_cast<double>(inv_neighbour));
}
// Admission (:626-632, :991-997): an explicit threshold drops sim < threshold; without one, sim <= 0 (both zeros) goes.
YAMS_RULE bool graph_admits(float sim, bool explicit_threshold, float threshold) {
    return explicit_threshold ? !(sim < threshold) : !(sim <= 0.0f);
}

// ---- the allow-mask: bit (row & 31) of word row / 32 (yams_scan_corpus_t.row_mask, non-null here) -----------------
YAMS_RULE bool row_allowed(const uint32_t* row_mask, uint64_t row) {
    return (row_mask[row >> 5] >> (row & 31)) & 1u;
}

// ---- local row ordinal -> the id the caller sees (yams_scan_corpus_t: row_base, stripes; stripe_rows 0 = contiguous) ----
YAMS_RULE int64_t global_row_id(int64_t row_base, uint32_t stripe_rows, uint32_t n_stripes, uint32_t stripe_index, uint32_t row) {
    if (stripe_rows == 0) return row_base + static_cast<int64_t>(row);
    const uint64_t t = row / stripe_rows, w = row % stripe_rows;
    return row_base + static_cast<int64_t>((t * n_stripes + stripe_index) * stripe_rows + w);
}

// ---- an unused result slot: score -inf, row -1, distance +inf, rank 0xffffffff, document YAMS_SCAN_NO_DOC ------------
// (the three tails are nullable: an entry point writes the ones it has)
YAMS_RULE void write_empty_slot(uint64_t o, float* out_scores, int64_t* out_rows, float* out_dist, uint32_t* out_ranks,
                                uint32_t* out_docs) {
    out_scores[o] = -__builtin_inff();
    out_rows[o] = -1;
    if (out_dist) out_dist[o] = __builtin_inff();
    if (out_ranks) out_ranks[o] = 0xffffffffu;
    if (out_docs) out_docs[o] = YAMS_SCAN_NO_DOC;
}

// ---- the entity predicate (searchEntities' WHERE, :2821-2829) ---------------------------------------------------
// Three optional column equalities.  The "unset" value of a column equals no filter value; a null column behind a named
// field never gets here (the host refuses the call).
YAMS_RULE bool entity_admits(const yams_scan_entity_filter_t& f, const uint8_t* row_type, const uint32_t* row_node_type,
                             const uint32_t* row_doc, uint64_t row) {
    if ((f.fields & YAMS_SCAN_ENTITY_FILTER_TYPE) && !(f.embedding_type < YAMS_SCAN_ENTITY_TYPE_UNSET && row_type[row] == f.embedding_type)) return false;
    if ((f.fields & YAMS_SCAN_ENTITY_FILTER_NODE_TYPE) && !(f.node_type != YAMS_SCAN_ENTITY_UNSET && row_node_type[row] == f.node_type)) return false;
    if ((f.fields & YAMS_SCAN_ENTITY_FILTER_DOC) && !(f.doc != YAMS_SCAN_ENTITY_UNSET && row_doc[row] == f.doc)) return false;
    return true;
}

} // namespace yams_accel
