// rerank_oracle.cpp — OUR C++ restatement of the late-interaction rerank: computeMaxSim over a window of documents and
// maxPoolEmbeddings + normalizeEmbedding, written from the contract in include/yams_mi355x_accel.h.  Built with
// -ffp-contract=off: form 0 is a rounded multiply then a rounded add, form 1 calls std::fmaf.  A shared library for ctypes, and
// included by rerank_shell_test.cpp as the stand-in table's arithmetic.
#include <cmath>
#include <cstdint>
#include <limits>

extern "C" {

// sim(q, d): one chain from +0.0f in element order
float rerank_oracle_dot(const float* a, const float* b, uint32_t dim, uint32_t form) {
    float sum = 0.0f;
    if (form == 1u) {
        for (uint32_t i = 0; i < dim; ++i) sum = std::fmaf(a[i], b[i], sum);
    } else {
        for (uint32_t i = 0; i < dim; ++i) {
            const float p = a[i] * b[i];
            sum = sum + p;
        }
    }
    return sum;
}

// out_rowmax / out_rowarg: nullable, [n_docs][tq]; rowarg = the token that stayed, 0xffffffff where none did
void rerank_oracle_maxsim(const float* query, uint32_t tq, uint32_t dim, const float* rows, const uint64_t* off, uint64_t n_docs,
                          uint32_t form, float* out_scores, float* out_rowmax, uint32_t* out_rowarg) {
    for (uint64_t doc = 0; doc < n_docs; ++doc) {
        float score = 0.0f;
        for (uint32_t q = 0; q < tq; ++q) {
            float maxSim = -std::numeric_limits<float>::infinity();
            uint32_t arg = 0xffffffffu;
            for (uint64_t r = off[doc]; r < off[doc + 1]; ++r) {
                const float sim = rerank_oracle_dot(query + static_cast<uint64_t>(q) * dim, rows + r * dim, dim, form);
                if (sim > maxSim) {
                    maxSim = sim;
                    arg = static_cast<uint32_t>(r - off[doc]);
                }
            }
            score = score + maxSim;
            if (out_rowmax) out_rowmax[doc * tq + q] = maxSim;
            if (out_rowarg) out_rowarg[doc * tq + q] = arg;
        }
        out_scores[doc] = score;
    }
}

void rerank_oracle_maxpool(const float* rows, uint32_t dim, const uint64_t* off, uint64_t n_docs, float* out) {
    for (uint64_t doc = 0; doc < n_docs; ++doc) {
        float* p = out + doc * dim;
        for (uint32_t i = 0; i < dim; ++i) {
            float v = -std::numeric_limits<float>::infinity();
            for (uint64_t r = off[doc]; r < off[doc + 1]; ++r) {
                const float x = rows[r * dim + i];
                if (v < x) v = x;
            }
            if (!std::isfinite(v)) v = 0.0f;
            p[i] = v;
        }
        double norm = 0.0;
        for (uint32_t i = 0; i < dim; ++i) norm += static_cast<double>(p[i]) * static_cast<double>(p[i]);
        norm = std::sqrt(norm);
        for (uint32_t i = 0; i < dim; ++i) p[i] = norm > 1e-8 ? static_cast<float>(static_cast<double>(p[i]) / norm) : 0.0f;
    }
}

} // extern "C"
