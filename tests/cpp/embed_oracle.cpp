// embed_oracle.cpp — OUR C++ restatement of the embedding model's pooling head (CLS, max or mean over the tokens of each text,
// then the L2 normalisation), written from the contract in include/yams_mi355x_accel.h.  Built with -ffp-contract=off: the MEAN
// step is a rounded multiply then a rounded add (with masks of 0 and 1 the product is exact and the forms agree).  A shared
// library for ctypes, and included by embed_shell_test.cpp as the stand-in table's arithmetic and the shell's host loop.
#include <algorithm>
#include <cmath>
#include <cstdint>

extern "C" {

// in place: the fp64 chain of squares in element order, sqrt, v / norm or zeros
void embed_oracle_normalize_row(float* v, uint32_t dim) {
    double norm = 0.0;
    for (uint32_t d = 0; d < dim; ++d) norm += static_cast<double>(v[d]) * static_cast<double>(v[d]);
    norm = std::sqrt(norm);
    for (uint32_t d = 0; d < dim; ++d) v[d] = norm > 1e-8 ? static_cast<float>(static_cast<double>(v[d]) / norm) : 0.0f;
}

// mode: 0 CLS, 1 MAX, 2 MEAN.  mask: nullable (then mask_len counts as 0).  order: nullable; a permutation of the token
// indices [seq] in which the tokens are visited (the discriminating checks of the tests: reversed, pairwise is separate).
// counts: nullable, [2] = tokens considered, active tokens (both 0 for CLS).  Weights above 1 are served as the reference
// serves them: w = float(mask).
void embed_oracle_pool(const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask, uint32_t mask_len,
                       uint32_t mode, uint32_t normalize, const uint32_t* order, float* out, uint64_t* counts) {
    const uint32_t t_len = mask ? std::min(seq, mask_len) : 0u;
    uint64_t considered = 0, active = 0;
    for (uint64_t b = 0; b < batch; ++b) {
        float* emb = out + b * dim;
        for (uint32_t d = 0; d < dim; ++d) emb[d] = 0.0f;
        const float* data = hidden + b * seq * dim;
        if (mode == 0u) {
            for (uint32_t d = 0; d < dim; ++d) emb[d] = data[d];
        } else {
            float total = 0.0f;
            for (uint32_t k = 0; k < seq; ++k) {
                const uint32_t i = order ? order[k] : k;
                if (i >= t_len) continue;
                const int32_t mv = mask[b * mask_len + i];
                ++considered;
                if (mv > 0) ++active;
                const float* x = data + static_cast<uint64_t>(i) * dim;
                if (mode == 1u) {
                    if (mv <= 0) continue;
                    for (uint32_t d = 0; d < dim; ++d) emb[d] = emb[d] < x[d] ? x[d] : emb[d];
                } else {
                    const float w = static_cast<float>(mv);
                    if (w <= 0.0f) continue;
                    total = total + w;
                    for (uint32_t d = 0; d < dim; ++d) {
                        const float p = x[d] * w;
                        emb[d] = emb[d] + p;
                    }
                }
            }
            if (mode == 2u && total > 0.0f)
                for (uint32_t d = 0; d < dim; ++d) emb[d] = emb[d] / total;
        }
        if (normalize) embed_oracle_normalize_row(emb, dim);
    }
    if (counts) { counts[0] = considered; counts[1] = active; }
}

void embed_oracle_normalize(const float* rows, uint64_t batch, uint32_t dim, float* out) {
    for (uint64_t b = 0; b < batch; ++b) {
        for (uint32_t d = 0; d < dim; ++d) out[b * dim + d] = rows[b * dim + d];
        embed_oracle_normalize_row(out + b * dim, dim);
    }
}

} // extern "C"
