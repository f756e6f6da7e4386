// features_oracle — our C++ restatement of the array arithmetic of TopologyInputExtractor::extract (aggregateEmbedding,
// computeVarianceWeights, applyMatryoshkaCoarse, bucketCountSketch, composeFeatureVector), written from the contract in
// include/yams_mi355x_accel.h.  Built with -ffp-contract=off: the separate form's multiply and add stay two roundings, the
// fused form calls std::fma.  A shared library for ctypes (tests/_features_oracle.py), included by features_shell_test.cpp as
// the stand-in table's arithmetic, and the one-core figure scripts/features_bench.py sets the device's times beside.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

extern "C" {

// out [n_docs][dim], out_counts [n_docs]: the first record assigned, the later ones added, / float(count) when count > 1
void features_aggregate_oracle(const float* rows, uint32_t dim, const uint64_t* off, const uint32_t* records, uint64_t n_docs, float* out,
                               uint32_t* out_counts) {
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t lo = off[d], cnt = off[d + 1] - lo;
        float* o = out + d * dim;
        out_counts[d] = static_cast<uint32_t>(cnt);
        if (cnt == 0) { std::fill(o, o + dim, 0.0f); continue; }
        std::memcpy(o, rows + static_cast<uint64_t>(records[lo]) * dim, static_cast<size_t>(dim) * 4);
        for (uint64_t m = 1; m < cnt; ++m) {
            const float* r = rows + static_cast<uint64_t>(records[lo + m]) * dim;
            for (uint32_t i = 0; i < dim; ++i) o[i] += r[i];
        }
        if (cnt > 1)
            for (uint32_t i = 0; i < dim; ++i) o[i] /= static_cast<float>(cnt);
    }
}

// mean [dim], var [dim] over the rows select[0 .. m) (0 .. m-1 without select); m >= 1
void features_variance_oracle(const float* rows, uint32_t dim, const uint32_t* select, uint64_t m, int fused, double* mean, double* var) {
    std::fill(mean, mean + dim, 0.0);
    std::fill(var, var + dim, 0.0);
    for (uint64_t k = 0; k < m; ++k) {
        const float* e = rows + static_cast<uint64_t>(select ? select[k] : k) * dim;
        for (uint32_t i = 0; i < dim; ++i) mean[i] += static_cast<double>(e[i]);
    }
    for (uint32_t i = 0; i < dim; ++i) mean[i] /= static_cast<double>(m);
    for (uint64_t k = 0; k < m; ++k) {
        const float* e = rows + static_cast<uint64_t>(select ? select[k] : k) * dim;
        for (uint32_t i = 0; i < dim; ++i) {
            const double d = static_cast<double>(e[i]) - mean[i];
            if (fused) var[i] = std::fma(d, d, var[i]);
            else { const double p = d * d; var[i] = var[i] + p; }
        }
    }
    for (uint32_t i = 0; i < dim; ++i) var[i] /= static_cast<double>(m);
}

// weights [dim]: float(sqrt(var)) at the target dimensions of largest variance (this library's std::partial_sort), 0 elsewhere.
// Returns 0, or 1 when a variance is a NaN (the comparator is then no strict weak order: nothing is sorted or written).
int features_weights_oracle(const double* var, uint32_t dim, uint32_t target, float* weights) {
    for (uint32_t i = 0; i < dim; ++i)
        if (var[i] != var[i]) return 1;
    std::vector<size_t> idx(dim);
    std::iota(idx.begin(), idx.end(), size_t{0});
    std::partial_sort(idx.begin(), idx.begin() + static_cast<std::ptrdiff_t>(target), idx.end(),
                      [&](size_t a, size_t b) { return var[a] > var[b]; });
    std::fill(weights, weights + dim, 0.0f);
    for (uint32_t k = 0; k < target; ++k) weights[idx[k]] = static_cast<float>(std::sqrt(var[idx[k]]));
    return 0;
}

} // extern "C"

namespace features_oracle_detail {
inline void l2_normalize(float* v, size_t n) {
    double sumSq = 0.0;
    for (size_t i = 0; i < n; ++i) sumSq += static_cast<double>(v[i]) * static_cast<double>(v[i]);      // exact products
    if (sumSq <= 0.0) return;
    const float norm = static_cast<float>(std::sqrt(sumSq));
    for (size_t i = 0; i < n; ++i) v[i] /= norm;
}
} // namespace features_oracle_detail

extern "C" {

// out [n][out_stride] (zero-filled behind the row's length), out_dims [n].  Returns the longest possible row; writes nothing
// when out_stride is smaller.
uint32_t features_compose_oracle(const float* dense, uint64_t n, uint32_t dim, const float* weights, const float* entity, uint32_t k,
                                 const uint8_t* entity_on, const uint32_t* sig, uint32_t sig_len, const uint8_t* sketch_on,
                                 uint32_t sketch_dim, float alpha_e, float alpha_m, float* out, uint32_t out_stride, uint32_t* out_dims) {
    std::vector<uint32_t> kept;
    if (weights)
        for (uint32_t i = 0; i < dim; ++i)
            if (weights[i] > 0.0f) kept.push_back(i);
    const uint32_t kc = weights ? static_cast<uint32_t>(kept.size()) : dim;
    const bool has_e = entity && k, has_m = sig && sig_len && sketch_dim;
    const uint32_t longest = kc + (has_e ? k : 0u) + (has_m ? sketch_dim : 0u);
    if (out_stride < longest) return longest;
    std::vector<float> sketch(sketch_dim);
    for (uint64_t r = 0; r < n; ++r) {
        float* o = out + r * out_stride;
        std::fill(o, o + out_stride, 0.0f);
        const float* x = dense + r * dim;
        for (uint32_t j = 0; j < kc; ++j) o[j] = weights ? x[kept[j]] * weights[kept[j]] : x[j];
        features_oracle_detail::l2_normalize(o, kc);
        const bool e_on = has_e && entity_on[r], m_on = has_m && sketch_on[r];
        uint32_t len = kc;
        if (e_on || m_on) {
            const float aE = e_on ? alpha_e : 0.0f, aM = m_on ? alpha_m : 0.0f;
            const float t = (1.0f - aE) - aM;
            const float aD = (0.0f < t) ? t : 0.0f;
            for (uint32_t j = 0; j < kc; ++j) o[j] = o[j] * aD;
            if (e_on) {
                for (uint32_t j = 0; j < k; ++j) o[len + j] = entity[r * k + j] * aE;
                len += k;
            }
            if (m_on) {
                std::fill(sketch.begin(), sketch.end(), 0.0f);
                for (uint32_t i = 0; i < sig_len; ++i) sketch[sig[r * sig_len + i] % sketch_dim] += 1.0f;
                features_oracle_detail::l2_normalize(sketch.data(), sketch_dim);
                for (uint32_t j = 0; j < sketch_dim; ++j) o[len + j] = sketch[j] * aM;
                len += sketch_dim;
            }
        }
        out_dims[r] = len;
    }
    return longest;
}

} // extern "C"
