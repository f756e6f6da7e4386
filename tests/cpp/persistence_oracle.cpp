// persistence_oracle.cpp — a restatement of computePersistenceH0 (the contract in include/yams_mi355x_accel.h) in plain C++,
// for the cases a pure-Python exact fma is too slow for.  Built by tests/_persistence_build.py as a shared library with
// -ffp-contract=off, so that `acc + d * d` is a rounded multiply and a rounded add; the fused form spells std::fma out.
// It does the real Kruskal over stably sorted edges (nothing about minimum spanning trees is assumed), goes on to the last
// merge so that all m - 1 weights are returned, and sums the first m - 2 quotients.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace {

struct Edge { std::uint32_t i, j; double distance; };

std::size_t find_root(std::vector<std::size_t>& parent, std::size_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
}

double chain(const float* a, const float* b, std::uint32_t dim, int fused) {
    double acc = 0.0;
    if (fused) {
        for (std::uint32_t k = 0; k < dim; ++k) {
            const double d = static_cast<double>(a[k]) - static_cast<double>(b[k]);
            acc = std::fma(d, d, acc);
        }
    } else {
        for (std::uint32_t k = 0; k < dim; ++k) {
            const double d = static_cast<double>(a[k]) - static_cast<double>(b[k]);
            const double p = d * d;
            acc = acc + p;
        }
    }
    return std::sqrt(acc);
}

} // namespace

// points [m][dim]; out_dist nullable [m][m]; out_weights nullable [m - 1] (Kruskal's merges, ascending); the rest required.
// Returns the number of merges summed into *out_value.
extern "C" std::uint64_t persistence_oracle(const float* points, std::uint64_t m, std::uint32_t dim, int fused, double* out_dist,
                                            double* out_weights, double* out_norm, std::uint64_t* out_index, double* out_value) {
    *out_norm = 0.0; *out_index = 0; *out_value = 0.0;
    if (out_dist)
        for (std::uint64_t i = 0; i < m; ++i) out_dist[i * m + i] = 0.0;
    if (m < 2 || dim == 0) return 0;
    const std::size_t edge_count = m * (m - 1) / 2;
    std::vector<Edge> edges;
    edges.reserve(edge_count);
    std::vector<double> all;
    all.reserve(edge_count);
    for (std::uint64_t i = 0; i < m; ++i)
        for (std::uint64_t j = i + 1; j < m; ++j) {
            const double d = chain(points + i * dim, points + j * dim, dim, fused);
            edges.push_back(Edge{static_cast<std::uint32_t>(i), static_cast<std::uint32_t>(j), d});
            all.push_back(d);
            if (out_dist) { out_dist[i * m + j] = d; out_dist[j * m + i] = d; }
        }
    std::stable_sort(edges.begin(), edges.end(), [](const Edge& a, const Edge& b) { return a.distance < b.distance; });
    const std::size_t idx = static_cast<std::size_t>(std::clamp(0.95 * static_cast<double>(all.size() - 1), 0.0, static_cast<double>(all.size() - 1)));
    std::nth_element(all.begin(), all.begin() + static_cast<std::ptrdiff_t>(idx), all.end());
    const double norm = all[idx];
    *out_norm = norm;
    *out_index = idx;
    std::vector<std::size_t> parent(m), rank(m, 0);
    std::iota(parent.begin(), parent.end(), std::size_t{0});
    double total = 0.0;
    std::uint64_t merges = 0, summed = 0;
    for (const Edge& e : edges) {
        if (merges + 1 >= m) break;
        std::size_t ra = find_root(parent, e.i), rb = find_root(parent, e.j);
        if (ra == rb) continue;
        if (rank[ra] < rank[rb]) std::swap(ra, rb);
        parent[rb] = ra;
        if (rank[ra] == rank[rb]) ++rank[ra];
        if (out_weights) out_weights[merges] = e.distance;
        if (merges + 2 < m && norm > 0.0) { total += e.distance / norm; ++summed; }
        ++merges;
    }
    *out_value = norm > 0.0 ? total : 0.0;
    return summed;
}
