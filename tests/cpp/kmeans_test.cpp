// kmeans_test.cpp — AccelKMeans (include/yams_accel/topology_kmeans.hpp) against a host loop: this file's own scalar
// restatement of the contract in include/yams_mi355x_accel.h (fp64 chains in element order, fp32 means in row order).
//   kmeans_test <plugin.so> [--expect-no-gpu]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "yams_accel/topology_kmeans.hpp"

using namespace yams;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::printf("CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

namespace host {
using Vec = std::vector<float>;

double sumsq(const Vec& a) { double s = 0; for (float x : a) s += double(x) * double(x); return s; }

double dist(const Vec& a, const Vec& b) {
    double dot = 0;
    for (size_t i = 0; i < a.size(); ++i) dot += double(a[i]) * double(b[i]);
    const double na = sumsq(a), nb = sumsq(b);
    if (na <= 0 || nb <= 0) return 2.0;
    const double c = dot / (std::sqrt(na) * std::sqrt(nb));
    return 1.0 - (c < -1.0 ? -1.0 : (1.0 < c ? 1.0 : c));
}

Vec unit(Vec v) {
    const double n = sumsq(v);
    if (n > 0) { const float inv = float(1.0 / std::sqrt(n)); for (auto& x : v) x *= inv; }
    return v;
}

Vec centre(const std::vector<Vec>& rows, const std::vector<size_t>& members) {
    Vec s(rows[0].size(), 0.0f);
    for (size_t u : members) for (size_t d = 0; d < s.size(); ++d) s[d] += rows[u][d];
    for (auto& x : s) x /= float(members.size());
    return unit(s);
}

// the clustering of the usable rows; returns k
size_t cluster(const std::vector<Vec>& rows, size_t k, size_t iters, std::vector<size_t>& member) {
    const size_t n = rows.size();
    if (k == 0) k = size_t(std::round(std::sqrt(double(n))));
    k = std::min(std::max<size_t>(k, 2), n);
    std::vector<Vec> cent{unit(rows[0])};
    std::vector<char> taken(n, 0); taken[0] = 1;
    std::vector<double> md(n, std::numeric_limits<double>::max());
    while (cent.size() < k) {
        size_t far = n; double fd = -1.0;
        for (size_t u = 0; u < n; ++u) {
            if (taken[u]) continue;
            md[u] = std::min(md[u], dist(rows[u], cent.back()));      // (std::min keeps md on a NaN)
            if (md[u] > fd) { fd = md[u]; far = u; }
        }
        if (far == n) break;
        taken[far] = 1; cent.push_back(unit(rows[far]));
    }
    k = cent.size();
    member.assign(n, 0);
    for (size_t it = 0; it < (iters ? iters : 10); ++it) {
        bool changed = false;
        for (size_t u = 0; u < n; ++u) {
            size_t best = 0; double bd = std::numeric_limits<double>::max();
            for (size_t c = 0; c < k; ++c) { const double d = dist(rows[u], cent[c]); if (d < bd) { bd = d; best = c; } }
            if (best != member[u]) { member[u] = best; changed = true; }
        }
        std::vector<std::vector<size_t>> lists(k);
        for (size_t u = 0; u < n; ++u) lists[member[u]].push_back(u);
        for (size_t c = 0; c < k; ++c) if (!lists[c].empty()) cent[c] = centre(rows, lists[c]);
        for (size_t c = 0; c < k; ++c) {
            if (!lists[c].empty()) continue;
            size_t worst = n, donor = k; double wd = -1.0;
            for (size_t u = 0; u < n; ++u) {
                if (lists[member[u]].size() <= 1) continue;
                const double d = dist(rows[u], cent[member[u]]);
                if (d > wd) { wd = d; worst = u; donor = member[u]; }
            }
            if (worst == n) continue;
            auto& dl = lists[donor];
            dl.erase(std::find(dl.begin(), dl.end(), worst));
            member[worst] = c; lists[c].push_back(worst);
            cent[c] = unit(rows[worst]); cent[donor] = centre(rows, dl);
            changed = true;
        }
        if (!changed) break;
    }
    return k;
}

std::vector<int64_t> run(const std::vector<Vec>& emb, size_t k, size_t iters) {
    std::vector<int64_t> out(emb.size(), -1);
    std::vector<size_t> usable; size_t dim = 0;
    for (size_t i = 0; i < emb.size(); ++i) {
        if (emb[i].empty()) continue;
        if (!dim) dim = emb[i].size();
        if (emb[i].size() == dim) usable.push_back(i);
    }
    if (usable.size() < 2) { for (size_t i = 0; i < out.size(); ++i) out[i] = int64_t(i); return out; }
    std::vector<Vec> rows; for (size_t u : usable) rows.push_back(emb[u]);
    std::vector<size_t> member;
    int64_t next = int64_t(cluster(rows, k, iters, member));
    for (size_t u = 0; u < usable.size(); ++u) out[usable[u]] = int64_t(member[u]);
    for (auto& a : out) if (a < 0) a = next++;
    return out;
}
} // namespace host

static void compare(const topology::AccelKMeans& km, const std::vector<host::Vec>& emb, size_t k, size_t iters, const char* what) {
    auto got = km.run(emb, k, iters);
    CHECK(got.has_value());
    if (!got.has_value()) { std::printf("  %s: %s\n", what, got.error().message.c_str()); return; }
    const auto want = host::run(emb, k, iters);
    const bool same = got.value() == want;
    CHECK(same);
    if (!same) std::printf("  %s: assignment differs from the host loop\n", what);
}

int main(int argc, char** argv) {
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    if (argc < 2) { std::printf("usage: %s <plugin.so> [--expect-no-gpu]\n", argv[0]); return 2; }
    const bool expectNoGpu = argc > 2 && std::strcmp(argv[2], "--expect-no-gpu") == 0;
    auto loaded = accel::Plugin::load(argv[1], "{\"device\":0}");
    if (expectNoGpu) {   // no device: the plugin refuses to initialise, nothing falls back
        CHECK(!loaded.has_value());
        if (!loaded.has_value()) CHECK(loaded.error().code == ErrorCode::NotInitialized);
        std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
        return failures ? 1 : 0;
    }
    if (!loaded.has_value()) { std::printf("plugin load failed: %s\n", loaded.error().message.c_str()); return 1; }
    auto made = topology::AccelKMeans::create(loaded.value());
    if (!made.has_value()) { std::printf("no topology_cluster_v1: %s\n", made.error().message.c_str()); return 1; }
    const topology::AccelKMeans& km = *made.value();

    std::mt19937 rng(5);
    std::normal_distribution<float> nd(0.f, 1.f);
    auto rows = [&](size_t n, size_t dim, size_t groups) {
        std::vector<host::Vec> c(groups, host::Vec(dim)), out(n, host::Vec(dim));
        for (auto& v : c) for (auto& x : v) x = nd(rng);
        for (size_t i = 0; i < n; ++i) for (size_t d = 0; d < dim; ++d) out[i][d] = c[i % groups][d] + 0.3f * nd(rng);
        return out;
    };
    compare(km, {}, 0, 0, "no documents");
    compare(km, rows(600, 48, 12), 0, 0, "600 x 48, default");
    compare(km, rows(400, 33, 8), 9, 0, "400 x 33, k = 9");
    compare(km, rows(400, 64, 8), 0, 1, "400 x 64, one iteration");
    {   // ragged: an empty row first, rows of other dimensions, duplicates and zero rows among the usable ones
        auto e = rows(150, 20, 5);
        e[0].clear(); e[17] = host::Vec(19, 1.0f); e[60] = host::Vec(21, 1.0f); e[149].clear();
        for (size_t i = 30; i < 60; ++i) e[i] = e[i % 4 + 1];
        std::fill(e[100].begin(), e[100].end(), 0.0f); std::fill(e[101].begin(), e[101].end(), 0.0f);
        compare(km, e, 25, 0, "ragged with duplicates, k = 25");
        compare(km, e, 0, 3, "ragged with duplicates, three iterations");
    }
    compare(km, {host::Vec{}, host::Vec{1.f, 2.f}, host::Vec{1.f}}, 0, 0, "one usable row");
    compare(km, {host::Vec{1.f, 2.f}, host::Vec{-1.f, 0.5f}}, 0, 0, "two rows");
    compare(km, rows(9, 4, 3), 40, 0, "k above n");
    {   // a non-finite row is refused, not served
        auto e = rows(20, 8, 2);
        e[3][2] = std::numeric_limits<float>::infinity();
        auto got = km.run(e, 0, 0);
        CHECK(!got.has_value());
        if (!got.has_value()) CHECK(got.error().code == ErrorCode::InvalidArgument);
    }
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
