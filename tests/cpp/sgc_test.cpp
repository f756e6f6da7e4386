// sgc_test.cpp — AccelSGC (include/yams_accel/topology_sgc.hpp), the shell of applySGCSmoothing.
//
//   sgc_test                  the shell over a stand-in table (a scalar CPU loop written from the contract in
//                             yams_mi355x_accel.h): early returns, write-back of the rows of the right size only, a refusal
//                             leaves the documents untouched, the lists are symmetric and hold no self-loop
//   sgc_test --plugin <lib>   the same documents through the real plugin: its result must equal the stand-in's bit for bit
//   -DSGC_WITH_REFERENCE      (built with -DYAMS_ACCEL_USE_HOST_TYPES and linked with the reference's own topology_sgc.cpp)
//                             the shell's result must equal applySGCSmoothing bit for bit on seeded cases: this holds the
//                             claim that the shell's lists come out in the reference's order to the reference itself
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifdef SGC_WITH_REFERENCE
#include <yams/topology/topology_sgc.h>
#endif
#include <yams_accel/topology_sgc.hpp>

using namespace yams::topology;

namespace {

int g_failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++g_failures; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

bool g_refuse = false;
int g_calls = 0;

// The contract's loop, one element at a time.
yams_status_t stand_in_smooth(void*, const float* rows, uint64_t n, uint32_t dim, const uint64_t* off, const uint32_t* cols, const float* w,
                              uint32_t hops, float* out, yams_sgc_diag_t* diag) {
    ++g_calls;
    if (g_refuse) return YAMS_ERR_UNSUPPORTED;
    std::vector<double> inv(n);
    for (uint64_t i = 0; i < n; ++i) {
        double deg = 1.0;
        for (uint64_t e = off[i]; e < off[i + 1]; ++e) deg += static_cast<double>(w[e]);
        inv[i] = deg > 0.0 ? 1.0 / std::sqrt(deg) : 0.0;
    }
    std::vector<float> cur(rows, rows + n * dim), next(n * dim);
    uint64_t skipped = 0;
    for (uint32_t h = 0; h < hops; ++h) {
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t d = 0; d < dim; ++d) {
                float acc = static_cast<float>((inv[i] * inv[i]) * static_cast<double>(cur[i * dim + d]));
                for (uint64_t e = off[i]; e < off[i + 1]; ++e) {
                    const double scale = (static_cast<double>(w[e]) * inv[i]) * inv[cols[e]];
                    if (scale == 0.0) { skipped += h == 0 && d == 0; continue; }
                    acc = acc + static_cast<float>(scale * static_cast<double>(cur[static_cast<uint64_t>(cols[e]) * dim + d]));
                }
                next[i * dim + d] = acc;
            }
        cur.swap(next);
    }
    std::memcpy(out, cur.data(), n * dim * sizeof(float));
    if (diag) { *diag = yams_sgc_diag_t{}; diag->nnz = off[n]; diag->hops = hops; diag->edges_skipped_zero_scale = skipped; }
    return YAMS_OK;
}

yams_topology_smooth_v1 g_stand_in = {YAMS_IFACE_TOPOLOGY_SMOOTH_V1_VERSION, nullptr, &stand_in_smooth};

struct Rng {      // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double unit() { return static_cast<double>(next() >> 11) / 9007199254740992.0; }
};

std::vector<TopologyDocumentInput> seeded(uint64_t seed, std::size_t n, std::size_t dim, std::size_t k) {
    Rng r{seed};
    std::vector<TopologyDocumentInput> docs(n);
    for (std::size_t i = 0; i < n; ++i) {
        docs[i].documentHash = "h" + std::to_string(i);
        std::size_t m = dim;
        const double p = r.unit();
        if (i > 0 && p < 0.02) m = 0; else if (i > 0 && p < 0.04) m = dim + 1;      // ragged rows
        docs[i].embedding.resize(m);
        for (auto& v : docs[i].embedding) v = static_cast<float>(r.unit() * 4.0 - 2.0);
        if (m && r.unit() < 0.1) docs[i].embedding[0] = -0.0f;
        for (std::size_t j = 0; j < k; ++j) {
            TopologyNeighbor nb;
            nb.documentHash = r.unit() < 0.02 ? std::string("missing") : "h" + std::to_string(r.next() % n);
            nb.score = static_cast<float>(r.unit() * 1.2 - 0.1);
            nb.reciprocal = r.unit() < 0.85;
            docs[i].neighbors.push_back(nb);
        }
    }
    docs[n / 2].documentHash = docs[n / 3].documentHash;      // a duplicate hash: the later document takes the edges
    docs[n / 4].documentHash.clear();
    return docs;
}

bool same_bits(const std::vector<TopologyDocumentInput>& a, const std::vector<TopologyDocumentInput>& b, std::size_t* differing) {
    *differing = 0;
    if (a.size() != b.size()) return false;
    for (std::size_t i = 0; i < a.size(); ++i) {
        if (a[i].embedding.size() != b[i].embedding.size()) return false;
        for (std::size_t d = 0; d < a[i].embedding.size(); ++d)
            *differing += std::memcmp(&a[i].embedding[d], &b[i].embedding[d], 4) != 0;
    }
    return *differing == 0;
}

void shell_properties() {
    auto sgc = AccelSGC::over(&g_stand_in);
    TopologyBuildConfig cfg;
    cfg.reciprocalOnly = true;
    // early returns: no call is made and nothing changes
    auto docs = seeded(1, 40, 5, 4);
    docs[5].embedding.assign(6, 1.5f);      // ragged: another size, and none
    docs[6].embedding.clear();
    const auto before = docs;
    std::size_t diff;
    g_calls = 0;
    EXPECT(sgc->apply(docs, cfg, 0).has_value() && g_calls == 0 && same_bits(docs, before, &diff));
    std::vector<TopologyDocumentInput> one(docs.begin(), docs.begin() + 1);
    EXPECT(sgc->apply(one, cfg, 2).has_value() && g_calls == 0);
    std::vector<TopologyDocumentInput> empty(3);
    EXPECT(sgc->apply(empty, cfg, 2).has_value() && g_calls == 0);
    // a refusal: an Error, documents untouched
    g_refuse = true;
    auto r = sgc->apply(docs, cfg, 2);
    EXPECT(!r.has_value() && r.error().code == yams::ErrorCode::NotImplemented && same_bits(docs, before, &diff));
    g_refuse = false;
    // served: rows of another size are not written, the others change
    EXPECT(sgc->apply(docs, cfg, 2).has_value() && g_calls == 2);
    std::size_t changed = 0;
    for (std::size_t i = 0; i < docs.size(); ++i) {
        EXPECT(docs[i].embedding.size() == before[i].embedding.size());
        if (before[i].embedding.size() != 5) EXPECT(docs[i].embedding == before[i].embedding);
        else changed += docs[i].embedding != before[i].embedding;
    }
    EXPECT(changed > 0 && sgc->lastDiag().hops == 2);
    // the lists: symmetric, no self-loop, weights >= 0, offsets consistent
    const SGCLists l = AccelSGC::buildLists(before, cfg);
    EXPECT(l.rowOffsets.size() == before.size() + 1 && l.rowOffsets[0] == 0 && l.rowOffsets.back() == l.cols.size() && l.cols.size() == l.weights.size());
    for (std::size_t i = 0; i + 1 < l.rowOffsets.size(); ++i)
        for (uint64_t e = l.rowOffsets[i]; e < l.rowOffsets[i + 1]; ++e) {
            const uint32_t j = l.cols[e];
            EXPECT(j != i && j < before.size() && l.weights[e] >= 0.0f);
            bool back = false;
            for (uint64_t b = l.rowOffsets[j]; b < l.rowOffsets[j + 1]; ++b) back |= l.cols[b] == i && l.weights[b] == l.weights[e];
            EXPECT(back);
        }
    // reciprocalOnly off admits more; minEdgeScore at a score's exact value keeps that score
    TopologyBuildConfig all = cfg;
    all.reciprocalOnly = false;
    EXPECT(AccelSGC::buildLists(before, all).cols.size() > l.cols.size());
    std::vector<TopologyDocumentInput> two(2);
    two[0].documentHash = "a"; two[1].documentHash = "b";
    two[0].neighbors.push_back(TopologyNeighbor{"b", 0.5f, true});
    all.minEdgeScore = 0.5;
    EXPECT(AccelSGC::buildLists(two, all).cols.size() == 2);
    all.minEdgeScore = 0.5000001;
    EXPECT(AccelSGC::buildLists(two, all).cols.empty());
}

} // namespace

int main(int argc, char** argv) {
    shell_properties();
    int cases = 0;
    const std::size_t dims[3] = {1, 37, 64};
#ifdef SGC_WITH_REFERENCE
    // the shell over the stand-in against the reference's own function
    auto sgc = AccelSGC::over(&g_stand_in);
    for (int c = 0; c < 6; ++c) {
        const std::size_t dim = dims[c % 3], hops = 1 + c % 3;
        TopologyBuildConfig cfg;
        cfg.reciprocalOnly = c % 2 == 0;
        cfg.minEdgeScore = c < 3 ? 0.0 : 0.05;
        auto ours = seeded(100 + c, 3000, dim, 8);
        auto theirs = ours;
        applySGCSmoothing(theirs, cfg, hops);
        std::size_t diff;
        const bool ok = sgc->apply(ours, cfg, hops).has_value() && same_bits(ours, theirs, &diff);
        if (!ok) std::printf("case %d (dim %zu, hops %zu): %zu elements differ from applySGCSmoothing\n", c, dim, hops, diff);
        EXPECT(ok);
        ++cases;
    }
#endif
    if (argc >= 3 && std::string(argv[1]) == "--plugin") {
        auto plugin = yams::accel::Plugin::load(argv[2], "{\"device\":0}");
        if (!plugin.has_value()) { std::printf("plugin load failed: %s\n", plugin.error().message.c_str()); return 2; }
        auto real = AccelSGC::create(plugin.value());
        if (!real.has_value()) { std::printf("topology_smooth_v1 not served\n"); return 2; }
        auto stand_in = AccelSGC::over(&g_stand_in);
        for (int c = 0; c < 3; ++c) {
            TopologyBuildConfig cfg;
            cfg.reciprocalOnly = c != 1;
            auto a = seeded(200 + c, 600, dims[c], 8);
            auto b = a;
            std::size_t diff;
            const bool ok = real.value()->apply(a, cfg, 1 + c).has_value() && stand_in->apply(b, cfg, 1 + c).has_value() && same_bits(a, b, &diff);
            if (!ok) std::printf("plugin case %d: %zu elements differ from the scalar loop\n", c, diff);
            EXPECT(ok);
            ++cases;
        }
    }
    std::printf("%d cases\n%s (%d failures)\n", cases, g_failures ? "FAILED" : "OK", g_failures);
    return g_failures ? 1 : 0;
}
