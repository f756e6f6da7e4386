// semgraph_test.cpp — AccelSemanticGraph (include/yams_accel/semantic_graph.hpp) on recorded cases: the edges (source hash,
// neighbour hash, similarity bits, weight bits, rank), their order and the two pair counts that the reference's own loop
// produced (tests/golden/semantic_neighbors.json, written out as text by tests/test_semgraph_cpu.py write_adapter_cases).
//   semgraph_test <cases.txt> <plugin.so>     over the plugin's semantic_graph_v1 (needs a device)
//   semgraph_test <cases.txt> --stub          over a table of this file: a scalar restatement of the entry's contract, so
//                                             the shell is tested where there is no device
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "yams_accel/semantic_graph.hpp"

using namespace yams;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::printf("CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

namespace stub {

// yams_graph_semantic_neighbors_host as the header states it, one pair at a time
yams_status_t neighbors(void*, const float* rows, uint64_t n, uint32_t dim, const uint32_t* tie_rank, const uint32_t* source_rows,
                        uint64_t n_sources, uint32_t k, uint32_t flags, float threshold, uint32_t** out_rows, float** out_sims,
                        uint32_t** out_counts, float** out_inv_norm, yams_graph_diag_t* diag) {
    *out_rows = nullptr; *out_sims = nullptr; *out_counts = nullptr;
    if (out_inv_norm) *out_inv_norm = nullptr;
    if (diag) std::memset(diag, 0, sizeof *diag);
    const uint64_t S = source_rows ? n_sources : n;
    if (k > YAMS_GRAPH_MAX_K || dim > YAMS_GRAPH_MAX_DIM) return YAMS_ERR_UNSUPPORTED;
    if (k == 0 || n < 2 || S == 0) return YAMS_OK;
    std::vector<float> inv(n);
    for (uint64_t r = 0; r < n; ++r) {
        double s = 0.0;
        for (uint32_t d = 0; d < dim; ++d) s += double(rows[r * dim + d]) * double(rows[r * dim + d]);
        if (!std::isfinite(s)) return YAMS_ERR_INVALID_ARG;
        inv[r] = s <= 0.0 ? 0.0f : float(1.0 / std::sqrt(s));
        if (std::isinf(inv[r])) return YAMS_ERR_INVALID_ARG;
    }
    auto* o_rows = static_cast<uint32_t*>(std::malloc(S * k * 4));
    auto* o_sims = static_cast<float*>(std::malloc(S * k * 4));
    auto* o_counts = static_cast<uint32_t*>(std::malloc(S * 4));
    struct Cand { float sim; uint32_t rank, row; };
    for (uint64_t s = 0; s < S; ++s) {
        const uint64_t src = source_rows ? source_rows[s] : s;
        std::vector<Cand> c;
        for (uint64_t r = 0; r < n && inv[src] > 0.0f; ++r) {
            if (r == src || !(inv[r] > 0.0f)) continue;
            if (diag) ++diag->pairs_scored;
            double dot = 0.0;
            for (uint32_t d = 0; d < dim; ++d) dot += double(rows[src * dim + d]) * double(rows[r * dim + d]);
            const float sim = float((dot * double(inv[src])) * double(inv[r]));
            if ((flags & YAMS_GRAPH_FLAG_EXPLICIT_THRESHOLD) ? sim < threshold : sim <= 0.0f) continue;
            if (diag) ++diag->pairs_admitted;
            c.push_back(Cand{sim, tie_rank ? tie_rank[r] : uint32_t(r), uint32_t(r)});
        }
        std::sort(c.begin(), c.end(), [](const Cand& a, const Cand& b) { return a.sim != b.sim ? a.sim > b.sim : a.rank < b.rank; });
        o_counts[s] = uint32_t(std::min<size_t>(c.size(), k));
        for (uint32_t j = 0; j < k; ++j) {
            o_rows[s * k + j] = j < o_counts[s] ? c[j].row : 0xffffffffu;
            o_sims[s * k + j] = j < o_counts[s] ? c[j].sim : -INFINITY;
        }
    }
    *out_rows = o_rows; *out_sims = o_sims; *out_counts = o_counts;
    if (out_inv_norm) { *out_inv_norm = static_cast<float*>(std::malloc(n * 4)); std::memcpy(*out_inv_norm, inv.data(), n * 4); }
    return YAMS_OK;
}
void free_neighbors(void*, uint32_t* r, float* s, uint32_t* c, float* i) { std::free(r); std::free(s); std::free(c); std::free(i); }
yams_semantic_graph_v1 table = {YAMS_IFACE_SEMANTIC_GRAPH_V1_VERSION, nullptr, neighbors, free_neighbors};

} // namespace stub

static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: semgraph_test <cases.txt> <plugin.so | --stub>\n"); return 2; }
    std::unique_ptr<daemon::AccelSemanticGraph> graph;
    if (std::strcmp(argv[2], "--stub") == 0) {
        graph = daemon::AccelSemanticGraph::over(&stub::table);
    } else {
        auto plugin = accel::Plugin::load(argv[2], R"({"device":0})");
        if (!plugin.has_value()) { std::printf("plugin: %s\n", plugin.error().message.c_str()); return 1; }
        auto g = daemon::AccelSemanticGraph::create(plugin.value());
        if (!g.has_value()) { std::printf("interface: %s\n", g.error().message.c_str()); return 1; }
        graph = std::move(g.value());
    }
    std::ifstream in(argv[1]);
    std::string word;
    int cases = 0;
    while (in >> word) {
        if (word != "CASE") { std::printf("bad case file at %s\n", word.c_str()); return 2; }
        std::string name;
        size_t n, dim, k, n_edges;
        int has_threshold, n_sources;
        uint32_t thr_bits;
        in >> name >> n >> dim >> k >> has_threshold >> thr_bits >> n_sources;
        std::vector<std::string> hashes(n);
        std::vector<std::vector<float>> emb(n);
        for (size_t i = 0; i < n; ++i) {
            size_t d;
            in >> hashes[i] >> d;
            if (hashes[i] == "-") hashes[i].clear();
            emb[i].resize(d);
            for (auto& x : emb[i]) { uint32_t b; in >> b; x = from_bits(b); }
        }
        std::optional<std::vector<std::string>> sources;
        if (n_sources >= 0) { sources.emplace(size_t(n_sources)); for (auto& h : *sources) in >> h; }
        in >> word >> n_edges;
        struct Want { std::string src, dst; uint32_t sim, weight; size_t rank; };
        std::vector<Want> want(n_edges);
        for (auto& w : want) in >> w.src >> w.dst >> w.sim >> w.weight >> w.rank;
        size_t scored, admitted;
        in >> word >> scored >> admitted;
        (void)dim;
        auto r = graph->build(hashes, emb, sources, k, has_threshold ? std::optional<float>(from_bits(thr_bits)) : std::nullopt);
        ++cases;
        if (!r.has_value()) { ++failures; std::printf("%s: %s\n", name.c_str(), r.error().message.c_str()); continue; }
        const auto& got = r.value();
        bool ok = got.edges.size() == want.size() && got.similarityPairCount == scored && got.candidateNeighborCount == admitted;
        for (size_t i = 0; ok && i < want.size(); ++i) {
            const auto& e = got.edges[i];
            ok = e.sourceHash == want[i].src && e.neighborHash == want[i].dst && to_bits(e.similarity) == want[i].sim &&
                 to_bits(e.weight) == want[i].weight && e.rank == want[i].rank;
        }
        if (!ok) {
            ++failures;
            std::printf("%s: edges %zu (want %zu), pairs %zu / %zu (want %zu / %zu)\n", name.c_str(), got.edges.size(), want.size(),
                        got.similarityPairCount, got.candidateNeighborCount, scored, admitted);
        }
    }
    CHECK(cases >= 10);
    // the shell's own answers
    {
        std::vector<std::string> h{"b", "a"};
        std::vector<std::vector<float>> e{{1.0f, 0.0f}, {1.0f, 1.0f, 1.0f}};
        auto r = graph->build(h, e, std::nullopt, 8, std::nullopt);
        CHECK(!r.has_value() && r.error().code == ErrorCode::NotImplemented);           // differing dimensions
        std::vector<std::vector<float>> one{{1.0f, 0.0f}, {}};
        auto r1 = graph->build(h, one, std::nullopt, 8, std::nullopt);
        CHECK(r1.has_value() && r1.value().edges.empty() && r1.value().corpusHashes.size() == 1);   // one usable record
        std::vector<std::vector<float>> two{{1.0f, 0.0f}, {1.0f, 1.0f}};
        auto r2 = graph->build(h, two, std::optional<std::vector<std::string>>(std::vector<std::string>{"zz"}), 8, std::nullopt);
        CHECK(r2.has_value() && r2.value().edges.empty());                               // no requested source in the corpus
        auto r3 = graph->build(h, two, std::nullopt, 8, 7.5f);                           // clamped to 1.0: nothing reaches it
        CHECK(r3.has_value() && r3.value().edges.empty() && r3.value().similarityPairCount == 2);
        auto r4 = graph->build(h, two, std::nullopt, 65, std::nullopt);
        CHECK(!r4.has_value() && r4.error().code == ErrorCode::NotImplemented);           // beyond YAMS_GRAPH_MAX_K
    }
    std::printf("%d cases\n%s (%d failures)\n", cases, failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
