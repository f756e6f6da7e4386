// artifacts_shell_test.cpp — driver of include/yams_accel/topology_artifacts.hpp over one case file (written by
// tests/_artifacts_oracle.py write_case): per cluster the mean embedding of its members and the selected representatives, then
// the boundary spill; the results are printed and compared, by the Python tests, with tests/golden/cluster_artifacts.json.
//
//   artifacts_shell_test <case> [--fused]     AccelArtifacts over a stand-in table backed by the plain C++ loops below
//   artifacts_shell_test <case> [--fused] --plugin <lib>   the same through the real topology_artifacts_v1
//   built with -DARTIFACTS_WITH_REFERENCE and linked with the reference's own topology_representatives.cpp (and the stand-in
//   StaticCosineAnnIndex below, whose build fails: every cluster is then a candidate): the REFERENCE'S functions are called
//   instead of the shell, and the residual form this compiler gave them is probed and printed.  tests/golden/
//   make_artifacts_golden.py makes the golden file from that build.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#ifdef ARTIFACTS_WITH_REFERENCE
#include <yams/topology/topology_representatives.h>
#include <yams/vector/static_cosine_ann_index.h>
#include <topology_build_utils.h>      // the reference's src/topology (detail::meanEmbedding)
#endif
#include <yams_accel/topology_artifacts.hpp>

#ifdef ARTIFACTS_WITH_REFERENCE
namespace yams::vector {
class StaticCosineAnnIndex::Impl {};
StaticCosineAnnIndex::StaticCosineAnnIndex(std::unique_ptr<Impl> impl) : impl_(std::move(impl)) {}
StaticCosineAnnIndex::~StaticCosineAnnIndex() = default;
Result<std::shared_ptr<const StaticCosineAnnIndex>> StaticCosineAnnIndex::build(std::span<const std::size_t>, std::span<const std::vector<float>>) {
    return Error{ErrorCode::NotSupported, "stand-in: no index"};
}
Result<StaticCosineAnnSearchResult> StaticCosineAnnIndex::search(std::span<const float>, std::size_t, std::size_t) const {
    return Error{ErrorCode::NotSupported, "stand-in: no index"};
}
std::size_t StaticCosineAnnIndex::size() const noexcept { return 0; }
std::size_t StaticCosineAnnIndex::dimension() const noexcept { return 0; }
} // namespace yams::vector
using namespace yams::topology;
#else
namespace yams::topology {
// this test's own small types: the fields the two functions read or write
enum class DocumentTopologyRole : uint8_t { Core, Bridge, Medoid, Outlier };
struct TopologyDocumentInput { std::string documentHash; std::vector<float> embedding; };
struct TopologyBuildConfig {
    std::size_t maxNeighborsPerDocument{32};
    std::size_t overlapLimit{1};
    double overlapBoundaryDistanceRatio{1.05};
    double overlapResidualPenalty{1.0};
    bool allowOverlap{false};
};
struct DocumentClusterMembership {
    std::string documentHash, clusterId;
    DocumentTopologyRole role{DocumentTopologyRole::Core};
    std::vector<std::string> overlapClusterIds;
};
struct ClusterRoutingRepresentative { std::string documentHash; std::vector<float> embedding; };
struct ClusterArtifact {
    std::string clusterId;
    std::size_t memberCount{0};
    std::vector<std::string> memberDocumentHashes;
    std::vector<float> centroidEmbedding;
};
struct TopologyArtifactBatch { std::vector<ClusterArtifact> clusters; std::vector<DocumentClusterMembership> memberships; };
} // namespace yams::topology
using namespace yams::topology;

// ---- the stand-in table: the three entries as plain loops ----------------------------------------------------------------------
namespace standin {
bool fused = false;
inline double madd(double acc, double a, double b) {
    if (fused) return std::fma(a, b, acc);
    volatile double p = a * b;      // (volatile: a compiler that contracts may not fuse what is being defined here)
    return acc + p;
}
double cosineDistance(const float* a, const float* b, uint32_t dim) {
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (uint32_t i = 0; i < dim; ++i) {
        dot = std::fma(double(a[i]), double(b[i]), dot); na = std::fma(double(a[i]), double(a[i]), na); nb = std::fma(double(b[i]), double(b[i]), nb);
    }      // (exact products: fused or not, the same bits)
    if (na <= 0.0 || nb <= 0.0) return 2.0;
    const double c = dot / (std::sqrt(na) * std::sqrt(nb));
    return 1.0 - (c < -1.0 ? -1.0 : (1.0 < c ? 1.0 : c));
}
yams_status_t centroids(void*, const float* rows, uint64_t n, uint32_t dim, const uint64_t* off, const uint32_t* members, uint32_t c,
                        float** out_centroids, uint32_t** out_counts) {
    auto* cent = static_cast<float*>(std::calloc(size_t(c) * dim, 4));
    auto* cnt = static_cast<uint32_t*>(std::calloc(c, 4));
    for (uint32_t k = 0; k < c; ++k) {
        cnt[k] = uint32_t(off[k + 1] - off[k]);
        for (uint64_t m = off[k]; m < off[k + 1]; ++m) {
            if (members[m] >= n) { std::free(cent); std::free(cnt); return YAMS_ERR_INVALID_ARG; }
            for (uint32_t d = 0; d < dim; ++d) cent[size_t(k) * dim + d] += rows[size_t(members[m]) * dim + d];
        }
        if (cnt[k]) for (uint32_t d = 0; d < dim; ++d) cent[size_t(k) * dim + d] /= float(cnt[k]);
    }
    *out_centroids = cent; *out_counts = cnt;
    return YAMS_OK;
}
yams_status_t representatives(void*, const float* rows, uint64_t, uint32_t dim, const uint64_t* off, const uint32_t* cand, const float* cents,
                              const uint8_t* empty, uint32_t c, uint32_t n_extra, uint32_t** out_selected, uint32_t** out_counts) {
    auto* sel = static_cast<uint32_t*>(std::malloc(size_t(c) * n_extra * 4 + 4));
    auto* cnt = static_cast<uint32_t*>(std::calloc(c, 4));
    std::memset(sel, 0xff, size_t(c) * n_extra * 4);
    for (uint32_t k = 0; k < c; ++k) {
        if (empty && empty[k]) continue;
        const uint64_t m = off[k + 1] - off[k];
        const uint32_t* list = cand + off[k];
        std::vector<char> used(m, 0);
        std::vector<double> md(m, DBL_MAX);
        uint64_t last = 0;
        for (uint64_t s = 0; s < std::min<uint64_t>(m, n_extra); ++s) {
            const float* target = s == 0 ? cents + size_t(k) * dim : rows + size_t(list[last]) * dim;
            uint64_t best = m; double bestD = -1.0;
            for (uint64_t i = 0; i < m; ++i) {
                if (used[i]) continue;
                const double d = cosineDistance(rows + size_t(list[i]) * dim, target, dim);
                md[i] = d < md[i] ? d : md[i];
                if (md[i] > bestD) { bestD = md[i]; best = i; }
            }
            if (best == m) break;
            used[best] = 1; last = best; sel[size_t(k) * n_extra + s] = uint32_t(best); ++cnt[k];
        }
    }
    *out_selected = sel; *out_counts = cnt;
    return YAMS_OK;
}
yams_status_t residuals(void*, const float* rows, uint64_t n, uint32_t dim, const float* cents, uint32_t c, const uint32_t* primary,
                        const uint64_t* off, const uint32_t* cand, uint32_t form, double** out_pn, double** out_cn, double** out_rd) {
    if ((form == YAMS_RESIDUAL_FUSED) != fused) return YAMS_ERR_INVALID_ARG;
    const uint64_t pairs = off ? off[n] : n * c;
    auto* cn = static_cast<double*>(std::calloc(pairs + 1, 8));
    auto* pn = primary ? static_cast<double*>(std::calloc(n + 1, 8)) : nullptr;
    auto* rd = primary ? static_cast<double*>(std::calloc(pairs + 1, 8)) : nullptr;
    std::vector<double> pr(dim);
    for (uint64_t u = 0; u < n; ++u) {
        const float* e = rows + u * dim;
        const bool has = primary && primary[u] != YAMS_CLUSTER_NONE;
        double s = 0.0;
        for (uint32_t d = 0; d < dim; ++d) { pr[d] = has ? double(e[d]) - double(cents[size_t(primary[u]) * dim + d]) : 0.0; s = madd(s, pr[d], pr[d]); }
        if (pn) pn[u] = s;
        const uint64_t b = off ? off[u] : u * c, m = off ? off[u + 1] - off[u] : c;
        for (uint64_t j = 0; j < m; ++j) {
            const float* cc = cents + size_t(off ? cand[b + j] : j) * dim;
            double a = 0.0, q = 0.0;
            for (uint32_t d = 0; d < dim; ++d) { const double r = double(e[d]) - double(cc[d]); a = madd(a, r, r); q = madd(q, pr[d], r); }
            cn[b + j] = a;
            if (rd) rd[b + j] = q;
        }
    }
    if (out_pn) *out_pn = pn;
    *out_cn = cn;
    if (out_rd) *out_rd = rd;
    return YAMS_OK;
}
void free2f(void*, float* a, uint32_t* b) { std::free(a); std::free(b); }
void free2u(void*, uint32_t* a, uint32_t* b) { std::free(a); std::free(b); }
void free3(void*, double* a, double* b, double* c) { std::free(a); std::free(b); std::free(c); }
yams_topology_artifacts_v1 table = {1, nullptr, centroids, representatives, residuals, free2f, free2u, free3};
} // namespace standin
#endif

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
static bool rdStr(FILE* f, std::string& s) { uint32_t n; if (!rd(f, &n, 4)) return false; s.resize(n); return rd(f, s.data(), n); }
static bool rdVec(FILE* f, std::vector<float>& v) { uint32_t n; if (!rd(f, &n, 4)) return false; v.resize(n); return rd(f, v.data(), n * 4ull); }
static void printBits(const char* tag, const std::vector<float>& v) {
    std::printf("%s", tag);
    for (float x : v) { uint32_t b; std::memcpy(&b, &x, 4); std::printf(" %u", b); }
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: artifacts_shell_test <case> [--fused] [--plugin <lib>]\n"); return 2; }
    bool fused = false;
    const char* pluginPath = nullptr;
    for (int i = 2; i < argc; ++i) {
        if (std::string(argv[i]) == "--fused") fused = true;
        else if (std::string(argv[i]) == "--plugin" && i + 1 < argc) pluginPath = argv[++i];
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t nDocs, nClusters, nMemberships;
    std::vector<TopologyDocumentInput> docs;
    TopologyArtifactBatch batch;
    TopologyBuildConfig config;
    if (!rd(f, &nDocs, 4)) return 2;
    docs.resize(nDocs);
    for (auto& d : docs) if (!rdStr(f, d.documentHash) || !rdVec(f, d.embedding)) return 2;
    if (!rd(f, &nClusters, 4)) return 2;
    batch.clusters.resize(nClusters);
    for (auto& c : batch.clusters) {
        uint32_t m;
        if (!rdStr(f, c.clusterId) || !rd(f, &m, 4)) return 2;
        c.memberDocumentHashes.resize(m);
        for (auto& h : c.memberDocumentHashes) if (!rdStr(f, h)) return 2;
        c.memberCount = m;
    }
    if (!rd(f, &nMemberships, 4)) return 2;
    batch.memberships.resize(nMemberships);
    for (auto& m : batch.memberships) {
        uint8_t outlier;
        if (!rdStr(f, m.documentHash) || !rdStr(f, m.clusterId) || !rd(f, &outlier, 1)) return 2;
        if (outlier) m.role = DocumentTopologyRole::Outlier;
    }
    uint64_t limit, count; double ratio, penalty;
    if (!rd(f, &limit, 8) || !rd(f, &ratio, 8) || !rd(f, &penalty, 8) || !rd(f, &count, 8)) return 2;
    std::fclose(f);
    config.allowOverlap = true; config.overlapLimit = limit; config.overlapBoundaryDistanceRatio = ratio; config.overlapResidualPenalty = penalty;
    const std::span<const TopologyDocumentInput> span(docs);

#ifdef ARTIFACTS_WITH_REFERENCE
    (void)fused; (void)pluginPath;
    auto form = AccelArtifacts::probeResidualForm<TopologyDocumentInput, TopologyBuildConfig, TopologyArtifactBatch>(
        [](std::span<const TopologyDocumentInput> d, const TopologyBuildConfig& c, TopologyArtifactBatch& b) { return applyOrthogonalBoundarySpill(d, c, b); });
    std::printf("PROBE %s\n", !form.has_value() ? "neither" : (form.value() == ResidualForm::Fused ? "fused" : "separate"));
#else
    std::shared_ptr<yams::accel::Plugin> plugin;
    std::unique_ptr<AccelArtifacts> shell;
    const ResidualForm form = fused ? ResidualForm::Fused : ResidualForm::Separate;
    if (pluginPath) {
        auto p = yams::accel::Plugin::load(pluginPath, "{\"device\":0}");
        if (!p.has_value()) { std::fprintf(stderr, "plugin: %s\n", p.error().message.c_str()); return 3; }
        plugin = p.value();
        auto s = AccelArtifacts::create(plugin, form);
        if (!s.has_value()) return 3;
        shell = std::move(s.value());
    } else {
        standin::fused = fused;
        shell = AccelArtifacts::over(&standin::table, form);
        // the probe tells the stand-in's two forms apart, through the shell itself as the "host"
        auto probed = AccelArtifacts::probeResidualForm<TopologyDocumentInput, TopologyBuildConfig, TopologyArtifactBatch>(
            [&](std::span<const TopologyDocumentInput> d, const TopologyBuildConfig& c, TopologyArtifactBatch& b) {
                return shell->applyOrthogonalBoundarySpill(d, c, b).value();
            });
        std::printf("PROBE %s\n", !probed.has_value() ? "neither" : (probed.value() == ResidualForm::Fused ? "fused" : "separate"));
    }
#endif

    // per cluster: members as indices (the first document of a hash), the mean embedding, the representatives
    for (auto& cluster : batch.clusters) {
        std::vector<std::size_t> members;
        for (const auto& h : cluster.memberDocumentHashes) {
            std::size_t idx = docs.size() + 7;      // an unknown hash: an index out of range, which both functions skip
            for (std::size_t i = 0; i < docs.size(); ++i) if (docs[i].documentHash == h) { idx = i; break; }
            members.push_back(idx);
        }
#ifdef ARTIFACTS_WITH_REFERENCE
        cluster.centroidEmbedding = detail::meanEmbedding(span, members);
        const auto reps = selectDiverseRoutingRepresentatives(span, members, cluster.centroidEmbedding, count);
#else
        auto mean = shell->meanEmbedding(span, members);
        if (!mean.has_value()) { std::fprintf(stderr, "meanEmbedding: %s\n", mean.error().message.c_str()); return 4; }
        cluster.centroidEmbedding = mean.value();
        auto sel = shell->selectDiverseRoutingRepresentatives<ClusterRoutingRepresentative>(span, std::span<const std::size_t>(members),
                                                                                           std::span<const float>(cluster.centroidEmbedding), count);
        if (!sel.has_value()) { std::fprintf(stderr, "representatives: %s\n", sel.error().message.c_str()); return 4; }
        const auto reps = sel.value();
#endif
        printBits("MEAN", cluster.centroidEmbedding);
        std::printf("SEL");
        for (const auto& r : reps) std::printf(" %s", r.documentHash.c_str());
        std::printf("\n");
    }
#ifdef ARTIFACTS_WITH_REFERENCE
    const std::size_t assignments = applyOrthogonalBoundarySpill(span, config, batch);
#else
    auto spill = shell->applyOrthogonalBoundarySpill(span, config, batch);
    if (!spill.has_value()) { std::fprintf(stderr, "spill: %s\n", spill.error().message.c_str()); return 4; }
    const std::size_t assignments = spill.value();
#endif
    std::printf("ASSIGN %zu\n", assignments);
    for (const auto& m : batch.memberships) {
        std::printf("OVL");
        for (const auto& id : m.overlapClusterIds) std::printf(" %s", id.c_str());
        std::printf("\n");
    }
    for (const auto& c : batch.clusters) {
        std::printf("MEM");
        for (const auto& h : c.memberDocumentHashes) std::printf(" %s", h.c_str());
        std::printf("\n");
    }
    return 0;
}
