// route_shell_test — drives include/yams_accel/topology_route.hpp (AccelClusterRouter) on one case file
// (tests/_route_oracle.py write_case) and prints the index norms, the ordered routes and the work counters.
//   route_shell_test <case>...                the shell over a stand-in table (plain loops of the contract) and this file's own
//                                             small types: runs anywhere, also under ASan / UBSan
//   route_shell_test <case> --plugin <lib>    the same through the real topology_route_v1
//   route_shell_test <case> --batch           the case's request three times (one with another representative limit) through
//                                             routeBatch; every answer is printed
//   built with -DROUTE_WITH_REFERENCE and linked with the reference's own topology_baseline.cpp: the REFERENCE'S
//   buildRouteIndex and route are called instead of the shell.  tests/golden/make_route_golden.py makes the golden file from
//   that build.
// The ANN index is a stand-in in every build: it builds only where the case says so, and answers a search with the first
// `candidates` clusters and 3 evaluations per cluster.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <optional>
#include <string>
#include <vector>

static bool g_annBuilds = false;

#ifdef ROUTE_WITH_REFERENCE
#include <yams/topology/topology_baseline.h>
#include <yams/topology/protected_relation_cover.h>
#include <yams/topology/topology_representatives.h>
#include <yams/vector/static_cosine_ann_index.h>
// what the rest of that translation unit (the topology engine, never called here) references
namespace yams::topology {
std::string protectedRelationConstructionIdentity(std::span<const TopologyDocumentInput>, const TopologyBuildConfig&) { std::abort(); }
std::vector<ClusterRoutingRepresentative> selectDiverseRoutingRepresentatives(std::span<const TopologyDocumentInput>, std::span<const std::size_t>,
                                                                            std::span<const float>, std::size_t) { std::abort(); }
std::size_t applyOrthogonalBoundarySpill(std::span<const TopologyDocumentInput>, const TopologyBuildConfig&, TopologyArtifactBatch&) { std::abort(); }
} // namespace yams::topology
namespace yams::vector {
class StaticCosineAnnIndex::Impl { public: std::size_t n = 0; };
StaticCosineAnnIndex::StaticCosineAnnIndex(std::unique_ptr<Impl> impl) : impl_(std::move(impl)) {}
StaticCosineAnnIndex::~StaticCosineAnnIndex() = default;
Result<std::shared_ptr<const StaticCosineAnnIndex>> StaticCosineAnnIndex::build(std::span<const std::size_t> ids, std::span<const std::vector<float>>) {
    if (!g_annBuilds) return Error{ErrorCode::NotSupported, "stand-in: no index"};
    auto impl = std::make_unique<Impl>();
    impl->n = ids.size();
    return std::shared_ptr<const StaticCosineAnnIndex>(new StaticCosineAnnIndex(std::move(impl)));
}
Result<StaticCosineAnnSearchResult> StaticCosineAnnIndex::search(std::span<const float>, std::size_t candidates, std::size_t) const {
    StaticCosineAnnSearchResult r;
    for (std::size_t i = 0; i < std::min(candidates, impl_->n); ++i) r.hits.push_back({i, 0.0F});
    r.distanceEvaluations = 3 * impl_->n;
    return r;
}
std::size_t StaticCosineAnnIndex::size() const noexcept { return impl_->n; }
std::size_t StaticCosineAnnIndex::dimension() const noexcept { return 0; }
} // namespace yams::vector
using namespace yams::topology;
#else
#include <yams_accel/topology_route.hpp>
namespace yams::topology {
// this test's own small types: the fields the two functions read or write
struct AnnHit { std::size_t id{0}; float distance{0.0F}; };
struct AnnSearchResult { std::vector<AnnHit> hits; std::size_t distanceEvaluations{0}; };
struct StandInAnn {
    std::size_t n = 0;
    Result<AnnSearchResult> search(const std::vector<float>&, std::size_t candidates) const {
        AnnSearchResult r;
        for (std::size_t i = 0; i < std::min(candidates, n); ++i) r.hits.push_back({i, 0.0F});
        r.distanceEvaluations = 3 * n;
        return r;
    }
};
struct SparseRouteIndex {
    std::unordered_map<std::string, std::vector<std::size_t>> clustersByDocumentHash;
    std::vector<float> centroidNorms;
    std::vector<std::vector<float>> routingRepresentativeNorms;
    std::shared_ptr<const StandInAnn> centroidAnnIndex;
};
struct SparseRouteWork {
    std::size_t seedClusterLookups{0}, clusterMemberHashesScanned{0}, queryNormEvaluations{0}, representativeDistanceEvaluations{0},
        exactRepresentativeDistanceEvaluations{0}, denseAnnDistanceEvaluations{0}, denseAnnCandidates{0};
    bool denseAnnUsed{false};
};
struct DocumentClusterMembership {
    std::string documentHash, clusterId;
    std::optional<std::string> parentClusterId;
    std::vector<std::string> overlapClusterIds;
};
struct ClusterRepresentative { std::string clusterId, documentHash; };
struct ClusterRoutingRepresentative { std::string documentHash; std::vector<float> embedding; };
struct ClusterArtifact {
    std::string clusterId;
    std::size_t memberCount{0};
    double persistenceScore{0.0}, cohesionScore{0.0};
    std::optional<ClusterRepresentative> medoid;
    std::vector<std::string> memberDocumentHashes;
    std::vector<float> centroidEmbedding;
    std::vector<ClusterRoutingRepresentative> routingRepresentatives;
};
struct TopologyArtifactBatch { std::vector<ClusterArtifact> clusters; std::vector<DocumentClusterMembership> memberships; };
enum class RouteScoringMode : uint8_t { Current, SizeWeighted, SeedCoverage };
struct WeightedDocumentSeed { std::string documentHash; float weight{0.0F}; };
struct TopologyRouteRequest {
    std::vector<std::string> seedDocumentHashes;
    std::vector<WeightedDocumentSeed> weightedSeedDocuments;
    std::size_t limit{8};
    RouteScoringMode scoringMode{RouteScoringMode::Current};
    std::vector<float> queryEmbedding;
    float sparseDenseAlpha{0.5F};
    std::size_t maxRoutingRepresentatives{0}, denseAnnCandidateLimit{0};
};
struct ClusterRoute {
    std::string clusterId;
    std::optional<std::string> medoidDocumentHash;
    double routeScore{0.0}, stabilityScore{0.0};
    std::size_t memberCount{0};
    std::optional<double> semanticCost, sparseCost;
    double persistencePenalty{1.0}, cohesionPenalty{1.0}, sizePenalty{0.0};
};
} // namespace yams::topology
using namespace yams::topology;

// ---- the stand-in table: the entries as plain loops of the contract in include/yams_mi355x_accel.h -----------------------
namespace standin {
struct Table { std::vector<float> vectors, norms; std::vector<uint32_t> off; std::vector<uint8_t> has; std::vector<uint16_t> pos; uint32_t dim = 0; };
std::vector<std::unique_ptr<Table>> tables;
float norm(const float* v, uint32_t dim) {
    double acc = 0.0;
    for (uint32_t i = 0; i < dim; ++i) acc = std::fma(double(v[i]), double(v[i]), acc);      // (exact products: fused or not, the same bits)
    return float(std::sqrt(acc));
}
yams_status_t index_create(void*, const float* vectors, uint64_t v, uint32_t dim, const uint32_t* off, const uint8_t* has, const uint16_t* pos,
                           uint32_t c, uint64_t* out_id, float* out_norms) {
    if (dim == 0 || dim > YAMS_ROUTE_MAX_DIM || c > YAMS_ROUTE_MAX_CLUSTERS || off[0] != 0 || off[c] != v) return YAMS_ERR_INVALID_ARG;
    auto t = std::make_unique<Table>();
    t->dim = dim;
    t->vectors.assign(vectors, vectors + v * dim);
    t->off.assign(off, off + c + 1);
    t->has.assign(has, has + c);
    t->pos.assign(pos, pos + v);
    for (uint64_t r = 0; r < v; ++r) t->norms.push_back(norm(vectors + r * dim, dim));
    if (out_norms) std::memcpy(out_norms, t->norms.data(), v * 4);
    tables.push_back(std::move(t));
    *out_id = tables.size();
    return YAMS_OK;
}
yams_status_t index_info(void*, uint64_t, yams_route_index_info_t*) { return YAMS_ERR_UNSUPPORTED; }
float dense_of(const float* q, const float* v, uint32_t dim, float qn, float vn) {
    double acc = 0.0;
    for (uint32_t i = 0; i < dim; ++i) acc = std::fma(double(q[i]), double(v[i]), acc);
    volatile float product = qn * vn;      // (volatile: every float step is rounded where it stands)
    volatile float cosine = float(acc) / product;
    volatile float sum = cosine + 1.0F;
    const float d = sum * 0.5F;
    return (d < 0.0F) ? 0.0F : (1.0F < d) ? 1.0F : d;
}
yams_status_t dense(void*, uint64_t id, const float* queries, uint32_t nq, uint32_t rep_limit, const uint32_t* cand, float* out_dense,
                    uint8_t* out_observed, uint32_t* out_evals, yams_route_diag_t*) {
    if (id == 0 || id > tables.size() || !tables[id - 1]) return YAMS_ERR_NOT_FOUND;
    if (nq > YAMS_ROUTE_MAX_QUERIES) return YAMS_ERR_INVALID_ARG;
    const Table& t = *tables[id - 1];
    const uint32_t c = uint32_t(t.has.size()), words = (c + 31) / 32;
    for (uint32_t q = 0; q < nq; ++q) {
        const float* x = queries + size_t(q) * t.dim;
        const float qn = norm(x, t.dim);
        out_evals[q] = 0;
        for (uint32_t k = 0; k < c; ++k) {
            float cur = 0.0F; bool obs = false;
            if (!cand || ((cand[size_t(q) * words + k / 32] >> (k % 32)) & 1u)) {
                for (uint32_t r = t.off[k]; r < t.off[k + 1]; ++r) {
                    const bool centroid = t.has[k] && r == t.off[k];
                    const float vn = t.norms[r];
                    if (centroid) { if (!(qn > 0.0F && vn > 0.0F)) continue; }
                    else if ((rep_limit && t.pos[r] >= rep_limit - 1) || qn <= 0.0F || vn <= 0.0F) continue;
                    const float d = dense_of(x, t.vectors.data() + size_t(r) * t.dim, t.dim, qn, vn);
                    cur = centroid ? d : ((cur < d) ? d : cur);
                    obs = true; ++out_evals[q];
                }
            }
            out_dense[size_t(q) * c + k] = cur; out_observed[size_t(q) * c + k] = obs;
        }
    }
    return YAMS_OK;
}
yams_status_t index_destroy(void*, uint64_t id) {
    if (id == 0 || id > tables.size() || !tables[id - 1]) return YAMS_ERR_NOT_FOUND;
    tables[id - 1].reset();
    return YAMS_OK;
}
yams_topology_route_v1 table = {1, nullptr, index_create, index_info, dense, index_destroy};
} // namespace standin
#endif

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
static bool rdStr(FILE* f, std::string& s) { uint32_t n; if (!rd(f, &n, 4)) return false; s.resize(n); return rd(f, s.data(), n); }
static bool rdVec(FILE* f, std::vector<float>& v) { uint32_t n; if (!rd(f, &n, 4)) return false; v.resize(n); return rd(f, v.data(), n * 4ull); }
static void printOpt(const std::optional<double>& v) { if (v.has_value()) std::printf(" %a", *v); else std::printf(" none"); }
static void printRoutes(const std::vector<ClusterRoute>& routes, const SparseRouteWork& w) {
    for (const auto& r : routes) {
        std::printf("route %s %a", r.clusterId.c_str(), r.routeScore);
        printOpt(r.semanticCost); printOpt(r.sparseCost);
        std::printf("\n");
    }
    std::printf("work %zu %zu %zu %zu %d %zu %zu\n", w.seedClusterLookups, w.queryNormEvaluations, w.representativeDistanceEvaluations,
                w.exactRepresentativeDistanceEvaluations, w.denseAnnUsed ? 1 : 0, w.denseAnnCandidates, w.denseAnnDistanceEvaluations);
}

#ifndef ROUTE_WITH_REFERENCE
static std::unique_ptr<AccelClusterRouter> g_shell;
#endif

static int runCase(const char* casePath, bool batch) {
    FILE* f = std::fopen(casePath, "rb");
    if (!f) return 2;
    TopologyArtifactBatch artifacts;
    TopologyRouteRequest request;
    uint32_t nClusters, n;
    if (!rd(f, &nClusters, 4)) return 2;
    artifacts.clusters.resize(nClusters);
    for (auto& c : artifacts.clusters) {
        if (!rdStr(f, c.clusterId) || !rdVec(f, c.centroidEmbedding) || !rd(f, &n, 4)) return 2;
        c.routingRepresentatives.resize(n);
        for (auto& r : c.routingRepresentatives) if (!rdStr(f, r.documentHash) || !rdVec(f, r.embedding)) return 2;
        if (!rd(f, &n, 4)) return 2;
        c.memberDocumentHashes.resize(n);
        for (auto& h : c.memberDocumentHashes) if (!rdStr(f, h)) return 2;
        uint64_t count;
        if (!rd(f, &count, 8) || !rd(f, &c.persistenceScore, 8) || !rd(f, &c.cohesionScore, 8)) return 2;
        c.memberCount = count;
    }
    uint64_t maxReps, annLimit, limit; uint8_t mode, annBuilds;
    if (!rdVec(f, request.queryEmbedding) || !rd(f, &request.sparseDenseAlpha, 4) || !rd(f, &maxReps, 8) || !rd(f, &annLimit, 8) ||
        !rd(f, &limit, 8) || !rd(f, &mode, 1) || !rd(f, &n, 4)) return 2;
    request.maxRoutingRepresentatives = maxReps; request.denseAnnCandidateLimit = annLimit; request.limit = limit;
    request.scoringMode = static_cast<RouteScoringMode>(mode);
    request.seedDocumentHashes.resize(n);
    for (auto& h : request.seedDocumentHashes) if (!rdStr(f, h)) return 2;
    if (!rd(f, &n, 4)) return 2;
    request.weightedSeedDocuments.resize(n);
    for (auto& s : request.weightedSeedDocuments) if (!rdStr(f, s.documentHash) || !rd(f, &s.weight, 4)) return 2;
    if (!rd(f, &annBuilds, 1)) return 2;
    std::fclose(f);
    g_annBuilds = annBuilds != 0;

#ifdef ROUTE_WITH_REFERENCE
    (void)batch;
    const SparseRouteIndex index = SparseGuidedClusterRouter::buildRouteIndex(artifacts, request.denseAnnCandidateLimit > 0);
#else
    AccelClusterRouter* shell = g_shell.get();
    auto annBuild = [](const std::vector<std::size_t>& ids, const std::vector<std::vector<float>>&) -> std::shared_ptr<const StandInAnn> {
        if (!g_annBuilds) return nullptr;
        auto a = std::make_shared<StandInAnn>();
        a->n = ids.size();
        return a;
    };
    auto built = request.denseAnnCandidateLimit > 0 ? shell->buildRouteIndex<SparseRouteIndex>(artifacts, annBuild)
                                                    : shell->buildRouteIndex<SparseRouteIndex>(artifacts, nullptr);
    if (!built.has_value()) { std::printf("error index %s\n", built.error().message.c_str()); return 0; }
    const SparseRouteIndex index = std::move(built.value());
#endif
    std::printf("norms");
    for (std::size_t c = 0; c < index.centroidNorms.size(); ++c) {
        uint32_t b; std::memcpy(&b, &index.centroidNorms[c], 4); std::printf(" %u", b);
        for (float x : index.routingRepresentativeNorms[c]) { std::memcpy(&b, &x, 4); std::printf(" %u", b); }
    }
    std::printf("\n");

#ifdef ROUTE_WITH_REFERENCE
    SparseRouteWork work;
    auto routed = SparseGuidedClusterRouter{}.route(request, artifacts, index, &work);
    if (!routed) { std::printf("error route %s\n", routed.error().message.c_str()); return 0; }
    printRoutes(routed.value(), work);
#else
    if (!batch) {
        SparseRouteWork work;
        auto routed = shell->route<ClusterRoute>(request, artifacts, index, &work);
        if (!routed.has_value()) { std::printf("error route %s\n", routed.error().message.c_str()); return 0; }
        printRoutes(routed.value(), work);
    } else {
        std::vector<TopologyRouteRequest> requests(3, request);
        requests[1].maxRoutingRepresentatives = request.maxRoutingRepresentatives + 1;      // a call of its own between the two
        SparseRouteWork works[3];
        SparseRouteWork* ptrs[3] = {&works[0], &works[1], &works[2]};
        auto all = shell->routeBatch<ClusterRoute>(std::span<const TopologyRouteRequest>(requests), artifacts, index,
                                                   std::span<SparseRouteWork* const>(ptrs, 3));
        for (int i = 0; i < 3; ++i) {
            std::printf("request %d\n", i);
            if (!all[i].has_value()) { std::printf("error route %s\n", all[i].error().message.c_str()); continue; }
            printRoutes(all[i].value(), works[i]);
        }
    }
#endif
    return 0;
}

int main(int argc, char** argv) {
    bool batch = false;
    const char* pluginPath = nullptr;
    std::vector<const char*> cases;
    for (int i = 1; i < argc; ++i) {
        if (std::string(argv[i]) == "--batch") batch = true;
        else if (std::string(argv[i]) == "--plugin" && i + 1 < argc) pluginPath = argv[++i];
        else cases.push_back(argv[i]);
    }
    if (cases.empty()) { std::fprintf(stderr, "usage: route_shell_test <case>... [--batch] [--plugin <lib>]\n"); return 2; }
#ifdef ROUTE_WITH_REFERENCE
    (void)pluginPath;
#else
    std::shared_ptr<yams::accel::Plugin> plugin;
    if (pluginPath) {
        auto p = yams::accel::Plugin::load(pluginPath, "{\"device\":0}");
        if (!p.has_value()) { std::fprintf(stderr, "plugin: %s\n", p.error().message.c_str()); return 3; }
        plugin = p.value();
        auto s = AccelClusterRouter::create(plugin);
        if (!s.has_value()) return 3;
        g_shell = std::move(s.value());
    } else {
        g_shell = AccelClusterRouter::over(&standin::table);
    }
#endif
    int status = 0;
    for (std::size_t i = 0; i < cases.size() && status == 0; ++i) {      // several cases: one plugin, one shell, an index each
        std::printf("case %zu\n", i);
        status = runCase(cases[i], batch);
    }
#ifndef ROUTE_WITH_REFERENCE
    g_shell.reset();      // (the index goes before the plugin)
#endif
    return status;
}
