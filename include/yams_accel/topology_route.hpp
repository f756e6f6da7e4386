// topology_route.hpp — SparseGuidedClusterRouter::buildRouteIndex and ::route of the reference
// (src/topology/topology_baseline.cpp:700-769, :771-981) with the dense signal's array arithmetic on the device (plugin
// interface topology_route_v1): the query's cosine to every candidate cluster's centroid and routing representatives, the
// map to [0, 1] and the maximum per cluster (:873-920).
//
// What stays on the host, here, line for line:
//   buildRouteIndex   the hash map clustersByDocumentHash (:739-767), the centroid ANN index (:718-737: the host's own
//                     StaticCosineAnnIndex, through a callable), the shapes of centroidNorms / routingRepresentativeNorms
//   route             the index / artifact size tests (:775-779, :891-894), the seed sets and the sparse mass (:781-836), alpha
//                     and the ANN shortlist (:838-871: the host's own index->search), the blend
//                     alpha * sparseNorm + (1 - alpha) * dense — a float expression the host's compiler may contract, so it is
//                     compiled HERE, by the host's compiler —, the scoring modes, log1p, the sort and the cut (:922-980)
// What the device computes: vectorNorm of every cluster vector (once per index: they fill centroidNorms /
// routingRepresentativeNorms) and, per query, dense / denseObserved of every candidate cluster and the number of evaluations.
//
// A case is served exactly or not at all.  An Error comes back — and the host runs its own function — for: a non-empty
// centroid whose size differs from the index dimension (the reference then scores a zero dot, :670), a query of another size,
// and any refusal of the plugin.  Representatives of another size are left out of the device's table; their places in the
// list still count towards maxRoutingRepresentatives, and their norms are computed here (the same chain; its products are
// exact in fp64, so no compiler can change its bits).
//
// The functions are templates over the host's own types (TopologyArtifactBatch, SparseRouteIndex, TopologyRouteRequest,
// ClusterRoute, SparseRouteWork, RouteScoringMode): they read and write the fields the reference's functions do, by name.
// One AccelClusterRouter holds one resident index: buildRouteIndex replaces it.  Not thread-safe.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <optional>
#include <span>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "plugin.hpp"

namespace yams::topology {

class AccelClusterRouter {
public:
    static Result<std::unique_ptr<AccelClusterRouter>> create(std::shared_ptr<accel::Plugin> plugin) {
        auto vt = plugin->getInterface<yams_topology_route_v1>(YAMS_IFACE_TOPOLOGY_ROUTE_V1, YAMS_IFACE_TOPOLOGY_ROUTE_V1_VERSION);
        if (!vt.has_value()) return vt.error();
        return std::unique_ptr<AccelClusterRouter>(new AccelClusterRouter(std::move(plugin), vt.value()));
    }
    // Over a table the caller owns (a host that binds the interface itself).
    static std::unique_ptr<AccelClusterRouter> over(yams_topology_route_v1* vt) {
        return std::unique_ptr<AccelClusterRouter>(new AccelClusterRouter(nullptr, vt));
    }
    ~AccelClusterRouter() { drop(); }
    AccelClusterRouter(const AccelClusterRouter&) = delete;
    AccelClusterRouter& operator=(const AccelClusterRouter&) = delete;

    // vectorNorm (:680-689) for what the device's table does not hold
    static float hostNorm(const std::vector<float>& a) {
        if (a.empty()) return 0.0F;
        double acc = 0.0;
        for (const float v : a) acc += static_cast<double>(v) * static_cast<double>(v);
        return static_cast<float>(std::sqrt(acc));
    }

    // buildRouteIndex(artifacts, buildDenseAnnIndex).  buildAnn(centroidIds, centroids) is the host's
    // StaticCosineAnnIndex::build, returning what index.centroidAnnIndex holds (null when the build fails); pass nullptr for
    // buildDenseAnnIndex == false.
    template <class Index, class Batch, class AnnBuild>
    Result<Index> buildRouteIndex(const Batch& artifacts, AnnBuild&& buildAnn) {
        drop();
        const std::size_t nClusters = artifacts.clusters.size();
        if (nClusters > YAMS_ROUTE_MAX_CLUSTERS) return Error{ErrorCode::NotSupported, "more clusters than the accelerator's route index holds"};
        // the index dimension: the first non-empty centroid's, else the first non-empty representative's
        std::size_t dim = 0;
        for (const auto& cluster : artifacts.clusters)
            if (!cluster.centroidEmbedding.empty()) { dim = cluster.centroidEmbedding.size(); break; }
        for (std::size_t c = 0; dim == 0 && c < nClusters; ++c)
            for (const auto& representative : artifacts.clusters[c].routingRepresentatives)
                if (!representative.embedding.empty()) { dim = representative.embedding.size(); break; }
        if (dim > YAMS_ROUTE_MAX_DIM) return Error{ErrorCode::NotSupported, "dimension beyond the accelerator's route index"};

        Index index;
        index.centroidNorms.assign(nClusters, 0.0F);
        index.routingRepresentativeNorms.resize(nClusters);
        std::vector<float> table;
        std::vector<std::uint32_t> offsets(nClusters + 1, 0);
        std::vector<std::uint8_t> hasCentroid(nClusters, 0);
        std::vector<std::uint16_t> position;
        std::vector<std::pair<std::uint32_t, std::uint32_t>> slot;      // (cluster, place in its list + 1; 0 = the centroid) of every row
        for (std::size_t c = 0; c < nClusters; ++c) {
            const auto& cluster = artifacts.clusters[c];
            if (!cluster.centroidEmbedding.empty()) {
                if (cluster.centroidEmbedding.size() != dim)
                    return Error{ErrorCode::NotSupported, "a centroid of another size than the index dimension"};
                table.insert(table.end(), cluster.centroidEmbedding.begin(), cluster.centroidEmbedding.end());
                position.push_back(0);
                slot.emplace_back(static_cast<std::uint32_t>(c), 0u);
                hasCentroid[c] = 1;
            }
            auto& norms = index.routingRepresentativeNorms[c];
            norms.assign(cluster.routingRepresentatives.size(), 0.0F);
            std::size_t rows = 0;
            for (std::size_t p = 0; p < cluster.routingRepresentatives.size(); ++p) {
                const auto& embedding = cluster.routingRepresentatives[p].embedding;
                if (embedding.size() != dim || dim == 0) { norms[p] = hostNorm(embedding); continue; }      // never scored: :907
                if (p >= 0xffffu || ++rows > YAMS_ROUTE_MAX_REPRESENTATIVES)
                    return Error{ErrorCode::NotSupported, "more routing representatives than the accelerator's route index holds"};
                table.insert(table.end(), embedding.begin(), embedding.end());
                position.push_back(static_cast<std::uint16_t>(p));
                slot.emplace_back(static_cast<std::uint32_t>(c), static_cast<std::uint32_t>(p + 1));
            }
            offsets[c + 1] = static_cast<std::uint32_t>(position.size());
        }
        std::vector<float> norms(position.size());
        std::uint64_t id = 0;
        const yams_status_t st = vt_->index_create(vt_->self, table.data(), position.size(), static_cast<std::uint32_t>(dim ? dim : 1),
                                                   offsets.data(), hasCentroid.data(), position.data(), static_cast<std::uint32_t>(nClusters),
                                                   &id, norms.data());
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_route_v1.index_create refused the call"};
        id_ = id; live_ = true; dim_ = dim; clusters_ = nClusters;
        for (std::size_t r = 0; r < slot.size(); ++r) {
            if (slot[r].second == 0) index.centroidNorms[slot[r].first] = norms[r];
            else index.routingRepresentativeNorms[slot[r].first][slot[r].second - 1] = norms[r];
        }

        // :718-737 — the host's ANN index over the centroids, only when every cluster has a live one
        std::vector<std::size_t> centroidIds;
        std::vector<std::vector<float>> centroids;
        for (std::size_t c = 0; c < nClusters; ++c) {
            const auto& centroid = artifacts.clusters[c].centroidEmbedding;
            if (centroid.empty() || index.centroidNorms[c] <= 0.0F) { centroidIds.clear(); centroids.clear(); break; }
            centroidIds.push_back(c);
            centroids.push_back(centroid);
        }
        if constexpr (!std::is_same_v<std::decay_t<AnnBuild>, std::nullptr_t>) {
            if (!centroids.empty()) index.centroidAnnIndex = buildAnn(centroidIds, centroids);
        }

        // :739-767
        std::unordered_map<std::string, std::size_t> clusterIndexById;
        clusterIndexById.reserve(nClusters);
        for (std::size_t c = 0; c < nClusters; ++c) clusterIndexById.emplace(artifacts.clusters[c].clusterId, c);
        auto addMembership = [&](const std::string& hash, const std::string& clusterId) {
            const auto clusterIt = clusterIndexById.find(clusterId);
            if (hash.empty() || clusterIt == clusterIndexById.end()) return;
            auto& clusters = index.clustersByDocumentHash[hash];
            if (std::find(clusters.begin(), clusters.end(), clusterIt->second) == clusters.end()) clusters.push_back(clusterIt->second);
        };
        if (!artifacts.memberships.empty()) {
            for (const auto& membership : artifacts.memberships) {
                addMembership(membership.documentHash, membership.clusterId);
                if (membership.parentClusterId.has_value()) addMembership(membership.documentHash, *membership.parentClusterId);
                for (const auto& overlapClusterId : membership.overlapClusterIds) addMembership(membership.documentHash, overlapClusterId);
            }
        } else {
            for (std::size_t c = 0; c < nClusters; ++c)
                for (const auto& hash : artifacts.clusters[c].memberDocumentHashes) index.clustersByDocumentHash[hash].push_back(c);
        }
        return index;
    }

    // route(request, artifacts, index, work): `index` is what buildRouteIndex returned for `artifacts`.
    template <class Route, class Request, class Batch, class Index, class Work>
    Result<std::vector<Route>> route(const Request& request, const Batch& artifacts, const Index& index, Work* work = nullptr) {
        Work* works[1] = {work};
        auto all = routeBatch<Route>(std::span<const Request>(&request, 1), artifacts, index, std::span<Work* const>(works, 1));
        return std::move(all[0]);
    }

    // Several requests against one snapshot: one device call per 1024 scoring requests.  works: empty (a span of the host's Work type), or one (nullable)
    // pointer per request.  A request that cannot be served gets its own Error; a refusal of the plugin gives every scoring
    // request of that call an Error.
    template <class Route, class Request, class Batch, class Index, class Work>
    std::vector<Result<std::vector<Route>>> routeBatch(std::span<const Request> requests, const Batch& artifacts, const Index& index,
                                                      std::span<Work* const> works) {
        using Mode = std::decay_t<decltype(requests[0].scoringMode)>;
        const std::size_t nClusters = artifacts.clusters.size();
        std::vector<Result<std::vector<Route>>> out(requests.size());
        struct Pending {
            std::vector<double> sparseMass; double maxSparseMass = 0.0; float alpha = 0.0F; std::vector<bool> routeCandidates; bool scores = false;
            bool failed = false;
        };
        std::vector<Pending> pending(requests.size());
        if (!live_ || nClusters != clusters_ || index.centroidNorms.size() != nClusters || index.routingRepresentativeNorms.size() != nClusters) {
            for (auto& r : out) r = Error{ErrorCode::InvalidArgument, "sparse route index does not match topology clusters"};      // :775-779
            return out;
        }
        for (std::size_t c = 0; c < nClusters; ++c)
            if (index.routingRepresentativeNorms[c].size() != artifacts.clusters[c].routingRepresentatives.size()) {
                for (auto& r : out) r = Error{ErrorCode::InvalidArgument, "sparse route index does not match routing representatives"};  // :891-894
                return out;
            }

        std::vector<std::size_t> scoring;
        for (std::size_t i = 0; i < requests.size(); ++i) {
            const Request& request = requests[i];
            Work* work = i < works.size() ? works[i] : nullptr;
            Pending& p = pending[i];
            // :781-836
            std::unordered_set<std::string> seeds(request.seedDocumentHashes.begin(), request.seedDocumentHashes.end());
            std::unordered_map<std::string, float> weightedSeeds;
            weightedSeeds.reserve(request.weightedSeedDocuments.size());
            for (const auto& seed : request.weightedSeedDocuments) {
                if (seed.documentHash.empty() || !std::isfinite(seed.weight) || seed.weight <= 0.0F) continue;
                auto [it, inserted] = weightedSeeds.emplace(seed.documentHash, seed.weight);
                if (!inserted) it->second = std::max(it->second, seed.weight);
            }
            p.sparseMass.assign(nClusters, 0.0);
            auto vote = [&](const std::string& hash, double weight) {
                if (work != nullptr) ++work->seedClusterLookups;
                const auto clusterIt = index.clustersByDocumentHash.find(hash);
                if (clusterIt == index.clustersByDocumentHash.end()) return;
                for (const auto clusterIndex : clusterIt->second)
                    if (clusterIndex < nClusters) p.sparseMass[clusterIndex] += weight;
            };
            if (!weightedSeeds.empty()) {
                for (const auto& [hash, weight] : weightedSeeds) vote(hash, static_cast<double>(weight));
            } else {
                for (const auto& hash : seeds) vote(hash, 1.0);
            }
            for (const double mass : p.sparseMass) p.maxSparseMass = std::max(p.maxSparseMass, mass);

            // :838-871
            p.alpha = std::clamp(request.sparseDenseAlpha, 0.0F, 1.0F);
            const float queryNorm = hostNorm(request.queryEmbedding);
            if (!request.queryEmbedding.empty() && work != nullptr) ++work->queryNormEvaluations;
            p.routeCandidates.assign(nClusters, true);
            const bool denseAnnEligible = p.alpha < 1.0F && queryNorm > 0.0F && request.limit > 0 && request.denseAnnCandidateLimit > 0 &&
                                          index.centroidAnnIndex && nClusters > request.denseAnnCandidateLimit;
            if (denseAnnEligible) {
                const auto candidateLimit = std::min(nClusters, std::max(request.denseAnnCandidateLimit, request.limit));
                auto annResult = index.centroidAnnIndex->search(request.queryEmbedding, candidateLimit);
                if (annResult) {
                    std::fill(p.routeCandidates.begin(), p.routeCandidates.end(), false);
                    for (const auto& hit : annResult.value().hits)
                        if (hit.id < p.routeCandidates.size()) p.routeCandidates[hit.id] = true;
                    for (std::size_t c = 0; c < nClusters; ++c)
                        if (p.sparseMass[c] > 0.0) p.routeCandidates[c] = true;
                    if (work != nullptr) {
                        work->denseAnnUsed = true;
                        work->denseAnnCandidates = annResult.value().hits.size();
                        work->denseAnnDistanceEvaluations = annResult.value().distanceEvaluations;
                        work->representativeDistanceEvaluations += annResult.value().distanceEvaluations;
                    }
                }
            }
            // the loop :873-920 evaluates something only with alpha < 1 and a non-empty query (an empty one has norm 0)
            if (!(p.alpha >= 1.0F) && !request.queryEmbedding.empty() && nClusters > 0 && dim_ > 0) {
                if (request.queryEmbedding.size() != dim_) {
                    out[i] = Error{ErrorCode::NotSupported, "a query of another size than the index dimension"};
                    p.failed = true;
                    continue;
                }
                p.scores = true;
                scoring.push_back(i);
            }
        }

        // the device: dense / denseObserved / evaluations of every scoring request
        const std::size_t words = (nClusters + 31) / 32;
        std::vector<float> dense(requests.size() * nClusters, 0.0F);
        std::vector<std::uint8_t> observed(requests.size() * nClusters, 0);
        for (std::size_t b0 = 0; b0 < scoring.size();) {
            // one call holds requests of one maxRoutingRepresentatives
            const auto limitOf = [&](std::size_t i) {
                return static_cast<std::uint32_t>(std::min<std::size_t>(requests[i].maxRoutingRepresentatives, 0x10000u));
            };
            std::size_t b1 = b0 + 1;
            while (b1 < scoring.size() && b1 - b0 < YAMS_ROUTE_MAX_QUERIES && limitOf(scoring[b1]) == limitOf(scoring[b0])) ++b1;
            const std::size_t m = b1 - b0;
            std::vector<float> queries(m * dim_);
            std::vector<std::uint32_t> candidates(m * words, 0u);
            for (std::size_t j = 0; j < m; ++j) {
                const std::size_t i = scoring[b0 + j];
                std::copy(requests[i].queryEmbedding.begin(), requests[i].queryEmbedding.end(), queries.begin() + j * dim_);
                for (std::size_t c = 0; c < nClusters; ++c)
                    if (pending[i].routeCandidates[c]) candidates[j * words + c / 32] |= 1u << (c % 32);
            }
            std::vector<float> d(m * nClusters);
            std::vector<std::uint8_t> o(m * nClusters);
            std::vector<std::uint32_t> evals(m);
            const yams_status_t st = vt_->dense(vt_->self, id_, queries.data(), static_cast<std::uint32_t>(m), limitOf(scoring[b0]), candidates.data(),
                                                d.data(), o.data(), evals.data(), nullptr);
            for (std::size_t j = 0; j < m; ++j) {
                const std::size_t i = scoring[b0 + j];
                if (st != YAMS_OK) {
                    out[i] = Error{accel::mapStatus(st), "topology_route_v1.dense refused the call"};
                    pending[i].failed = true;
                    continue;
                }
                std::copy(d.begin() + j * nClusters, d.begin() + (j + 1) * nClusters, dense.begin() + i * nClusters);
                std::copy(o.begin() + j * nClusters, o.begin() + (j + 1) * nClusters, observed.begin() + i * nClusters);
                Work* work = i < works.size() ? works[i] : nullptr;
                if (work != nullptr) {
                    work->representativeDistanceEvaluations += evals[j];
                    work->exactRepresentativeDistanceEvaluations += evals[j];
                }
            }
            b0 = b1;
        }

        // :922-980
        for (std::size_t i = 0; i < requests.size(); ++i) {
            const Request& request = requests[i];
            const Pending& p = pending[i];
            if (p.failed) continue;
            const float alpha = p.alpha;
            std::vector<Route> routes;
            routes.reserve(nClusters);
            for (std::size_t c = 0; c < nClusters; ++c) {
                if (!p.routeCandidates[c]) continue;
                const auto& cluster = artifacts.clusters[c];
                const float denseSignal = dense[i * nClusters + c];
                const bool denseObserved = observed[i * nClusters + c] != 0;
                const float sparseNorm = p.maxSparseMass > 0.0 ? static_cast<float>(p.sparseMass[c] / p.maxSparseMass) : 0.0F;
                const double blended = static_cast<double>(alpha * sparseNorm + (1.0F - alpha) * denseSignal);
                const double cohesion = std::clamp(cluster.cohesionScore, 0.0, 1.0);
                const double stability = std::clamp(cluster.persistenceScore, 0.0, 1.0);
                const double sizeDamp = 1.0 / (1.0 + std::log1p(static_cast<double>(cluster.memberCount)));
                double routeScore = blended + (cluster.persistenceScore * 0.05);
                if (request.scoringMode == Mode::SizeWeighted) {
                    routeScore = (blended + (0.05 * stability) + (0.05 * cohesion)) * sizeDamp;
                } else if (request.scoringMode == Mode::SeedCoverage) {
                    routeScore = static_cast<double>(sparseNorm) + (0.10 * denseSignal) + (cluster.persistenceScore * 0.05);
                }
                Route route{};
                route.clusterId = cluster.clusterId;
                route.medoidDocumentHash = cluster.medoid.has_value() ? std::optional<std::string>(cluster.medoid->documentHash) : std::nullopt;
                route.routeScore = routeScore;
                route.stabilityScore = cluster.persistenceScore;
                route.memberCount = cluster.memberCount;
                route.semanticCost = denseObserved ? std::optional<double>(1.0 - static_cast<double>(denseSignal)) : std::nullopt;
                route.sparseCost = p.maxSparseMass > 0.0 ? std::optional<double>(1.0 - static_cast<double>(sparseNorm)) : std::nullopt;
                route.persistencePenalty = 1.0 - stability;
                route.cohesionPenalty = 1.0 - cohesion;
                route.sizePenalty = 1.0 - sizeDamp;
                routes.push_back(std::move(route));
            }
            std::sort(routes.begin(), routes.end(), [](const Route& lhs, const Route& rhs) {
                if (lhs.routeScore != rhs.routeScore) return lhs.routeScore > rhs.routeScore;
                return lhs.clusterId < rhs.clusterId;
            });
            if (request.limit > 0 && routes.size() > request.limit) routes.resize(request.limit);
            out[i] = std::move(routes);
        }
        return out;
    }

private:
    AccelClusterRouter(std::shared_ptr<accel::Plugin> p, yams_topology_route_v1* vt) : plugin_(std::move(p)), vt_(vt) {}
    void drop() {
        if (live_) (void)vt_->index_destroy(vt_->self, id_);
        live_ = false;
    }
    std::shared_ptr<accel::Plugin> plugin_;
    yams_topology_route_v1* vt_;
    std::uint64_t id_ = 0;
    bool live_ = false;
    std::size_t dim_ = 0, clusters_ = 0;
};

} // namespace yams::topology
