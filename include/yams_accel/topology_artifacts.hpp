// topology_artifacts.hpp — the two public functions of include/yams/topology/topology_representatives.h in the reference
// (selectDiverseRoutingRepresentatives, applyOrthogonalBoundarySpill; src/topology/topology_representatives.cpp:33-91, :93-287)
// and detail::meanEmbedding (src/topology/topology_build_utils.h:27-56) with their array arithmetic on the device (plugin
// interface topology_artifacts_v1).
//
// What stays on the host, here, line for line:
//   meanEmbedding        the first non-empty member fixes the size, members of another size are skipped (h:31-41)
//   representatives      the early returns (:37), admission (:43-53: index in range, hash non-empty, the centroid's size, all
//                        elements finite), the sort by hash (:54-56), the copies of hash and embedding (:85-88)
//   boundary spill       the early return (:96-101), the hash maps (:103-116: the FIRST document / cluster of a key wins, as
//                        emplace leaves it), the observedRadiusSquared maximum (:119-141), the admission tests and `loss`
//                        (:196-262), the sort (:264-270: its comparator |d| > 1e-12 is not a strict weak order, so its result
//                        belongs to this host's std::sort), the member-list edits (:272-284)
// What the device computes: the selection loop (:58-90) and the three chains radiusSquared / primaryNormSquared /
// candidateNormSquared + residualDot (:128-135, :189-195, :235-242).
//
// THE RESIDUAL FORM IS A PROPERTY OF THE HOST'S BUILD.  The products of those chains are not exact in fp64, so the bits depend
// on whether the host's compiler contracted `x += a * b` into an fma (aarch64 with the default -ffp-contract does; x86-64
// without -mfma does not).  probeResidualForm() asks the host's OWN applyOrthogonalBoundarySpill on crafted cases (the model is
// l2_calibration.hpp) and reports which of the two forms the device offers reproduces it; a host whose answers match neither
// gets an Error and runs its own loop.
//
// The candidate clusters of a document come from a callable (CandidateSource): a host that has its centroid ANN index passes
// the hits of centroidAnnIndex->search(embedding, overlapCandidateLimit) (:205-213); an empty answer — and no callable — means
// every cluster in index order (:214-220), which the device serves from its dense mode when no document has a list.
//
// The functions are templates over the host's own types (TopologyDocumentInput, TopologyBuildConfig, TopologyArtifactBatch,
// ClusterRoutingRepresentative): they read and write the fields the reference's functions do, by name.
// A refusal of the plugin comes back as an Error and nothing is changed: the host then runs its own function.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <span>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "plugin.hpp"

namespace yams::topology {

enum class ResidualForm : std::uint32_t { Separate = YAMS_RESIDUAL_SEPARATE, Fused = YAMS_RESIDUAL_FUSED };

// The candidate clusters of one document (indices into artifacts.clusters, any order); empty = every cluster.
using CandidateSource = std::function<std::vector<std::size_t>(std::span<const float> embedding, std::size_t limit)>;

namespace artifact_probe {
// Two independent cases, found by a CPU search with an exact fma.  One document e = (1, 1); primary centroid (p0, p1),
// candidate centroid (p1, p0): the candidate's residuals are the primary's, swapped.  Unfused, both sums are
// round(round(x^2) + round(y^2)): equal, the candidate is admitted (ratio 1.0, penalty 0.0) and the function returns 1.
// Fused, candidateNormSquared = fma(x, x, round(y^2)) exceeds primaryNormSquared = fma(y, y, round(x^2)) by one ulp
// (case 0: 0x1.ffffff1e927c2p+0 against ...c1p+0; case 1: 0x1.ffffff18e317ap+0 against ...79p+0): rejected, 0.
inline constexpr std::uint32_t kCentroidBits[2][2] = {{0x32500321u, 0x3272d7e7u}, {0x324fa392u, 0x327e963fu}};
inline float fromBits(std::uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
} // namespace artifact_probe

class AccelArtifacts {
public:
    static Result<std::unique_ptr<AccelArtifacts>> create(std::shared_ptr<accel::Plugin> plugin, ResidualForm form) {
        auto vt = plugin->getInterface<yams_topology_artifacts_v1>(YAMS_IFACE_TOPOLOGY_ARTIFACTS_V1, YAMS_IFACE_TOPOLOGY_ARTIFACTS_V1_VERSION);
        if (!vt.has_value()) return vt.error();
        return std::unique_ptr<AccelArtifacts>(new AccelArtifacts(std::move(plugin), vt.value(), form));
    }
    // Over a table the caller owns (a host that binds the interface itself).
    static std::unique_ptr<AccelArtifacts> over(yams_topology_artifacts_v1* vt, ResidualForm form) {
        return std::unique_ptr<AccelArtifacts>(new AccelArtifacts(nullptr, vt, form));
    }
    ResidualForm form() const { return form_; }

    // Which form is the host's own applyOrthogonalBoundarySpill?  hostSpill(documents, config, artifacts) is that function.
    template <class Document, class Config, class Batch, class HostSpill>
    static Result<ResidualForm> probeResidualForm(HostSpill&& hostSpill) {
        std::size_t answers[2];
        for (int k = 0; k < 2; ++k) {
            const float p0 = artifact_probe::fromBits(artifact_probe::kCentroidBits[k][0]);
            const float p1 = artifact_probe::fromBits(artifact_probe::kCentroidBits[k][1]);
            std::vector<Document> docs(2);
            docs[0].documentHash = "probe-a"; docs[0].embedding = {1.0F, 1.0F};
            docs[1].documentHash = "probe-b"; docs[1].embedding = {p1, p0};      // the candidate's own member, at its centroid
            Config config{};
            config.allowOverlap = true;
            config.overlapLimit = 1;
            config.overlapBoundaryDistanceRatio = 1.0;
            config.overlapResidualPenalty = 0.0;
            Batch batch{};
            batch.clusters.resize(2);
            batch.clusters[0].clusterId = "probe-primary"; batch.clusters[0].centroidEmbedding = {p0, p1};
            batch.clusters[0].memberDocumentHashes = {"probe-a"}; batch.clusters[0].memberCount = 1;
            batch.clusters[1].clusterId = "probe-candidate"; batch.clusters[1].centroidEmbedding = {p1, p0};
            batch.clusters[1].memberDocumentHashes = {"probe-b"}; batch.clusters[1].memberCount = 1;
            batch.memberships.resize(1);
            batch.memberships[0].documentHash = "probe-a"; batch.memberships[0].clusterId = "probe-primary";
            answers[k] = hostSpill(std::span<const Document>(docs), config, batch);
        }
        if (answers[0] == 1 && answers[1] == 1) return ResidualForm::Separate;
        if (answers[0] == 0 && answers[1] == 0) return ResidualForm::Fused;
        return Error{ErrorCode::NotSupported, "the host's applyOrthogonalBoundarySpill matches neither residual form"};
    }

    // detail::meanEmbedding(documents, members).  Empty when no member counts.
    template <class Document>
    Result<std::vector<float>> meanEmbedding(std::span<const Document> documents, const std::vector<std::size_t>& members) const {
        std::size_t dim = 0;
        std::vector<float> packed;
        std::uint32_t count = 0;
        for (const std::size_t index : members) {
            if (index >= documents.size() || documents[index].embedding.empty()) continue;
            const auto& e = documents[index].embedding;
            if (dim == 0) dim = e.size();
            else if (e.size() != dim) continue;
            packed.insert(packed.end(), e.begin(), e.end());
            ++count;
        }
        if (count == 0) return std::vector<float>{};
        if (dim > UINT32_MAX) return Error{ErrorCode::NotImplemented, "dimension beyond the accelerator's range"};
        std::vector<std::uint32_t> list(count);
        for (std::uint32_t i = 0; i < count; ++i) list[i] = i;
        const std::uint64_t off[2] = {0, count};
        float* cent = nullptr; std::uint32_t* cnt = nullptr;
        const yams_status_t st = vt_->centroids(vt_->self, packed.data(), count, static_cast<std::uint32_t>(dim), off, list.data(), 1, &cent, &cnt);
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_artifacts_v1.centroids refused the call"};
        std::vector<float> out(cent, cent + dim);
        vt_->free_centroids(vt_->self, cent, cnt);
        return out;
    }

    // selectDiverseRoutingRepresentatives(documents, members, centroidEmbedding, routingRepresentativeCount)
    template <class Representative, class Document>
    Result<std::vector<Representative>> selectDiverseRoutingRepresentatives(std::span<const Document> documents,
                                                                            std::span<const std::size_t> members,
                                                                            std::span<const float> centroidEmbedding,
                                                                            std::size_t routingRepresentativeCount) const {
        std::vector<Representative> selected;
        if (routingRepresentativeCount <= 1 || centroidEmbedding.empty()) return selected;
        std::vector<std::size_t> candidates;
        candidates.reserve(members.size());
        for (const auto member : members) {
            if (member >= documents.size() || documents[member].documentHash.empty() ||
                documents[member].embedding.size() != centroidEmbedding.size())
                continue;
            if (std::all_of(documents[member].embedding.begin(), documents[member].embedding.end(), [](float v) { return std::isfinite(v); }))
                candidates.push_back(member);
        }
        std::sort(candidates.begin(), candidates.end(),
                  [&](std::size_t lhs, std::size_t rhs) { return documents[lhs].documentHash < documents[rhs].documentHash; });
        const std::size_t extra = routingRepresentativeCount - 1;
        if (candidates.empty()) return selected;
        if (extra > YAMS_CLUSTER_MAX_REPRESENTATIVES || centroidEmbedding.size() > UINT32_MAX || candidates.size() >= (1ull << 31))
            return Error{ErrorCode::NotImplemented, "representatives beyond the accelerator's range"};
        const std::size_t dim = centroidEmbedding.size(), m = candidates.size();
        std::vector<float> packed(m * dim);
        std::vector<std::uint32_t> list(m);
        for (std::size_t i = 0; i < m; ++i) {
            std::copy(documents[candidates[i]].embedding.begin(), documents[candidates[i]].embedding.end(), packed.begin() + i * dim);
            list[i] = static_cast<std::uint32_t>(i);
        }
        const std::uint64_t off[2] = {0, m};
        std::uint32_t* sel = nullptr; std::uint32_t* cnt = nullptr;
        const yams_status_t st = vt_->representatives(vt_->self, packed.data(), m, static_cast<std::uint32_t>(dim), off, list.data(),
                                                      centroidEmbedding.data(), nullptr, 1, static_cast<std::uint32_t>(extra), &sel, &cnt);
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_artifacts_v1.representatives refused the call"};
        selected.reserve(cnt[0]);
        for (std::uint32_t s = 0; s < cnt[0]; ++s) {
            const auto document = candidates[sel[s]];
            Representative r{};
            r.documentHash = documents[document].documentHash;
            r.embedding = documents[document].embedding;
            selected.push_back(std::move(r));
        }
        vt_->free_representatives(vt_->self, sel, cnt);
        return selected;
    }

    // applyOrthogonalBoundarySpill(documents, config, artifacts).  `source` (may be empty) gives a document's candidate
    // clusters.  On an Error `artifacts` is unchanged.
    template <class Document, class Config, class Batch>
    Result<std::size_t> applyOrthogonalBoundarySpill(std::span<const Document> documents, const Config& config, Batch& artifacts,
                                                     const CandidateSource& source = {}) const {
        if (!config.allowOverlap || config.overlapLimit == 0 || artifacts.clusters.size() < 2 ||
            !std::isfinite(config.overlapBoundaryDistanceRatio) || config.overlapBoundaryDistanceRatio < 1.0 ||
            !std::isfinite(config.overlapResidualPenalty) || config.overlapResidualPenalty < 0.0)
            return std::size_t{0};
        const std::size_t nClusters = artifacts.clusters.size();
        std::unordered_map<std::string, const Document*> documentByHash;
        documentByHash.reserve(documents.size());
        for (const auto& document : documents)
            if (!document.documentHash.empty() && !document.embedding.empty()) documentByHash.emplace(document.documentHash, &document);
        std::unordered_map<std::string, std::size_t> clusterIndexById;
        clusterIndexById.reserve(nClusters);
        for (std::size_t index = 0; index < nClusters; ++index)
            if (!artifacts.clusters[index].clusterId.empty()) clusterIndexById.emplace(artifacts.clusters[index].clusterId, index);

        // One matrix for the device: the dimension of the first non-empty centroid; centroids and documents of another size
        // take no part in any chain the reference would compute against a centroid of THIS size.  A batch whose centroids have
        // several sizes is not served (the reference pairs each document with the centroids of its own size).
        std::size_t dim = 0;
        for (const auto& cluster : artifacts.clusters) {
            if (cluster.centroidEmbedding.empty()) continue;
            if (dim == 0) dim = cluster.centroidEmbedding.size();
            else if (cluster.centroidEmbedding.size() != dim) return Error{ErrorCode::NotImplemented, "centroids of several sizes"};
        }
        if (dim == 0) return std::size_t{0};      // every pairing fails `embedding.size() != centroid.size() || embedding.empty()`
        if (dim > YAMS_CLUSTER_MAX_DIM || nClusters > YAMS_CLUSTER_MAX_K) return Error{ErrorCode::NotImplemented, "beyond the accelerator's range"};
        std::vector<float> cents(nClusters * dim, 0.0F);
        for (std::size_t c = 0; c < nClusters; ++c)
            if (!artifacts.clusters[c].centroidEmbedding.empty())
                std::copy(artifacts.clusters[c].centroidEmbedding.begin(), artifacts.clusters[c].centroidEmbedding.end(), cents.begin() + c * dim);
        constexpr double kResidualEpsilon = 1e-12;
        const std::uint32_t form = static_cast<std::uint32_t>(form_);

        // ---- the radius pass (:119-141): one pair per (cluster, member) whose sizes agree
        std::vector<double> observedRadiusSquared(nClusters, 0.0);
        {
            std::vector<float> rows;
            std::vector<std::uint64_t> off{0};
            std::vector<std::uint32_t> cand;
            for (std::size_t c = 0; c < nClusters; ++c) {
                const auto& cluster = artifacts.clusters[c];
                if (cluster.centroidEmbedding.empty()) continue;      // (an empty centroid: the loop adds nothing, radius stays 0 — and a
                for (const auto& hash : cluster.memberDocumentHashes) {      //  document of size 0 is not in documentByHash)
                    const auto it = documentByHash.find(hash);
                    if (it == documentByHash.end() || it->second->embedding.size() != dim) continue;
                    rows.insert(rows.end(), it->second->embedding.begin(), it->second->embedding.end());
                    cand.push_back(static_cast<std::uint32_t>(c));
                    off.push_back(cand.size());
                }
            }
            if (!cand.empty()) {
                double* pn = nullptr; double* cn = nullptr; double* rd = nullptr;
                const yams_status_t st = vt_->residuals(vt_->self, rows.data(), cand.size(), static_cast<std::uint32_t>(dim), cents.data(),
                                                        static_cast<std::uint32_t>(nClusters), nullptr, off.data(), cand.data(), form, &pn, &cn, &rd);
                if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_artifacts_v1.residuals refused the radius pass"};
                for (std::size_t i = 0; i < cand.size(); ++i)
                    if (std::isfinite(cn[i])) observedRadiusSquared[cand[i]] = std::max(observedRadiusSquared[cand[i]], cn[i]);
                vt_->free_residuals(vt_->self, pn, cn, rd);
            }
        }
        constexpr std::size_t kMinimumOverlapCandidateLimit = 32;
        const auto overlapCandidateLimit =
            std::max({kMinimumOverlapCandidateLimit, static_cast<std::size_t>(config.maxNeighborsPerDocument), static_cast<std::size_t>(config.overlapLimit) + 1});

        // ---- the memberships that reach the chains (:174-187), their candidates (:204-220)
        struct Row { std::size_t membership; std::size_t primary; const Document* document; };
        std::vector<Row> live;
        std::vector<std::vector<std::size_t>> lists;
        bool anyList = false;
        for (std::size_t mi = 0; mi < artifacts.memberships.size(); ++mi) {
            const auto& membership = artifacts.memberships[mi];
            if (!membership.overlapClusterIds.empty()) continue;
            const auto documentIt = documentByHash.find(membership.documentHash);
            const auto primaryIt = clusterIndexById.find(membership.clusterId);
            if (documentIt == documentByHash.end() || primaryIt == clusterIndexById.end()) continue;
            const auto& embedding = documentIt->second->embedding;
            if (embedding.size() != artifacts.clusters[primaryIt->second].centroidEmbedding.size() || embedding.empty()) continue;
            live.push_back(Row{mi, primaryIt->second, documentIt->second});
            lists.emplace_back(source ? source(std::span<const float>(embedding), overlapCandidateLimit) : std::vector<std::size_t>{});
            anyList = anyList || !lists.back().empty();
        }
        if (live.empty()) return std::size_t{0};
        std::vector<float> rows(live.size() * dim);
        std::vector<std::uint32_t> primary(live.size());
        for (std::size_t i = 0; i < live.size(); ++i) {
            std::copy(live[i].document->embedding.begin(), live[i].document->embedding.end(), rows.begin() + i * dim);
            primary[i] = static_cast<std::uint32_t>(live[i].primary);
        }
        // the chains are computed for the candidates with a centroid of this size (:225-234); the others are skipped below
        std::vector<std::uint64_t> off;
        std::vector<std::uint32_t> cand;
        if (anyList) {
            off.push_back(0);
            for (auto& list : lists) {
                if (list.empty()) { list.resize(nClusters); for (std::size_t c = 0; c < nClusters; ++c) list[c] = c; }
                for (const auto c : list)
                    cand.push_back(c < nClusters ? static_cast<std::uint32_t>(c) : static_cast<std::uint32_t>(live[off.size() - 1].primary));
                off.push_back(cand.size());      // (an index out of range is skipped below (:225); it travels as the primary, also skipped)
            }
        }
        double* pn = nullptr; double* cn = nullptr; double* rd = nullptr;
        const yams_status_t st = vt_->residuals(vt_->self, rows.data(), live.size(), static_cast<std::uint32_t>(dim), cents.data(),
                                                static_cast<std::uint32_t>(nClusters), primary.data(), anyList ? off.data() : nullptr,
                                                anyList ? cand.data() : nullptr, form, &pn, &cn, &rd);
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_artifacts_v1.residuals refused the call"};

        // ---- admission, loss, sort, member-list edits (:196-284), in membership order
        struct Candidate { std::size_t clusterIndex{0}; double loss{0.0}; };
        std::size_t assignments = 0;
        const double boundaryRatioSquared = config.overlapBoundaryDistanceRatio * config.overlapBoundaryDistanceRatio;
        for (std::size_t i = 0; i < live.size(); ++i) {
            auto& membership = artifacts.memberships[live[i].membership];
            using Role = std::remove_cv_t<std::remove_reference_t<decltype(membership.role)>>;
            const double primaryNormSquared = pn[i];
            if (!std::isfinite(primaryNormSquared)) continue;
            const bool primaryDirectionObserved = primaryNormSquared > kResidualEpsilon;
            if (!primaryDirectionObserved && membership.role != Role::Outlier) continue;
            const std::size_t base = anyList ? off[i] : i * nClusters, count = anyList ? off[i + 1] - off[i] : nClusters;
            std::vector<Candidate> candidates;
            candidates.reserve(count);
            for (std::size_t j = 0; j < count; ++j) {
                const std::size_t clusterIndex = anyList ? lists[i][j] : j;
                if (clusterIndex >= nClusters || clusterIndex == live[i].primary) continue;
                if (artifacts.clusters[clusterIndex].centroidEmbedding.size() != dim) continue;
                const double candidateNormSquared = cn[base + j], residualDot = rd[base + j];
                if (!std::isfinite(candidateNormSquared)) continue;
                double loss = candidateNormSquared;
                if (primaryDirectionObserved) {
                    if (candidateNormSquared > primaryNormSquared * boundaryRatioSquared) continue;
                    const double projectionSquared = (residualDot * residualDot) / primaryNormSquared;
                    loss += config.overlapResidualPenalty * projectionSquared;
                } else {
                    const double candidateRadiusSquared = observedRadiusSquared[clusterIndex];
                    if (candidateRadiusSquared <= kResidualEpsilon || candidateNormSquared > candidateRadiusSquared * boundaryRatioSquared) continue;
                }
                if (std::isfinite(loss)) candidates.push_back(Candidate{clusterIndex, loss});
            }
            std::sort(candidates.begin(), candidates.end(), [&](const Candidate& lhs, const Candidate& rhs) {
                if (std::abs(lhs.loss - rhs.loss) > kResidualEpsilon) return lhs.loss < rhs.loss;
                return artifacts.clusters[lhs.clusterIndex].clusterId < artifacts.clusters[rhs.clusterIndex].clusterId;
            });
            const auto limit = std::min<std::size_t>(config.overlapLimit, candidates.size());
            membership.overlapClusterIds.reserve(limit);
            for (std::size_t k = 0; k < limit; ++k) {
                auto& secondary = artifacts.clusters[candidates[k].clusterIndex];
                if (std::find(secondary.memberDocumentHashes.begin(), secondary.memberDocumentHashes.end(), membership.documentHash) ==
                    secondary.memberDocumentHashes.end()) {
                    secondary.memberDocumentHashes.push_back(membership.documentHash);
                    std::sort(secondary.memberDocumentHashes.begin(), secondary.memberDocumentHashes.end());
                    secondary.memberCount = secondary.memberDocumentHashes.size();
                }
                membership.overlapClusterIds.push_back(secondary.clusterId);
                ++assignments;
            }
        }
        vt_->free_residuals(vt_->self, pn, cn, rd);
        return assignments;
    }

private:
    AccelArtifacts(std::shared_ptr<accel::Plugin> p, yams_topology_artifacts_v1* vt, ResidualForm form)
        : plugin_(std::move(p)), vt_(vt), form_(form) {}
    std::shared_ptr<accel::Plugin> plugin_;
    yams_topology_artifacts_v1* vt_;
    ResidualForm form_;
};

} // namespace yams::topology
