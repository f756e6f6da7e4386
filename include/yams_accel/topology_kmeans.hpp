// topology_kmeans.hpp — runKMeans of the topology engine "kmeans_v1" (src/topology/topology_alternate_engines.cpp:341-478 in
// the reference) with the clustering of the usable rows on the device (plugin interface topology_cluster_v1).
//
// AccelKMeans::run reproduces the function's outer shell on the host:
//   :349-361  usable rows: not empty, and of the first non-empty row's dimension
//   :362-365  fewer than two usable rows (or no dimension): assignment = iota
//   :468-477  usable rows carry their cluster; the others become singletons numbered k, k + 1, ... in row order
// and hands the usable rows, packed, to topology_cluster_v1.kmeans, whose result equals the CPU loop's bit for bit.
// The seam is the one call at :669 (`runKMeans(documents, config.kmeansK, config.kmeansMaxIterations)`): what follows it,
// buildBatchFromAssignment, sits in an anonymous namespace of the reference and cannot be called from outside, so a host
// swaps the call, not the engine.  A refusal of the plugin (YAMS_ERR_UNSUPPORTED beyond the documented
// limits, INVALID_ARG for non-finite rows) comes back as an Error: the host then runs its own loop.
#pragma once
#include <cstdint>
#include <memory>
#include <numeric>
#include <span>
#include <vector>

#include "plugin.hpp"

namespace yams::topology {

class AccelKMeans {
public:
    static Result<std::unique_ptr<AccelKMeans>> create(std::shared_ptr<accel::Plugin> plugin) {
        auto vt = plugin->getInterface<yams_topology_cluster_v1>(YAMS_IFACE_TOPOLOGY_CLUSTER_V1, YAMS_IFACE_TOPOLOGY_CLUSTER_V1_VERSION);
        if (!vt.has_value()) return vt.error();
        return std::unique_ptr<AccelKMeans>(new AccelKMeans(std::move(plugin), vt.value()));
    }

    // embeddings[i] = documents[i].embedding.  Returns the per-document cluster assignment of runKMeans.
    Result<std::vector<std::int64_t>> run(std::span<const std::vector<float>> embeddings, std::size_t requestedK,
                                          std::size_t maxIterations) const {
        const std::size_t n = embeddings.size();
        std::vector<std::int64_t> assignment(n, -1);
        if (n == 0) return assignment;
        std::vector<std::size_t> usable;
        usable.reserve(n);
        std::size_t dim = 0;
        for (std::size_t i = 0; i < n; ++i) {
            if (embeddings[i].empty()) continue;
            if (dim == 0) dim = embeddings[i].size();
            if (embeddings[i].size() == dim) usable.push_back(i);
        }
        if (usable.size() < 2 || dim == 0) {
            std::iota(assignment.begin(), assignment.end(), 0);
            return assignment;
        }
        if (requestedK > UINT32_MAX || maxIterations > UINT32_MAX || dim > UINT32_MAX)
            return Error{ErrorCode::NotImplemented, "k-means arguments beyond the accelerator's range"};
        std::vector<float> packed(usable.size() * dim);
        for (std::size_t u = 0; u < usable.size(); ++u)
            std::copy(embeddings[usable[u]].begin(), embeddings[usable[u]].end(), packed.begin() + u * dim);
        std::uint32_t* membership = nullptr;
        std::uint32_t k = 0, iterations = 0;
        const yams_status_t st = vt_->kmeans(vt_->self, packed.data(), usable.size(), static_cast<std::uint32_t>(dim),
                                             static_cast<std::uint32_t>(requestedK), static_cast<std::uint32_t>(maxIterations),
                                             &membership, nullptr, &k, &iterations);
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_cluster_v1.kmeans refused the call"};
        for (std::size_t u = 0; u < usable.size(); ++u) assignment[usable[u]] = static_cast<std::int64_t>(membership[u]);
        vt_->free_clusters(vt_->self, membership, nullptr);
        lastIterations_ = iterations;
        std::int64_t singleton = static_cast<std::int64_t>(k);
        for (std::size_t i = 0; i < n; ++i)
            if (assignment[i] < 0) assignment[i] = singleton++;
        return assignment;
    }

    std::uint32_t lastIterations() const { return lastIterations_; }

private:
    AccelKMeans(std::shared_ptr<accel::Plugin> p, yams_topology_cluster_v1* vt) : plugin_(std::move(p)), vt_(vt) {}
    std::shared_ptr<accel::Plugin> plugin_;
    yams_topology_cluster_v1* vt_;
    mutable std::uint32_t lastIterations_ = 0;
};

} // namespace yams::topology
