// topology_sgc.hpp — applySGCSmoothing of the topology build (src/topology/topology_sgc.cpp:23-179 in the reference, header
// include/yams/topology/topology_sgc.h) with the degree pass and the hop loop on the device (plugin interface
// topology_smooth_v1).
//
// AccelSGC::apply does on the host what the reference does around the loop:
//   :25-50    hops == 0, fewer than two documents, or no non-empty embedding: nothing changes; dim = the size of the first
//             non-empty embedding
//   :52-58    hash -> index; a later document overwrites an earlier one of the same hash
//   :60-84    admission, in the order of documents[i].neighbors: skipped are an empty or unknown hash, j == i, a
//             non-reciprocal neighbour under reciprocalOnly, score < float(minEdgeScore); weight = max(0.0f, score)
//   :86-112   symmetrisation: key (max(i, j) << 32) | min(i, j) in a std::unordered_map<uint64_t, float> reserved to n * 4;
//             the first sighting is emplaced, later ones keep the larger weight; then, for each entry IN ITERATION ORDER,
//             (hi, w) is appended to the list of lo and (lo, w) to the list of hi
//   :130-137  the n x dim matrix; a document whose embedding has another size is a row of +0.0f, which STAYS in the matrix
//             (as a neighbour it adds +0.0f: a -0.0f accumulator becomes +0.0f) ...
//   :163-168  ... and is never written back
// and hands matrix and lists, packed, to topology_smooth_v1.smooth, whose result equals the CPU loop's bit for bit.
//
// THE ORDER OF A LIST IS A PROPERTY OF THE HOST'S STANDARD LIBRARY.  Every output element is an fp32 chain over the row's
// list in list order, and that order is the iteration order of the unordered_map above: it depends on the library's hash of
// uint64_t, its bucket policy and its growth.  That is why this shell — compiled IN the host, with the host's library —
// builds the lists with the same container type, the same reserve and the same sequence of insertions, and why the device
// takes the order as an input and keeps it.  AccelSGC::buildLists exposes the lists for tests.
// A refusal of the plugin (YAMS_ERR_UNSUPPORTED beyond the limits, INVALID_ARG for non-finite embeddings or scores) comes
// back as an Error and `documents` is untouched: the host then runs its own loop.
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "plugin.hpp"
#ifdef YAMS_ACCEL_USE_HOST_TYPES
#include <yams/topology/topology_artifacts.h> // the host's own TopologyDocumentInput / TopologyNeighbor / TopologyBuildConfig
#endif

namespace yams::topology {

#ifndef YAMS_ACCEL_USE_HOST_TYPES
// this repository's own small types for builds outside the YAMS tree: the fields the smoothing reads or writes
struct TopologyNeighbor {
    std::string documentHash;
    float score{0.0F};
    bool reciprocal{false};
};
struct TopologyDocumentInput {
    std::string documentHash;
    std::vector<float> embedding;
    std::vector<TopologyNeighbor> neighbors;
};
struct TopologyBuildConfig {
    double minEdgeScore{0.0};
    bool reciprocalOnly{true};
};
#endif

// The symmetrised neighbour lists in compressed rows: row i's edges are [rowOffsets[i], rowOffsets[i + 1]), in sum order.
struct SGCLists {
    std::vector<std::uint64_t> rowOffsets;   // [n + 1]
    std::vector<std::uint32_t> cols;
    std::vector<float> weights;
};

class AccelSGC {
public:
    static Result<std::unique_ptr<AccelSGC>> create(std::shared_ptr<accel::Plugin> plugin) {
        auto vt = plugin->getInterface<yams_topology_smooth_v1>(YAMS_IFACE_TOPOLOGY_SMOOTH_V1, YAMS_IFACE_TOPOLOGY_SMOOTH_V1_VERSION);
        if (!vt.has_value()) return vt.error();
        return std::unique_ptr<AccelSGC>(new AccelSGC(std::move(plugin), vt.value()));
    }
    // Over a table the caller owns (a host that binds the interface itself).
    static std::unique_ptr<AccelSGC> over(yams_topology_smooth_v1* vt) { return std::unique_ptr<AccelSGC>(new AccelSGC(nullptr, vt)); }

    // Steps :52-112: admission and symmetrisation.  n = documents.size() must be below 2^32 (the key holds two 32-bit halves).
    static SGCLists buildLists(const std::vector<TopologyDocumentInput>& documents, const TopologyBuildConfig& config) {
        const std::size_t n = documents.size();
        std::unordered_map<std::string, std::size_t> indexOf;
        indexOf.reserve(n);
        for (std::size_t i = 0; i < n; ++i)
            if (!documents[i].documentHash.empty()) indexOf[documents[i].documentHash] = i;      // the later document wins

        // the pairs in the order the reference meets them, the order of the map's insertions
        std::unordered_map<std::uint64_t, float> best;
        best.reserve(n * 4);
        const float floorScore = static_cast<float>(config.minEdgeScore);
        for (std::size_t i = 0; i < n; ++i) {
            for (const auto& nb : documents[i].neighbors) {
                if (nb.documentHash.empty()) continue;
                const auto found = indexOf.find(nb.documentHash);
                if (found == indexOf.end()) continue;
                const std::size_t j = found->second;
                if (j == i) continue;
                if (config.reciprocalOnly && !nb.reciprocal) continue;
                if (nb.score < floorScore) continue;      // (a NaN score passes: every comparison with it is false)
                const float w = std::max(0.0F, nb.score);   // (and becomes weight 0: max returns its first argument)
                const std::uint64_t lo = std::min(i, j), hi = std::max(i, j);
                const std::uint64_t pair = (hi << 32U) | lo;
                auto seen = best.find(pair);
                if (seen == best.end()) best.emplace(pair, w);
                else seen->second = std::max(seen->second, w);
            }
        }
        // two passes over the map in its iteration order: the counts, then the fill — the order within a row is the order
        // in which push_back would have met the entries
        SGCLists lists;
        lists.rowOffsets.assign(n + 1, 0);
        for (const auto& [pair, w] : best) {
            (void)w;
            ++lists.rowOffsets[(pair & 0xFFFFFFFFU) + 1];
            ++lists.rowOffsets[(pair >> 32U) + 1];
        }
        for (std::size_t i = 0; i < n; ++i) lists.rowOffsets[i + 1] += lists.rowOffsets[i];
        lists.cols.resize(lists.rowOffsets[n]);
        lists.weights.resize(lists.rowOffsets[n]);
        std::vector<std::uint64_t> cursor(lists.rowOffsets.begin(), lists.rowOffsets.end() - 1);
        for (const auto& [pair, w] : best) {
            const std::uint64_t lo = pair & 0xFFFFFFFFU, hi = pair >> 32U;
            lists.cols[cursor[lo]] = static_cast<std::uint32_t>(hi); lists.weights[cursor[lo]++] = w;
            lists.cols[cursor[hi]] = static_cast<std::uint32_t>(lo); lists.weights[cursor[hi]++] = w;
        }
        return lists;
    }

    // applySGCSmoothing(documents, config, hops) with the loop on the device.  On an Error `documents` is unchanged.
    Result<void> apply(std::vector<TopologyDocumentInput>& documents, const TopologyBuildConfig& config, std::size_t hops) const {
        const std::size_t n = documents.size();
        if (hops == 0 || n < 2) return Result<void>();
        std::size_t dim = 0;
        for (const auto& doc : documents)
            if (!doc.embedding.empty()) { dim = doc.embedding.size(); break; }
        if (dim == 0) return Result<void>();
        if (n >= (1ull << 31) || dim > UINT32_MAX || hops > UINT32_MAX)
            return Error{ErrorCode::NotImplemented, "SGC arguments beyond the accelerator's range"};
        const SGCLists lists = buildLists(documents, config);
        std::vector<float> packed(n * dim, 0.0F);      // a row of another size stays +0.0f
        for (std::size_t i = 0; i < n; ++i)
            if (documents[i].embedding.size() == dim) std::copy(documents[i].embedding.begin(), documents[i].embedding.end(), packed.begin() + i * dim);
        std::vector<float> smoothed(n * dim);
        yams_sgc_diag_t diag{};
        const yams_status_t st = vt_->smooth(vt_->self, packed.data(), n, static_cast<std::uint32_t>(dim), lists.rowOffsets.data(),
                                             lists.cols.data(), lists.weights.data(), static_cast<std::uint32_t>(hops), smoothed.data(), &diag);
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_smooth_v1.smooth refused the call"};
        lastDiag_ = diag;
        for (std::size_t i = 0; i < n; ++i)
            if (documents[i].embedding.size() == dim) std::copy(smoothed.begin() + i * dim, smoothed.begin() + (i + 1) * dim, documents[i].embedding.begin());
        return Result<void>();
    }

    const yams_sgc_diag_t& lastDiag() const { return lastDiag_; }

private:
    AccelSGC(std::shared_ptr<accel::Plugin> p, yams_topology_smooth_v1* vt) : plugin_(std::move(p)), vt_(vt) {}
    std::shared_ptr<accel::Plugin> plugin_;
    yams_topology_smooth_v1* vt_;
    mutable yams_sgc_diag_t lastDiag_{};
};

} // namespace yams::topology
