// semantic_graph.hpp — the semantic-neighbour graph of EmbeddingService::updateSemanticNeighborGraphUnlocked
// (src/daemon/components/EmbeddingService.cpp in the reference) with the N^2 * D pair loop on the device (plugin interface
// semantic_graph_v1).
//
// AccelSemanticGraph::build does on the host what the reference does around the loop:
//   :865-870    records with an empty hash or an empty embedding are skipped; the FIRST record of a hash wins
//   :875-878    rows whose inverse norm is <= 0 leave the corpus (the device does that: it computes the norms)
//   :398        an explicit threshold is clamped to [0, 1]
//   :902-918    sources: every corpus row, or the corpus rows whose hash was requested, in corpus order
//   :949-954    ties between equal similarities go to the smaller hash: the ranks of the hashes in std::string order
//   :1018-1019  effective threshold of a source = the explicit one, or its last kept similarity
//   :1042       edge weight = std::clamp(similarity, effectiveThreshold, 1.0f); rank = position + 1 (:1052)
// and emits (source hash, neighbour hash, similarity, weight, rank) in the reference's order: sources in corpus order, each
// source's neighbours best first.  The reverse edge of every tuple, the KG node lookup (a neighbour without a node is skipped
// and does not take a rank, :1032-1036) and the JSON properties stay the host's.
// Embeddings of differing dimensions (the reference scores such a pair 0.0f, :419-421) are not served: NotImplemented.  A
// refusal of the plugin (YAMS_ERR_UNSUPPORTED beyond the limits, INVALID_ARG for non-finite rows) comes back as an Error: the
// host then runs its own loop.
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>
#include <numeric>
#include <optional>
#include <span>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "plugin.hpp"

namespace yams::daemon {

struct SemanticNeighborEdge {
    std::string sourceHash;
    std::string neighborHash;
    float similarity = 0.0f;
    float weight = 0.0f;
    std::size_t rank = 0;      // 1 = the best neighbour of its source
};

struct SemanticGraphResult {
    std::vector<SemanticNeighborEdge> edges;
    std::size_t similarityPairCount = 0;
    std::size_t candidateNeighborCount = 0;
    float minEffectiveThreshold = 1.0f;      // (:963-964, :1020-1021)
    float maxEffectiveThreshold = 0.0f;
    std::vector<std::string> corpusHashes;   // the de-duplicated records, in stream order ...
    std::vector<float> invNorm;              // ... and their inverse norms (0 = not part of the corpus)
};

class AccelSemanticGraph {
public:
    static Result<std::unique_ptr<AccelSemanticGraph>> create(std::shared_ptr<accel::Plugin> plugin) {
        auto vt = plugin->getInterface<yams_semantic_graph_v1>(YAMS_IFACE_SEMANTIC_GRAPH_V1, YAMS_IFACE_SEMANTIC_GRAPH_V1_VERSION);
        if (!vt.has_value()) return vt.error();
        return std::unique_ptr<AccelSemanticGraph>(new AccelSemanticGraph(std::move(plugin), vt.value()));
    }
    // Over a table the caller owns (a host that binds the interface itself).
    static std::unique_ptr<AccelSemanticGraph> over(yams_semantic_graph_v1* vt) {
        return std::unique_ptr<AccelSemanticGraph>(new AccelSemanticGraph(nullptr, vt));
    }

    // hashes[i] / embeddings[i] = document_hash / embedding of the i-th document-level record in stream order.
    // sourceHashes == nullopt: every corpus row is a source (sourceAllCorpus).
    Result<SemanticGraphResult> build(std::span<const std::string> hashes, std::span<const std::vector<float>> embeddings,
                                      const std::optional<std::vector<std::string>>& sourceHashes, std::size_t topK,
                                      std::optional<float> explicitThreshold) const {
        SemanticGraphResult out;
        if (hashes.size() != embeddings.size()) return Error{ErrorCode::InvalidArgument, "one hash per embedding"};
        std::vector<std::size_t> kept;
        std::unordered_set<std::string> seen;
        std::size_t dim = 0;
        for (std::size_t i = 0; i < hashes.size(); ++i) {
            if (hashes[i].empty() || embeddings[i].empty()) continue;
            if (!seen.insert(hashes[i]).second) continue;
            if (dim == 0) dim = embeddings[i].size();
            if (embeddings[i].size() != dim) return Error{ErrorCode::NotImplemented, "embeddings of differing dimensions"};
            kept.push_back(i);
        }
        const std::size_t n = kept.size();
        if (topK > UINT32_MAX || dim > UINT32_MAX) return Error{ErrorCode::NotImplemented, "arguments beyond the accelerator's range"};
        out.corpusHashes.reserve(n);
        for (std::size_t i : kept) out.corpusHashes.push_back(hashes[i]);
        out.invNorm.assign(n, 0.0f);
        if (n == 0) return out;
        std::vector<float> packed(n * dim);
        for (std::size_t u = 0; u < n; ++u) std::copy(embeddings[kept[u]].begin(), embeddings[kept[u]].end(), packed.begin() + u * dim);
        // ranks of the hashes in std::string order
        std::vector<std::uint32_t> order(n), rank(n);
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](std::uint32_t a, std::uint32_t b) { return out.corpusHashes[a] < out.corpusHashes[b]; });
        for (std::size_t r = 0; r < n; ++r) rank[order[r]] = static_cast<std::uint32_t>(r);
        std::vector<std::uint32_t> sources;
        if (sourceHashes.has_value()) {
            std::unordered_set<std::string> requested;
            for (const auto& h : *sourceHashes)
                if (!h.empty()) requested.insert(h);
            for (std::size_t u = 0; u < n; ++u)
                if (requested.count(out.corpusHashes[u])) sources.push_back(static_cast<std::uint32_t>(u));
            if (sources.empty()) return out;
        }
        const std::size_t nSources = sourceHashes.has_value() ? sources.size() : n;
        const bool explicitMode = explicitThreshold.has_value();
        const float threshold = explicitMode ? std::clamp(*explicitThreshold, 0.0f, 1.0f) : 0.0f;
        std::uint32_t* rows = nullptr; float* sims = nullptr; std::uint32_t* counts = nullptr; float* inv = nullptr;
        yams_graph_diag_t diag{};
        const yams_status_t st = vt_->neighbors(vt_->self, packed.data(), n, static_cast<std::uint32_t>(dim), rank.data(),
                                                sourceHashes.has_value() ? sources.data() : nullptr, nSources,
                                                static_cast<std::uint32_t>(topK), explicitMode ? YAMS_GRAPH_FLAG_EXPLICIT_THRESHOLD : 0u,
                                                threshold, &rows, &sims, &counts, &inv, &diag);
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "semantic_graph_v1.neighbors refused the call"};
        out.similarityPairCount = diag.pairs_scored;
        out.candidateNeighborCount = diag.pairs_admitted;
        if (inv) std::copy(inv, inv + n, out.invNorm.begin());
        if (rows) {      // (null arrays: an empty result — fewer than two rows, topK == 0)
            for (std::size_t s = 0; s < nSources; ++s) {
                const std::uint32_t cnt = counts[s];
                if (cnt == 0) continue;
                const std::size_t src = sourceHashes.has_value() ? sources[s] : s;
                const float* ss = sims + s * topK;
                const float effective = explicitMode ? threshold : ss[cnt - 1];
                out.minEffectiveThreshold = std::min(out.minEffectiveThreshold, effective);
                out.maxEffectiveThreshold = std::max(out.maxEffectiveThreshold, effective);
                for (std::uint32_t j = 0; j < cnt; ++j)
                    out.edges.push_back(SemanticNeighborEdge{out.corpusHashes[src], out.corpusHashes[rows[s * topK + j]], ss[j],
                                                             clampAsStd(ss[j], effective, 1.0f), j + 1u});
            }
        }
        vt_->free_neighbors(vt_->self, rows, sims, counts, inv);
        return out;
    }

private:
    // std::clamp's comparisons written out: a last kept similarity one step above 1.0f makes lo > hi, which std::clamp
    // leaves undefined and every implementation answers with lo
    static float clampAsStd(float v, float lo, float hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }
    AccelSemanticGraph(std::shared_ptr<accel::Plugin> p, yams_semantic_graph_v1* vt) : plugin_(std::move(p)), vt_(vt) {}
    std::shared_ptr<accel::Plugin> plugin_;
    yams_semantic_graph_v1* vt_;
};

} // namespace yams::daemon
