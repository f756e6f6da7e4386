// topology_features.hpp — the array arithmetic of TopologyInputExtractor::extract of the reference
// (src/topology/topology_input_extractor.cpp: aggregateEmbedding :397-430, computeVarianceWeights :114-165,
// applyMatryoshkaCoarse :167-187, bucketCountSketch :192-203, composeFeatureVector :344-388) on the device (plugin interface
// topology_features_v1).
//
// What stays on the host, here, line for line:
//   aggregateEmbeddings     the short-circuit on a DOCUMENT-level record (:398-402), the skip of empty records (:407) and of
//                           records whose size differs from the first contributing one (:415).  The device sums the
//                           contributing records in their order.
//   collectVarianceSample   the 4096-row cap of :596-606.
//   computeVarianceWeights  the early returns (:116-122, :134-136), the equal-size filter (:126-127), and THE SELECTION OF THE
//                           KEPT DIMENSIONS: this host's own std::partial_sort with the reference's comparator over the
//                           variances the device returned, then float(sqrt(var)) — so the order of equal variances at the
//                           cut is the host library's, as the reference leaves it.  A NaN among the variances makes that
//                           comparator no strict weak order: nothing is sorted, InvalidArgument comes back.
//   composeFeatureVectors   the conditions of :353-354 (matryoshka on?) and :363-364 (which parts a row has), and of :169-171,
//                           where dense is returned UN-normalised (weights of another size): with both parts off the rows
//                           come back as they are, no call; with a part on the call is NotImplemented (the device entry has
//                           no un-normalised dense view) and the host runs its own function.
//
// THE VARIANCE FORM IS A PROPERTY OF THE HOST'S BUILD.  d = double(e) - mean carries up to 53 bits, so d * d is not exact and
// the bits of `var += d * d` depend on whether the host's compiler contracted it into an fma.  probeVarianceForm() asks the
// host's OWN computeVarianceWeights on recorded samples of three rows and two dimensions whose second column is the first
// reversed — the same residuals in another order, so which of the two variances is the larger is decided in the last place —
// and reports which of the two forms the device offers reproduces its weights; a host whose answers match neither gets an
// Error and runs its own function.
//
// A refusal of the plugin comes back as an Error; the host then runs its own function.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <span>
#include <utility>
#include <vector>

#include "plugin.hpp"

namespace yams::topology {

enum class VarianceForm : std::uint32_t { Separate = YAMS_RESIDUAL_SEPARATE, Fused = YAMS_RESIDUAL_FUSED };

namespace features_probe {
// Three samples of three rows x two dimensions (target 1), found by a CPU search with an exact fma (the restatement the
// tests carry; one draw in about thirty qualifies).  kRows: the bits of the six floats, row after row; kWeights[case][form]: the bits of the two weights
// computeVarianceWeights returns, form 0 = separate multiply and add, form 1 = fma.  The forms keep different dimensions.
inline constexpr int kCases = 3;
inline constexpr std::uint32_t kRows[kCases][6] = {
    {0x426c0000u, 0x44a40000u, 0x455e4000u, 0x455e4000u, 0x44a40000u, 0x426c0000u},
    {0x4574a000u, 0x45201000u, 0x447c4000u, 0x447c4000u, 0x45201000u, 0x4574a000u},
    {0x45c46000u, 0x45fe2000u, 0x44ed0000u, 0x44ed0000u, 0x45fe2000u, 0x45c46000u}};
inline constexpr std::uint32_t kWeights[kCases][2][2] = {{{0x44b4d40cu, 0x00000000u}, {0x00000000u, 0x44b4d40cu}},
                                                         {{0x44945c6eu, 0x00000000u}, {0x00000000u, 0x44945c6eu}},
                                                         {{0x00000000u, 0x45237487u}, {0x45237487u, 0x00000000u}}};
} // namespace features_probe

// One record of a document as aggregateEmbedding sees it (vector::VectorRecord's level and embedding).
struct FeatureRecord {
    bool documentLevel = false;
    std::span<const float> embedding;
};

// FeatureComposition's fields that composeFeatureVector reads.
struct FeatureCompositionView {
    bool enableEntityFusion = false;
    float entityFusionAlpha = 0.25F;
    bool enableMatryoshkaCoarseView = false;
    std::size_t matryoshkaTargetDim = 1024;
    bool enableMinHashSketch = false;
    std::size_t minhashSketchDim = 16;
    float minhashAlpha = 0.10F;
};

class AccelTopologyFeatures {
public:
    static constexpr std::size_t kVarianceSampleCap = 4096;      // :602

    static Result<std::unique_ptr<AccelTopologyFeatures>> create(std::shared_ptr<accel::Plugin> plugin, VarianceForm form) {
        auto vt = plugin->getInterface<yams_topology_features_v1>(YAMS_IFACE_TOPOLOGY_FEATURES_V1, YAMS_IFACE_TOPOLOGY_FEATURES_V1_VERSION);
        if (!vt.has_value()) return vt.error();
        return std::unique_ptr<AccelTopologyFeatures>(new AccelTopologyFeatures(std::move(plugin), vt.value(), form));
    }
    // Over a table the caller owns (a host that binds the interface itself).
    static std::unique_ptr<AccelTopologyFeatures> over(yams_topology_features_v1* vt, VarianceForm form) {
        return std::unique_ptr<AccelTopologyFeatures>(new AccelTopologyFeatures(nullptr, vt, form));
    }
    VarianceForm form() const { return form_; }

    // Which form is the host's own computeVarianceWeights?  hostFn(const std::vector<std::vector<float>>&, std::size_t
    // targetDim) -> std::vector<float> is that function.
    template <class HostVarianceWeights> static Result<VarianceForm> probeVarianceForm(HostVarianceWeights&& hostFn) {
        bool separate = true, fused = true;
        for (int k = 0; k < features_probe::kCases; ++k) {
            std::vector<std::vector<float>> sample(3, std::vector<float>(2));
            for (int r = 0; r < 3; ++r) std::memcpy(sample[r].data(), &features_probe::kRows[k][2 * r], 8);
            const std::vector<float> w = hostFn(sample, std::size_t{1});
            std::uint32_t bits[2] = {0xffffffffu, 0xffffffffu};
            if (w.size() == 2) std::memcpy(bits, w.data(), 8);
            separate = separate && w.size() == 2 && std::memcmp(bits, features_probe::kWeights[k][0], 8) == 0;
            fused = fused && w.size() == 2 && std::memcmp(bits, features_probe::kWeights[k][1], 8) == 0;
        }
        if (separate) return VarianceForm::Separate;
        if (fused) return VarianceForm::Fused;
        return Error{ErrorCode::NotSupported, "the host's computeVarianceWeights matches neither variance form"};
    }

    // aggregateEmbedding(records) of every document.  Documents whose first contributing records differ in size go to the
    // device in one call per size.
    Result<std::vector<std::vector<float>>> aggregateEmbeddings(const std::vector<std::vector<FeatureRecord>>& documents) const {
        std::vector<std::vector<float>> out(documents.size());
        struct Group { std::vector<std::size_t> docs; std::vector<std::uint64_t> offsets{0}; std::vector<float> rows; };
        std::map<std::size_t, Group> groups;
        for (std::size_t d = 0; d < documents.size(); ++d) {
            const auto& records = documents[d];
            bool served = false;
            for (const auto& record : records) {
                if (record.documentLevel && !record.embedding.empty()) {
                    out[d].assign(record.embedding.begin(), record.embedding.end());
                    served = true;
                    break;
                }
            }
            if (served) continue;
            Group* g = nullptr;
            std::size_t size = 0, contributing = 0;
            for (const auto& record : records) {
                if (record.embedding.empty()) {
                    continue;
                }
                if (!g) {
                    size = record.embedding.size();
                    g = &groups[size];
                } else if (size != record.embedding.size()) {
                    continue;
                }
                g->rows.insert(g->rows.end(), record.embedding.begin(), record.embedding.end());
                ++contributing;
            }
            if (g) {
                g->docs.push_back(d);
                g->offsets.push_back(g->offsets.back() + contributing);
            }
        }
        for (auto& [size, g] : groups) {
            if (size > YAMS_FEATURES_MAX_DIM) return Error{ErrorCode::NotImplemented, "embedding beyond the accelerator's range"};
            const std::uint64_t total = g.offsets.back();
            std::vector<std::uint32_t> records(total);
            std::iota(records.begin(), records.end(), 0u);
            std::vector<float> sums(g.docs.size() * size);
            std::vector<std::uint32_t> counts(g.docs.size());
            const yams_status_t st = vt_->aggregate(vt_->self, g.rows.data(), total, static_cast<std::uint32_t>(size), g.offsets.data(),
                                                    records.data(), g.docs.size(), sums.data(), counts.data());
            if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_features_v1.aggregate refused the call"};
            for (std::size_t i = 0; i < g.docs.size(); ++i)
                out[g.docs[i]].assign(sums.begin() + static_cast<std::ptrdiff_t>(i * size), sums.begin() + static_cast<std::ptrdiff_t>((i + 1) * size));
        }
        return out;
    }

    // :596-606 — the sample computeVarianceWeights is given: the non-empty embeddings in document order, 4096 at the most.
    static std::vector<std::vector<float>> collectVarianceSample(const std::vector<std::vector<float>>& documentEmbeddings) {
        std::vector<std::vector<float>> sample;
        for (const auto& e : documentEmbeddings) {
            if (!e.empty()) {
                sample.push_back(e);
                if (sample.size() >= kVarianceSampleCap) {
                    break;
                }
            }
        }
        return sample;
    }

    // computeVarianceWeights(embeddings, targetDim)
    Result<std::vector<float>> computeVarianceWeights(const std::vector<std::vector<float>>& embeddings, std::size_t targetDim) const {
        if (embeddings.empty() || targetDim == 0) {
            return std::vector<float>{};
        }
        const std::size_t fullDim = embeddings.front().size();
        if (targetDim >= fullDim) {
            return std::vector<float>{};
        }
        if (fullDim > YAMS_FEATURES_MAX_DIM) return Error{ErrorCode::NotImplemented, "embedding beyond the accelerator's range"};
        std::vector<float> rows;
        std::size_t n = 0;
        for (const auto& e : embeddings) {
            if (e.size() != fullDim) {
                continue;
            }
            rows.insert(rows.end(), e.begin(), e.end());
            ++n;
        }
        if (n == 0) {
            return std::vector<float>{};
        }
        std::vector<double> mean(fullDim), var(fullDim);
        const yams_status_t st = vt_->variance(vt_->self, rows.data(), n, static_cast<std::uint32_t>(fullDim), nullptr, 0,
                                               static_cast<std::uint32_t>(form_), mean.data(), var.data());
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_features_v1.variance refused the call"};
        for (const double v : var)
            if (v != v) return Error{ErrorCode::InvalidArgument, "a variance is a NaN: the reference's comparator is no strict weak order"};
        std::vector<std::size_t> idx(fullDim);
        std::iota(idx.begin(), idx.end(), std::size_t{0});
        std::partial_sort(idx.begin(), idx.begin() + static_cast<std::ptrdiff_t>(targetDim), idx.end(),
                          [&](std::size_t a, std::size_t b) { return var[a] > var[b]; });
        std::vector<float> weights(fullDim, 0.0F);
        for (std::size_t k = 0; k < targetDim; ++k) {
            weights[idx[k]] = static_cast<float>(std::sqrt(var[idx[k]]));
        }
        return weights;
    }

    // composeFeatureVector(dense[i], matryoshkaWeights, entitySignatures[i], sketch of minhashSignatures[i], cfg) of every
    // row.  dense: rows of one size (the extractor's embeddings of one space), none empty.  entitySignatures[i] empty = the
    // document has none (all non-empty ones of one size); minhashSignatures[i] empty = no body.  Either vector may itself be
    // empty (= none anywhere).
    Result<std::vector<std::vector<float>>> composeFeatureVectors(const std::vector<std::vector<float>>& dense,
                                                                  const std::vector<float>& matryoshkaWeights,
                                                                  const std::vector<std::vector<float>>& entitySignatures,
                                                                  const std::vector<std::vector<std::uint32_t>>& minhashSignatures,
                                                                  const FeatureCompositionView& cfg) const {
        const std::size_t n = dense.size();
        if (n == 0) return std::vector<std::vector<float>>{};
        const std::size_t dim = dense.front().size();
        for (const auto& row : dense)
            if (row.empty() || row.size() != dim) return Error{ErrorCode::InvalidArgument, "dense rows must be non-empty and of one size"};
        if ((!entitySignatures.empty() && entitySignatures.size() != n) || (!minhashSignatures.empty() && minhashSignatures.size() != n))
            return Error{ErrorCode::InvalidArgument, "one signature per row, or none at all"};
        // :353-354
        const bool matryoshka = cfg.enableMatryoshkaCoarseView && !matryoshkaWeights.empty() && cfg.matryoshkaTargetDim > 0 &&
                                cfg.matryoshkaTargetDim < dim;
        // :363-364, with extract's own condition on the sketch (:677)
        std::size_t k = 0, sigLen = 0;
        std::vector<std::uint8_t> entityOn(n, 0), sketchOn(n, 0);
        bool anyOn = false;
        for (std::size_t i = 0; i < n; ++i) {
            if (cfg.enableEntityFusion && !entitySignatures.empty() && !entitySignatures[i].empty()) {
                if (k != 0 && entitySignatures[i].size() != k) return Error{ErrorCode::InvalidArgument, "entity signatures of several sizes"};
                k = entitySignatures[i].size();
                entityOn[i] = 1;
                anyOn = true;
            }
            if (cfg.enableMinHashSketch && cfg.minhashSketchDim > 0 && !minhashSignatures.empty() && !minhashSignatures[i].empty()) {
                if (sigLen != 0 && minhashSignatures[i].size() != sigLen) return Error{ErrorCode::InvalidArgument, "signatures of several sizes"};
                sigLen = minhashSignatures[i].size();
                sketchOn[i] = 1;
                anyOn = true;
            }
        }
        // :169-171 — applyMatryoshkaCoarse hands dense back UN-normalised (targetDim is in range by :353-354)
        if (matryoshka && matryoshkaWeights.size() != dim) {
            if (!anyOn) return dense;
            return Error{ErrorCode::NotImplemented, "weights of another size with a fused part: the host's own function"};
        }
        if (dim > YAMS_FEATURES_MAX_DIM || k > YAMS_FEATURES_MAX_DIM || cfg.minhashSketchDim > YAMS_FEATURES_MAX_DIM ||
            sigLen > YAMS_FEATURES_MAX_SIG_LEN)
            return Error{ErrorCode::NotImplemented, "shape beyond the accelerator's range"};
        const std::uint32_t sketchDim = sigLen ? static_cast<std::uint32_t>(cfg.minhashSketchDim) : 0u;
        std::vector<float> flat(n * dim), entity(n * k, 0.0F);
        std::vector<std::uint32_t> sig(n * sigLen, 0u);
        for (std::size_t i = 0; i < n; ++i) {
            std::copy(dense[i].begin(), dense[i].end(), flat.begin() + static_cast<std::ptrdiff_t>(i * dim));
            if (entityOn[i]) std::copy(entitySignatures[i].begin(), entitySignatures[i].end(), entity.begin() + static_cast<std::ptrdiff_t>(i * k));
            if (sketchOn[i]) std::copy(minhashSignatures[i].begin(), minhashSignatures[i].end(), sig.begin() + static_cast<std::ptrdiff_t>(i * sigLen));
        }
        std::size_t kept = dim;
        if (matryoshka) kept = static_cast<std::size_t>(std::count_if(matryoshkaWeights.begin(), matryoshkaWeights.end(), [](float w) { return w > 0.0F; }));
        const std::uint32_t stride = static_cast<std::uint32_t>(kept + k + sketchDim);
        std::vector<float> out(n * stride);
        std::vector<std::uint32_t> dims(n);
        const yams_status_t st = vt_->compose(vt_->self, flat.data(), n, static_cast<std::uint32_t>(dim), matryoshka ? matryoshkaWeights.data() : nullptr,
                                              k ? entity.data() : nullptr, static_cast<std::uint32_t>(k), entityOn.data(),
                                              sigLen ? sig.data() : nullptr, static_cast<std::uint32_t>(sigLen), sketchOn.data(), sketchDim,
                                              cfg.entityFusionAlpha, cfg.minhashAlpha, out.data(), stride, dims.data());
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_features_v1.compose refused the call"};
        std::vector<std::vector<float>> rows(n);
        for (std::size_t i = 0; i < n; ++i)
            rows[i].assign(out.begin() + static_cast<std::ptrdiff_t>(i * stride), out.begin() + static_cast<std::ptrdiff_t>(i * stride + dims[i]));
        return rows;
    }

private:
    AccelTopologyFeatures(std::shared_ptr<accel::Plugin> p, yams_topology_features_v1* vt, VarianceForm form)
        : plugin_(std::move(p)), vt_(vt), form_(form) {}
    std::shared_ptr<accel::Plugin> plugin_;
    yams_topology_features_v1* vt_;
    VarianceForm form_;
};

} // namespace yams::topology
