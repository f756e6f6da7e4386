// topological_quality.hpp — yams::search::computePersistenceH0 of the reference (include/yams/search/topological_quality.h,
// src/search/topological_quality.cpp:75-148) with its array arithmetic on the device (plugin interface topology_quality_v1).
//
// What stays on the host, here, line for line: the early returns of both overloads (count < 2, dim == 0, a span shorter than
// count * dim, :77-79; an empty outer vector, a first row of size 0, ragged rows, :131-146) and the flattening of the
// vector-of-vectors overload.  What the device computes: the m (m - 1) / 2 distances, the percentile, the spanning tree; the
// plugin's host side sorts the tree's m - 1 weights and sums the m - 2 quotients.
//
// deterministicSubsample (:150-167) stays the host's altogether: it is std::shuffle over std::mt19937_64, and the sequence of
// std::shuffle belongs to the host's standard library.  The host draws its sample, then hands the points over.
//
// THE CHAIN FORM IS A PROPERTY OF THE HOST'S BUILD.  d = double(a[k]) - double(b[k]) carries up to 53 bits, so d * d is not
// exact and the bits of `acc += d * d` depend on whether the host's compiler contracted it into an fma.  probeChainForm() asks
// the host's OWN computePersistenceH0 on crafted three-point clouds — there the value is ONE quotient (shortest distance /
// middle distance), so a one-ulp difference of a distance is visible, while the sum over a large cloud absorbs it — and
// reports which of the two forms the device offers reproduces it; a host whose answers match neither gets an Error and runs
// its own function.
//
// A refusal of the plugin (more than YAMS_QUALITY_MAX_POINTS points, dim beyond YAMS_CLUSTER_MAX_DIM, a non-finite element,
// no memory for the matrix) comes back as an Error; the host then runs its own function.
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <span>
#include <utility>
#include <vector>

#include "plugin.hpp"

namespace yams::search {

enum class ChainForm : std::uint32_t { Separate = YAMS_RESIDUAL_SEPARATE, Fused = YAMS_RESIDUAL_FUSED };

namespace quality_probe {
// Three independent clouds of three points in two dimensions, found by a CPU search with an exact fma (the restatement the
// tests carry; 20 000 draws with mixed exponents gave a few hundred such clouds).  kPoints: the bits of the six
// floats, point after point; kValue[case][form]: the bits of computePersistenceH0's return value, form 0 = separate multiply and
// add, form 1 = fma.  In each case the two differ by one or two units in the last place.
inline constexpr int kCases = 3;
inline constexpr std::uint32_t kPoints[kCases][6] = {
    {0x3c7cc4f2u, 0xbf62fd3bu, 0x4107c0c1u, 0x3e62b175u, 0x40858bc2u, 0xbcf1f861u},
    {0xbd2bf56au, 0x3ec90e80u, 0xc04bb5c3u, 0xbc1df9eeu, 0x41334bebu, 0xc31f4ad4u},
    {0xbc5d077fu, 0x41b67fa4u, 0xc09161a7u, 0xc0010719u, 0xbf356996u, 0xbe2fb7f4u}};
inline constexpr std::uint64_t kValue[kCases][2] = {{0x3fef751539642ee7ull, 0x3fef751539642ee9ull},
                                                    {0x3f944677de6ac227ull, 0x3f944677de6ac228ull},
                                                    {0x3fc7afa60fb284d2ull, 0x3fc7afa60fb284d1ull}};
} // namespace quality_probe

class AccelTopologicalQuality {
public:
    static Result<std::unique_ptr<AccelTopologicalQuality>> create(std::shared_ptr<accel::Plugin> plugin, ChainForm form) {
        auto vt = plugin->getInterface<yams_topology_quality_v1>(YAMS_IFACE_TOPOLOGY_QUALITY_V1, YAMS_IFACE_TOPOLOGY_QUALITY_V1_VERSION);
        if (!vt.has_value()) return vt.error();
        return std::unique_ptr<AccelTopologicalQuality>(new AccelTopologicalQuality(std::move(plugin), vt.value(), form));
    }
    // Over a table the caller owns (a host that binds the interface itself).
    static std::unique_ptr<AccelTopologicalQuality> over(yams_topology_quality_v1* vt, ChainForm form) {
        return std::unique_ptr<AccelTopologicalQuality>(new AccelTopologicalQuality(nullptr, vt, form));
    }
    ChainForm form() const { return form_; }

    // Which form is the host's own computePersistenceH0?  hostFn(std::span<const float>, count, dim) is that function.
    template <class HostFn> static Result<ChainForm> probeChainForm(HostFn&& hostFn) {
        bool separate = true, fused = true;
        for (int k = 0; k < quality_probe::kCases; ++k) {
            float points[6];
            std::memcpy(points, quality_probe::kPoints[k], sizeof points);
            const double value = hostFn(std::span<const float>(points, 6), std::size_t{3}, std::size_t{2});
            std::uint64_t bits;
            std::memcpy(&bits, &value, 8);
            separate = separate && bits == quality_probe::kValue[k][0];
            fused = fused && bits == quality_probe::kValue[k][1];
        }
        if (separate) return ChainForm::Separate;
        if (fused) return ChainForm::Fused;
        return Error{ErrorCode::NotSupported, "the host's computePersistenceH0 matches neither chain form"};
    }

    // computePersistenceH0(embeddings, count, dim)
    Result<double> computePersistenceH0(std::span<const float> embeddings, std::size_t count, std::size_t dim) const {
        if (count < 2 || dim == 0 || embeddings.size() < count * dim) {
            return 0.0;
        }
        if (count > YAMS_QUALITY_MAX_POINTS || dim > YAMS_CLUSTER_MAX_DIM)
            return Error{ErrorCode::NotImplemented, "point cloud beyond the accelerator's range"};
        yams_persistence_h0_t out{};
        const yams_status_t st = vt_->persistence_h0(vt_->self, embeddings.data(), count, static_cast<std::uint32_t>(dim), nullptr, 0,
                                                     static_cast<std::uint32_t>(form_), &out, nullptr, nullptr);
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "topology_quality_v1.persistence_h0 refused the call"};
        return out.value;
    }

    // computePersistenceH0(embeddings)
    Result<double> computePersistenceH0(const std::vector<std::vector<float>>& embeddings) const {
        if (embeddings.empty()) {
            return 0.0;
        }
        const std::size_t count = embeddings.size();
        const std::size_t dim = embeddings.front().size();
        if (dim == 0) {
            return 0.0;
        }
        std::vector<float> flat;
        flat.reserve(count * dim);
        for (const auto& row : embeddings) {
            if (row.size() != dim) {
                return 0.0;
            }
            flat.insert(flat.end(), row.begin(), row.end());
        }
        return computePersistenceH0(std::span<const float>(flat), count, dim);
    }

private:
    AccelTopologicalQuality(std::shared_ptr<accel::Plugin> p, yams_topology_quality_v1* vt, ChainForm form)
        : plugin_(std::move(p)), vt_(vt), form_(form) {}
    std::shared_ptr<accel::Plugin> plugin_;
    yams_topology_quality_v1* vt_;
    ChainForm form_;
};

} // namespace yams::search
