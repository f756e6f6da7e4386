// embedding_pool.hpp — the pooling head of the reference's embedding sessions (plugins/onnx/onnx_model_pool.cpp:1808-1854 the
// batch path, :1729-1774 and :1448-1491 the same loops; :1935-1953 the rank-2 output) on the device (plugin interface
// embedding_pool_v1).  pool() takes what OnnxModelSession::runOnnxBatch has in hand once the encoder has run — the output
// tensor's data, B, SS, DD, the attention masks, the pooling mode and normalize_ — and returns what its loop builds.
//
// What stays on the host, here (hostPool below is the entry's contract written out over host memory, compiled by the host's own
// compiler; tests hold it to the golden file of the reference's loops):
//   masks[b].size() per text     the device takes ONE mask_len per call: masks of unequal lengths go to the host loop.
//   MEAN with a weight above 1   x * w is no longer exact, so the result depends on whether the host's build fuses the multiply
//                                into the add: the device refuses it, and so does the shell before it flattens anything.  The
//                                reference's own generateAttentionMask (onnx_text_processing.cpp:95-104) only produces 0 and 1.
//   whatever the flat entry calls unsupported (dim, seq or batch * seq beyond its limits): the host loop.
//   tokeniser, encoder session, batching, retries, cap learning: never the shell's.
//
// The second way in, HiddenStates::onDevice, is for a host that bound the encoder's output to device memory (ONNX Runtime I/O
// binding on the ROCm / MIGraphX execution provider): the hidden states never cross the bus, the masks and the B * DD result
// do.  Nothing can be handed to the host loop on that route: what the device refuses comes back as an Error.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "plugin.hpp"

namespace yams::embed {

// plugins/onnx/onnx_model_pool.cpp:1984, the order of the reference's enum
enum class Pooling { MEAN, CLS, MAX };

// The encoder's output [B][SS][DD] fp32: in host memory (the default) or at a device address of the plugin's device.
struct HiddenStates {
    const float* data;
    bool deviceResident;
    HiddenStates(const float* hostData) : data(hostData), deviceResident(false) {}      // NOLINT: a plain pointer is host memory
    static HiddenStates onDevice(const float* deviceData) { HiddenStates h(deviceData); h.deviceResident = true; return h; }
};

class AccelEmbeddingPooler {
public:
    static Result<std::unique_ptr<AccelEmbeddingPooler>> create(std::shared_ptr<accel::Plugin> plugin) {
        auto vt = plugin->getInterface<yams_embedding_pool_v1>(YAMS_IFACE_EMBEDDING_POOL_V1, YAMS_IFACE_EMBEDDING_POOL_V1_VERSION);
        if (!vt.has_value()) return vt.error();
        return std::unique_ptr<AccelEmbeddingPooler>(new AccelEmbeddingPooler(std::move(plugin), vt.value()));
    }
    // Over a table the caller owns (a host that binds the interface itself).
    static std::unique_ptr<AccelEmbeddingPooler> over(yams_embedding_pool_v1* vt) {
        return std::unique_ptr<AccelEmbeddingPooler>(new AccelEmbeddingPooler(nullptr, vt));
    }

    // Calls that reached the device table / calls the host loop served.
    std::uint64_t deviceCalls() const { return deviceCalls_; }
    std::uint64_t hostCalls() const { return hostCalls_; }

    static std::uint32_t modeOf(Pooling p) { return p == Pooling::CLS ? YAMS_EMBED_POOL_CLS : p == Pooling::MAX ? YAMS_EMBED_POOL_MAX : YAMS_EMBED_POOL_MEAN; }

    // The host loop the shell carries: the contract of yams_embed_pool (include/yams_mi355x_accel.h) written out over host memory,
    // with one mask per text of whatever length and weights of any value.  Compiled by the host's compiler with the host's
    // flags, so a weighted step (w > 1) fuses or not as the host's own loop does.  Per text: the considered tokens whose mask
    // is positive are picked first, then every picked row is folded into the text's output row in token order.
    static std::vector<std::vector<float>> hostPool(const float* hidden, std::size_t batch, std::size_t seq, std::size_t dim,
                                                    const std::vector<std::vector<std::int32_t>>& masks, Pooling mode, bool normalize) {
        std::vector<std::vector<float>> pooled(batch);
        std::vector<std::size_t> picked;
        for (std::size_t text = 0; text < batch; ++text) {
            std::vector<float>& row = pooled[text];
            const float* tokens = hidden + text * seq * dim;
            if (mode == Pooling::CLS) {
                row.assign(tokens, tokens + dim);      // token 0, whatever the mask says
            } else {
                row.assign(dim, 0.0f);
                const std::vector<std::int32_t>& mask = masks[text];
                const std::size_t considered = mask.size() < seq ? mask.size() : seq;
                picked.clear();
                for (std::size_t t = 0; t < considered; ++t)
                    if (mask[t] > 0) picked.push_back(t);
                if (mode == Pooling::MAX) {
                    for (const std::size_t t : picked) {
                        const float* x = tokens + t * dim;
                        for (std::size_t k = 0; k < dim; ++k)
                            if (row[k] < x[k]) row[k] = x[k];      // a NaN never enters; the floor is the initial +0.0f
                    }
                } else {
                    float weightSum = 0.0f;
                    for (const std::size_t t : picked) {
                        const float weight = static_cast<float>(mask[t]);
                        const float* x = tokens + t * dim;
                        weightSum = weightSum + weight;
                        for (std::size_t k = 0; k < dim; ++k) row[k] = row[k] + x[k] * weight;
                    }
                    if (weightSum > 0.0f)
                        for (std::size_t k = 0; k < dim; ++k) row[k] = row[k] / weightSum;
                }
            }
            if (normalize) hostNormalize(row);
        }
        return pooled;
    }
    // The contract's normalisation: one fp64 chain of squares in element order; a norm above 1e-8 divides in fp64, any other
    // norm (a NaN one too) gives zeros.
    static void hostNormalize(std::vector<float>& row) {
        double squares = 0.0;
        for (std::size_t k = 0; k < row.size(); ++k) squares = squares + static_cast<double>(row[k]) * static_cast<double>(row[k]);
        const double norm = std::sqrt(squares);
        const bool served = norm > 1e-8;
        for (std::size_t k = 0; k < row.size(); ++k) row[k] = served ? static_cast<float>(static_cast<double>(row[k]) / norm) : 0.0f;
    }

    // result[b] = the pooled (and, with normalize, L2-normalised) embedding of text b.  masks: one vector per text (unused for
    // CLS).  Host-resident hidden states: never an Error for what the device refuses as unsupported — the host loop serves it.
    Result<std::vector<std::vector<float>>> pool(HiddenStates hidden, std::size_t B, std::size_t SS, std::size_t DD,
                                                 const std::vector<std::vector<std::int32_t>>& masks, Pooling mode, bool normalize) {
        if (B == 0) return std::vector<std::vector<float>>();
        if (!hidden.data) return Error{ErrorCode::InvalidArgument, "null hidden states"};
        if (mode != Pooling::CLS && masks.size() < B) return Error{ErrorCode::InvalidArgument, "fewer masks than texts"};
        const bool host = !hidden.deviceResident;
        auto toHost = [&](const char* why) -> Result<std::vector<std::vector<float>>> {
            if (!host) return Error{ErrorCode::NotImplemented, why};
            ++hostCalls_;
            return hostPool(hidden.data, B, SS, DD, masks, mode, normalize);
        };
        if (DD == 0 || SS == 0) return Error{ErrorCode::InvalidArgument, "an empty tensor"};      // the flat entry's verdict, on both routes
        if (DD > YAMS_EMBED_MAX_DIM || SS > YAMS_EMBED_MAX_SEQ || B > YAMS_EMBED_MAX_ROWS / SS) return toHost("beyond the accelerator's limits");
        std::vector<std::int32_t> flat;
        std::size_t maskLen = 0;
        if (mode != Pooling::CLS) {
            maskLen = masks[0].size();
            for (std::size_t b = 0; b < B; ++b)
                if (masks[b].size() != maskLen) return toHost("masks of unequal lengths: the host's own loop");
            if (maskLen > 0xffffffffull) return toHost("a mask beyond the accelerator's limits");
            const std::size_t considered = std::min(SS, maskLen);
            if (mode == Pooling::MEAN)
                for (std::size_t b = 0; b < B; ++b)
                    for (std::size_t i = 0; i < considered; ++i)
                        if (masks[b][i] > 1) return toHost("a MEAN weight above 1: the host's own loop");
            flat.reserve(B * maskLen);
            for (std::size_t b = 0; b < B; ++b) flat.insert(flat.end(), masks[b].begin(), masks[b].end());
        }
        std::vector<float> out(B * DD);
        ++deviceCalls_;
        const auto fn = host ? vt_->pool : vt_->pool_device;
        const yams_status_t st = fn(vt_->self, hidden.data, B, static_cast<std::uint32_t>(SS), static_cast<std::uint32_t>(DD),
                                    flat.empty() ? nullptr : flat.data(), static_cast<std::uint32_t>(maskLen), modeOf(mode),
                                    normalize ? YAMS_EMBED_NORMALIZE : 0u, out.data(), &lastDiag_);
        if (st == YAMS_ERR_UNSUPPORTED) return toHost("embedding_pool_v1.pool: unsupported");
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "embedding_pool_v1.pool refused the call"};
        return rowsOf(out, B, DD);
    }

    // The rank-2 output [B][DD] (:1935-1953): every row copied and, with normalize, L2-normalised.
    Result<std::vector<std::vector<float>>> normalizeRows(HiddenStates rows, std::size_t B, std::size_t DD, bool normalize) {
        if (B == 0) return std::vector<std::vector<float>>();
        if (!rows.data) return Error{ErrorCode::InvalidArgument, "null rows"};
        const bool host = !rows.deviceResident;
        if (DD == 0) return Error{ErrorCode::InvalidArgument, "an empty tensor"};
        if (host && (!normalize || DD > YAMS_EMBED_MAX_DIM || B > YAMS_EMBED_MAX_ROWS)) {      // a copy, or beyond the limits
            ++hostCalls_;
            std::vector<std::vector<float>> copied = rowsOf(std::vector<float>(rows.data, rows.data + B * DD), B, DD);
            if (normalize)
                for (auto& row : copied) hostNormalize(row);
            return copied;
        }
        if (!normalize) return Error{ErrorCode::NotImplemented, "a plain copy of device rows is the host's own"};
        std::vector<float> out(B * DD);
        ++deviceCalls_;
        const auto fn = host ? vt_->normalize : vt_->normalize_device;
        const yams_status_t st = fn(vt_->self, rows.data, B, static_cast<std::uint32_t>(DD), out.data());
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "embedding_pool_v1.normalize refused the call"};
        return rowsOf(out, B, DD);
    }

    // The diag of the last pool() call the device served.
    const yams_embed_diag_t& lastDiag() const { return lastDiag_; }

private:
    AccelEmbeddingPooler(std::shared_ptr<accel::Plugin> p, yams_embedding_pool_v1* vt) : plugin_(std::move(p)), vt_(vt) {}

    static std::vector<std::vector<float>> rowsOf(const std::vector<float>& out, std::size_t B, std::size_t DD) {
        std::vector<std::vector<float>> result(B);
        for (std::size_t b = 0; b < B; ++b)
            result[b].assign(out.begin() + static_cast<std::ptrdiff_t>(b * DD), out.begin() + static_cast<std::ptrdiff_t>((b + 1) * DD));
        return result;
    }

    std::shared_ptr<accel::Plugin> plugin_;
    yams_embedding_pool_v1* vt_;
    yams_embed_diag_t lastDiag_{};
    std::uint64_t deviceCalls_ = 0, hostCalls_ = 0;
};

} // namespace yams::embed
