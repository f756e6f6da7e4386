// colbert_rerank.hpp — the late-interaction rerank of the reference's OnnxColbertSession (plugins/onnx/onnx_colbert_session.cpp:
// computeMaxSim :247-259 with dot :286-293, maxPoolEmbeddings :214-230, normalizeEmbedding :232-245) on the device (plugin
// interface late_interaction_rerank_v1).  scoreDocuments returns what the loop of score_documents
// (plugins/onnx/model_provider.cpp:1886-1888) returns, in one call for the whole window.
//
// What stays on the host, here, line for line:
//   dot's n = std::min(a.size(), b.size())   the device takes ONE dim per call: the shell sends min(query token size, document
//                                            token size) columns of both sides.  An embedding set whose token vectors differ
//                                            in length among themselves has no such dim: it goes to the host's own function.
//   maxPoolEmbeddings' i < token.size()      a token shorter than dim contributes to fewer dimensions: such a set goes back to
//                                            the host too.
//   tokeniser, encoder, skiplist, marker ids, the final sort: never the shell's.
//
// THE FORM IS A PROPERTY OF THE HOST'S BUILD.  `sum += a[i] * b[i]` in fp32 is a rounded multiply and a rounded add, or one
// fmaf, as the host's compiler made it; the score bits differ.  The shell asks the host's OWN computeMaxSim (the callable it is
// created with) on three recorded samples of one query token and one document token whose score bits differ between the forms,
// once per object, and asks the device for the form that reproduces them; a host whose answers match neither is served by its
// own function throughout.
//
// A refusal of the plugin comes back as an Error; the host then runs its own function.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <span>
#include <utility>
#include <vector>

#include "plugin.hpp"

namespace yams::rerank {

enum class DotForm : std::uint32_t { Separate = YAMS_RESIDUAL_SEPARATE, Fused = YAMS_RESIDUAL_FUSED };

// include/yams/daemon/resource/onnx_colbert_session.h:24-27, the fields the arithmetic reads
struct ColbertEmbeddings {
    std::vector<std::vector<float>> token_embeddings;
    std::vector<std::int32_t> token_ids;
};

namespace rerank_probe {
// Three samples of one query token and one document token of four dimensions, found by a CPU search with an exact fmaf (the
// restatement the tests carry; about one draw in two qualifies).  kQuery / kDoc: the bits of the four floats; kScore[case][form]:
// the bits computeMaxSim returns, form 0 = separate multiply and add, form 1 = fmaf.
inline constexpr int kCases = 3;
inline constexpr std::uint32_t kQuery[kCases][4] = {{0xc0871597u, 0x3ead8027u, 0x3f66e3f9u, 0xbf829596u},
                                                    {0xc032613au, 0x3f9092e4u, 0x40c07d12u, 0x40250ecbu},
                                                    {0xbec6a791u, 0x3e98f70au, 0x405f603cu, 0xbf55f4e9u}};
inline constexpr std::uint32_t kDoc[kCases][4] = {{0x402f8035u, 0x3fd8e77cu, 0x406402d2u, 0x408087bdu},
                                                  {0xbee24eceu, 0x3ecdad04u, 0xbf574e66u, 0xbf4063ffu},
                                                  {0xbf0371e6u, 0xbef08807u, 0xc0f22c5du, 0xbf1f578au}};
inline constexpr std::uint32_t kScore[kCases][2] = {{0xc13e2d66u, 0xc13e2d65u}, {0xc0a9f8acu, 0xc0a9f8abu}, {0xc1ceadbdu, 0xc1ceadbeu}};
} // namespace rerank_probe

class AccelColbertReranker {
public:
    using HostMaxSim = std::function<float(const ColbertEmbeddings&, const ColbertEmbeddings&)>;

    // hostMaxSim: the host's own computeMaxSim.  It is probed here, once, and serves whatever the device does not.
    static Result<std::unique_ptr<AccelColbertReranker>> create(std::shared_ptr<accel::Plugin> plugin, HostMaxSim hostMaxSim) {
        auto vt = plugin->getInterface<yams_late_interaction_rerank_v1>(YAMS_IFACE_LATE_INTERACTION_RERANK_V1,
                                                                        YAMS_IFACE_LATE_INTERACTION_RERANK_V1_VERSION);
        if (!vt.has_value()) return vt.error();
        return std::unique_ptr<AccelColbertReranker>(new AccelColbertReranker(std::move(plugin), vt.value(), std::move(hostMaxSim)));
    }
    // Over a table the caller owns (a host that binds the interface itself).
    static std::unique_ptr<AccelColbertReranker> over(yams_late_interaction_rerank_v1* vt, HostMaxSim hostMaxSim) {
        return std::unique_ptr<AccelColbertReranker>(new AccelColbertReranker(nullptr, vt, std::move(hostMaxSim)));
    }

    // The form the probe found; empty: neither, the device path is refused and every score is the host function's.
    std::optional<DotForm> form() const { return form_; }
    // Calls that reached the device table / scores the host's own function gave (probe calls not counted).
    std::uint64_t deviceCalls() const { return deviceCalls_; }
    std::uint64_t hostScores() const { return hostScores_; }

    // Which form is hostFn?  Empty: neither.
    static std::optional<DotForm> probeForm(const HostMaxSim& hostFn) {
        bool separate = true, fused = true;
        for (int k = 0; k < rerank_probe::kCases; ++k) {
            ColbertEmbeddings q, d;
            q.token_embeddings.assign(1, std::vector<float>(4));
            d.token_embeddings.assign(1, std::vector<float>(4));
            std::memcpy(q.token_embeddings[0].data(), rerank_probe::kQuery[k], 16);
            std::memcpy(d.token_embeddings[0].data(), rerank_probe::kDoc[k], 16);
            const float s = hostFn(q, d);
            std::uint32_t bits;
            std::memcpy(&bits, &s, 4);
            separate = separate && bits == rerank_probe::kScore[k][0];
            fused = fused && bits == rerank_probe::kScore[k][1];
        }
        if (separate) return DotForm::Separate;
        if (fused) return DotForm::Fused;
        return std::nullopt;
    }

    // computeMaxSim(query, document)
    float computeMaxSim(const ColbertEmbeddings& query, const ColbertEmbeddings& document) {
        return scoreDocuments(query, std::span<const ColbertEmbeddings>(&document, 1)).front();
    }

    // { computeMaxSim(query, d) for d in documents }: the loop of model_provider.cpp:1886-1888.  Documents whose token vectors
    // are of one length go to the device, one call per length; the others, and everything the device refuses, are the host
    // function's.
    std::vector<float> scoreDocuments(const ColbertEmbeddings& query, std::span<const ColbertEmbeddings> documents) {
        std::vector<float> scores(documents.size());
        std::vector<char> done(documents.size(), 0);
        const std::size_t tq = query.token_embeddings.size();
        const std::optional<std::size_t> dq = uniformSize(query);
        if (form_ && dq && tq <= YAMS_RERANK_MAX_QUERY_TOKENS) {
            // the window by document token size (an empty document has none: any group serves it — it scores -inf per query token)
            std::map<std::size_t, std::vector<std::size_t>> groups;
            std::vector<std::size_t> empties;
            for (std::size_t i = 0; i < documents.size(); ++i) {
                if (documents[i].token_embeddings.empty()) { empties.push_back(i); continue; }
                if (const auto dd = uniformSize(documents[i])) groups[*dd].push_back(i);
            }
            if (!empties.empty()) {
                auto& first = groups.empty() ? groups[tq ? *dq : std::size_t{1}] : groups.begin()->second;
                first.insert(first.end(), empties.begin(), empties.end());
            }
            for (const auto& [dd, members] : groups) {
                const std::size_t dim = tq ? std::min(*dq, dd) : dd;
                // dim == 0: every dot is the empty sum +0.0f, which the device entry (dim >= 1) does not serve
                if (dim == 0 || dim > YAMS_RERANK_MAX_DIM) continue;
                std::vector<float> q(tq * dim), rows;
                for (std::size_t t = 0; t < tq; ++t) std::copy_n(query.token_embeddings[t].begin(), dim, q.begin() + static_cast<std::ptrdiff_t>(t * dim));
                std::vector<std::uint64_t> offsets{0};
                for (const std::size_t i : members) {
                    for (const auto& token : documents[i].token_embeddings) rows.insert(rows.end(), token.begin(), token.begin() + static_cast<std::ptrdiff_t>(dim));
                    offsets.push_back(rows.size() / dim);
                }
                std::vector<float> out(members.size());
                ++deviceCalls_;
                const yams_status_t st = vt_->maxsim(vt_->self, q.data(), static_cast<std::uint32_t>(tq), static_cast<std::uint32_t>(dim), rows.data(),
                                                     offsets.data(), members.size(), static_cast<std::uint32_t>(*form_), out.data(), nullptr, nullptr,
                                                     nullptr);
                if (st != YAMS_OK) continue;      // refused: the host's own function below
                for (std::size_t k = 0; k < members.size(); ++k) {
                    scores[members[k]] = out[k];
                    done[members[k]] = 1;
                }
            }
        }
        for (std::size_t i = 0; i < documents.size(); ++i)
            if (!done[i]) {
                scores[i] = host_(query, documents[i]);
                ++hostScores_;
            }
        return scores;
    }

    // normalizeEmbedding(maxPoolEmbeddings(d, dim)) of every document.  A token shorter than dim: NotImplemented, the host's own
    // functions (their i < token.size()).
    Result<std::vector<std::vector<float>>> poolAndNormalize(std::span<const ColbertEmbeddings> documents, std::size_t dim) {
        if (dim == 0) return std::vector<std::vector<float>>(documents.size());
        if (dim > YAMS_RERANK_MAX_DIM) return Error{ErrorCode::NotImplemented, "dim beyond the accelerator's range"};
        std::vector<float> rows;
        std::vector<std::uint64_t> offsets{0};
        for (const auto& d : documents) {
            for (const auto& token : d.token_embeddings) {
                if (token.size() < dim) return Error{ErrorCode::NotImplemented, "a token shorter than dim: the host's own function"};
                rows.insert(rows.end(), token.begin(), token.begin() + static_cast<std::ptrdiff_t>(dim));
            }
            offsets.push_back(rows.size() / dim);
        }
        std::vector<float> out(documents.size() * dim);
        ++deviceCalls_;
        const yams_status_t st = vt_->maxpool(vt_->self, rows.data(), static_cast<std::uint32_t>(dim), offsets.data(), documents.size(), out.data());
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "late_interaction_rerank_v1.maxpool refused the call"};
        std::vector<std::vector<float>> pooled(documents.size());
        for (std::size_t i = 0; i < documents.size(); ++i)
            pooled[i].assign(out.begin() + static_cast<std::ptrdiff_t>(i * dim), out.begin() + static_cast<std::ptrdiff_t>((i + 1) * dim));
        return pooled;
    }

private:
    AccelColbertReranker(std::shared_ptr<accel::Plugin> p, yams_late_interaction_rerank_v1* vt, HostMaxSim host)
        : plugin_(std::move(p)), vt_(vt), host_(std::move(host)), form_(probeForm(host_)) {}

    // the one length of the set's token vectors; empty when they differ (an empty set: 0)
    static std::optional<std::size_t> uniformSize(const ColbertEmbeddings& e) {
        if (e.token_embeddings.empty()) return std::size_t{0};
        const std::size_t n = e.token_embeddings.front().size();
        for (const auto& token : e.token_embeddings)
            if (token.size() != n) return std::nullopt;
        return n;
    }

    std::shared_ptr<accel::Plugin> plugin_;
    yams_late_interaction_rerank_v1* vt_;
    HostMaxSim host_;
    std::optional<DotForm> form_;
    std::uint64_t deviceCalls_ = 0, hostScores_ = 0;
};

} // namespace yams::rerank
