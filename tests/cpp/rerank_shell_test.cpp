// rerank_shell_test — drives include/yams_accel/colbert_rerank.hpp (AccelColbertReranker) on a case file
// (tests/_rerank_oracle.py write_cases) and prints, per case, the bits of its output.
//   rerank_shell_test [--fused] <cases>                 the shell over a stand-in table (the restatement of rerank_oracle.cpp)
//                                                       with a host function of the given form: runs anywhere, also under
//                                                       ASan / UBSan
//   rerank_shell_test [--fused] --plugin <lib> <cases>  the same through the real late_interaction_rerank_v1
//   rerank_shell_test --selftest                        the shell's own rules over the stand-in: the probe's three answers,
//                                                       ragged token vectors, min(dim), refusals, empties
//   built with -DRERANK_WITH_REFERENCE and rerank_ref_cut.inc on the include path (the four member functions of the reference,
//   cut by tests/golden/make_rerank_golden.py into its temporary directory): the REFERENCE'S functions are called instead of
//   the shell; it prints `probe -` and the generator judges the form from the flip cases.
// Output: `probe <separate|fused|neither|->`, then per case one line `case <index> <hex of the floats' bytes>` (the scores of a
// maxsim case, the pooled rows of a pool case one after the other).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#ifdef RERANK_WITH_REFERENCE
struct ColbertEmbeddings {
    std::vector<std::vector<float>> token_embeddings;
};
struct ReferenceImpl {
#include "rerank_ref_cut.inc"      // maxPoolEmbeddings, normalizeEmbedding, computeMaxSim, dot — the reference's text
};
#else
#include <yams_accel/colbert_rerank.hpp>
#include "rerank_oracle.cpp"
using yams::rerank::AccelColbertReranker;
using yams::rerank::ColbertEmbeddings;
using yams::rerank::DotForm;
#endif

namespace {

struct Reader {
    std::vector<unsigned char> bytes; size_t at = 0;
    std::uint32_t u32() { std::uint32_t v; std::memcpy(&v, bytes.data() + at, 4); at += 4; return v; }
    ColbertEmbeddings tokens(std::uint32_t n, std::uint32_t dim) {
        ColbertEmbeddings e;
        e.token_embeddings.assign(n, std::vector<float>(dim));
        for (auto& t : e.token_embeddings) {
            if (dim) std::memcpy(t.data(), bytes.data() + at, dim * 4);
            at += dim * 4;
        }
        return e;
    }
};

void printCase(std::uint32_t index, const std::vector<float>& v) {
    std::printf("case %u ", index);
    for (const float x : v) {
        unsigned char b[4];
        std::memcpy(b, &x, 4);
        std::printf("%02x%02x%02x%02x", b[0], b[1], b[2], b[3]);
    }
    std::printf("\n");
}

#ifndef RERANK_WITH_REFERENCE
int g_calls = 0;
bool g_refuse = false;
std::uint32_t g_last_dim = 0, g_last_form = 99;

// the stand-in table: the flat entries' limits and statuses, the restatement's arithmetic
yams_status_t standin_maxsim(void*, const float* query, uint32_t tq, uint32_t dim, const float* rows, const uint64_t* off, uint64_t n_docs,
                             uint32_t form, float* out_scores, float* out_rowmax, uint32_t* out_rowarg, yams_rerank_diag_t* diag) {
    ++g_calls;
    g_last_dim = dim;
    g_last_form = form;
    if (g_refuse) return YAMS_ERR_RESOURCE_EXHAUSTED;
    if (dim > YAMS_RERANK_MAX_DIM || tq > YAMS_RERANK_MAX_QUERY_TOKENS || n_docs > YAMS_RERANK_MAX_DOCS) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0 || form > YAMS_RESIDUAL_FUSED) return YAMS_ERR_INVALID_ARG;
    if (n_docs == 0) return YAMS_OK;
    if (!off || !out_scores || off[0] != 0 || (tq && !query)) return YAMS_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < n_docs; ++i)
        if (off[i + 1] < off[i]) return YAMS_ERR_INVALID_ARG;
    if (off[n_docs] && !rows) return YAMS_ERR_INVALID_ARG;
    rerank_oracle_maxsim(query, tq, dim, rows, off, n_docs, form, out_scores, out_rowmax, out_rowmax ? out_rowarg : nullptr);
    if (diag) *diag = yams_rerank_diag_t{YAMS_RERANK_PATH_VALU, form, off[n_docs], n_docs, tq, 0};
    return YAMS_OK;
}
yams_status_t standin_maxpool(void*, const float* rows, uint32_t dim, const uint64_t* off, uint64_t n_docs, float* out) {
    ++g_calls;
    if (g_refuse) return YAMS_ERR_RESOURCE_EXHAUSTED;
    if (dim > YAMS_RERANK_MAX_DIM || n_docs > YAMS_RERANK_MAX_DOCS) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0) return YAMS_ERR_INVALID_ARG;
    if (n_docs == 0) return YAMS_OK;
    if (!off || !out || off[0] != 0 || (off[n_docs] && !rows)) return YAMS_ERR_INVALID_ARG;
    rerank_oracle_maxpool(rows, dim, off, n_docs, out);
    return YAMS_OK;
}
yams_late_interaction_rerank_v1 g_standin = {YAMS_IFACE_LATE_INTERACTION_RERANK_V1_VERSION, nullptr, standin_maxsim, standin_maxpool};

// what a host of the given form computes: the reference's loops over vectors of vectors, dot with n = min of the two sizes
int g_host_calls = 0;
float hostMaxSim(const ColbertEmbeddings& query, const ColbertEmbeddings& document, std::uint32_t form) {
    ++g_host_calls;
    float score = 0.0f;
    for (const auto& q : query.token_embeddings) {
        float maxSim = -std::numeric_limits<float>::infinity();
        for (const auto& d : document.token_embeddings) {
            const float sim = rerank_oracle_dot(q.data(), d.data(), static_cast<std::uint32_t>(std::min(q.size(), d.size())), form);
            if (sim > maxSim) maxSim = sim;
        }
        score += maxSim;
    }
    return score;
}
AccelColbertReranker::HostMaxSim hostOf(std::uint32_t form) {
    return [form](const ColbertEmbeddings& q, const ColbertEmbeddings& d) { return hostMaxSim(q, d, form); };
}

std::uint32_t bitsOf(float x) { std::uint32_t b; std::memcpy(&b, &x, 4); return b; }
bool sameScores(const std::vector<float>& a, const std::vector<float>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (bitsOf(a[i]) != bitsOf(b[i]) && !(a[i] != a[i] && b[i] != b[i])) return false;
    return true;
}
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "selftest: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

ColbertEmbeddings ramp(std::size_t tokens, std::size_t dim, float seed) {
    ColbertEmbeddings e;
    for (std::size_t t = 0; t < tokens; ++t) {
        std::vector<float> v(dim);
        for (std::size_t i = 0; i < dim; ++i) v[i] = std::sin(seed + 1.7f * static_cast<float>(t) + 0.31f * static_cast<float>(i)) * (1.0f + static_cast<float>(i % 5));
        e.token_embeddings.push_back(std::move(v));
    }
    return e;
}

int selftest() {
    // ---- the probe's three answers ----
    for (std::uint32_t form = 0; form < 2; ++form) {
        auto s = AccelColbertReranker::over(&g_standin, hostOf(form));
        CHECK(s->form().has_value() && static_cast<std::uint32_t>(*s->form()) == form);
        const ColbertEmbeddings q = ramp(5, 48, 0.5f);
        const std::vector<ColbertEmbeddings> docs = {ramp(9, 48, 1.0f), ramp(0, 48, 0.0f), ramp(33, 48, 2.0f)};
        g_calls = 0;
        const std::vector<float> got = s->scoreDocuments(q, docs);
        CHECK(g_calls == 1 && g_last_form == form && g_last_dim == 48 && s->hostScores() == 0);
        std::vector<float> want;
        for (const auto& d : docs) want.push_back(hostMaxSim(q, d, form));
        CHECK(sameScores(got, want));
        CHECK(got[1] == -std::numeric_limits<float>::infinity());      // an empty document
        CHECK(bitsOf(s->computeMaxSim(q, docs[2])) == bitsOf(want[2]));
    }
    {   // neither form: a host that sums in fp64.  The device path is refused: no call reaches the table.
        auto odd = [](const ColbertEmbeddings& q, const ColbertEmbeddings& d) {
            double score = 0.0;
            for (const auto& a : q.token_embeddings) {
                double best = -std::numeric_limits<double>::infinity();
                for (const auto& b : d.token_embeddings) {
                    double sum = 0.0;
                    for (size_t i = 0; i < std::min(a.size(), b.size()); ++i) sum += static_cast<double>(a[i]) * b[i];
                    best = std::max(best, sum);
                }
                score += best;
            }
            return static_cast<float>(score * 1.0000001);
        };
        auto s = AccelColbertReranker::over(&g_standin, odd);
        CHECK(!s->form().has_value());
        const ColbertEmbeddings q = ramp(3, 8, 0.25f);
        const std::vector<ColbertEmbeddings> docs = {ramp(4, 8, 1.0f), ramp(2, 8, 3.0f)};
        g_calls = 0;
        const std::vector<float> got = s->scoreDocuments(q, docs);
        CHECK(g_calls == 0 && s->hostScores() == 2 && s->deviceCalls() == 0);
        CHECK(bitsOf(got[0]) == bitsOf(odd(q, docs[0])) && bitsOf(got[1]) == bitsOf(odd(q, docs[1])));
    }
    // ---- ragged token vectors go back to the host; the others of the window are still served ----
    for (std::uint32_t form = 0; form < 2; ++form) {
        auto s = AccelColbertReranker::over(&g_standin, hostOf(form));
        const ColbertEmbeddings q = ramp(4, 16, 0.5f);
        ColbertEmbeddings ragged = ramp(6, 16, 1.5f);
        ragged.token_embeddings[3].resize(11);
        const std::vector<ColbertEmbeddings> docs = {ramp(5, 16, 1.0f), ragged, ramp(7, 16, 2.0f)};
        g_calls = 0; g_host_calls = 0;
        const std::vector<float> got = s->scoreDocuments(q, docs);
        CHECK(g_calls == 1 && g_host_calls == 1 && s->hostScores() == 1);
        std::vector<float> want;
        for (const auto& d : docs) want.push_back(hostMaxSim(q, d, form));
        CHECK(sameScores(got, want));
        // a ragged query: everything is the host's
        ColbertEmbeddings rq = q;
        rq.token_embeddings[1].resize(3);
        g_calls = 0; g_host_calls = 0;
        const std::vector<float> got2 = s->scoreDocuments(rq, docs);
        CHECK(g_calls == 0 && g_host_calls == 3);
        want.clear();
        for (const auto& d : docs) want.push_back(hostMaxSim(rq, d, form));
        CHECK(sameScores(got2, want));
    }
    // ---- min(dim): the query shorter, a document shorter, documents of two sizes in one window ----
    for (std::uint32_t form = 0; form < 2; ++form) {
        auto s = AccelColbertReranker::over(&g_standin, hostOf(form));
        const ColbertEmbeddings q = ramp(3, 12, 0.5f);
        const std::vector<ColbertEmbeddings> longer = {ramp(5, 20, 1.0f)}, shorter = {ramp(5, 7, 1.0f)};
        g_calls = 0;
        CHECK(bitsOf(s->scoreDocuments(q, longer)[0]) == bitsOf(hostMaxSim(q, longer[0], form)) && g_last_dim == 12 && g_calls == 1);
        CHECK(bitsOf(s->scoreDocuments(q, shorter)[0]) == bitsOf(hostMaxSim(q, shorter[0], form)) && g_last_dim == 7 && g_calls == 2);
        const std::vector<ColbertEmbeddings> both = {longer[0], shorter[0], ramp(2, 20, 4.0f)};
        g_calls = 0;
        const std::vector<float> got = s->scoreDocuments(q, both);
        CHECK(g_calls == 2 && s->hostScores() == 0);
        for (size_t i = 0; i < both.size(); ++i) CHECK(bitsOf(got[i]) == bitsOf(hostMaxSim(q, both[i], form)));
    }
    {   // ---- a refusal: the host's own function; an empty query; an empty window ----
        auto s = AccelColbertReranker::over(&g_standin, hostOf(0));
        const ColbertEmbeddings q = ramp(3, 8, 0.5f), none;
        const std::vector<ColbertEmbeddings> docs = {ramp(4, 8, 1.0f), ramp(1, 8, 2.0f)};
        g_refuse = true; g_host_calls = 0;
        const std::vector<float> got = s->scoreDocuments(q, docs);
        g_refuse = false;
        CHECK(g_host_calls == 2 && bitsOf(got[0]) == bitsOf(hostMaxSim(q, docs[0], 0)));
        const std::vector<float> zero = s->scoreDocuments(none, docs);
        CHECK(zero.size() == 2 && bitsOf(zero[0]) == 0u && bitsOf(zero[1]) == 0u);
        CHECK(s->scoreDocuments(q, {}).empty());
        // pooling: served, a short token refused, a refusal mapped
        const auto pooled = s->poolAndNormalize(docs, 8);
        CHECK(pooled.has_value() && pooled.value().size() == 2 && pooled.value()[0].size() == 8);
        std::vector<float> rows;
        for (const auto& t : docs[0].token_embeddings) rows.insert(rows.end(), t.begin(), t.end());
        const std::uint64_t off[2] = {0, 4};
        std::vector<float> want(8);
        rerank_oracle_maxpool(rows.data(), 8, off, 1, want.data());
        CHECK(sameScores(pooled.value()[0], want));
        CHECK(s->poolAndNormalize(docs, 6).has_value() && s->poolAndNormalize(docs, 6).value()[1].size() == 6);
        const auto shortTok = s->poolAndNormalize(docs, 9);
        CHECK(!shortTok.has_value() && shortTok.error().code == yams::ErrorCode::NotImplemented);
        g_refuse = true;
        const auto refused = s->poolAndNormalize(docs, 8);
        g_refuse = false;
        CHECK(!refused.has_value());
        const std::vector<ColbertEmbeddings> empty = {none};
        const auto zeros = s->poolAndNormalize(empty, 4);
        CHECK(zeros.has_value() && zeros.value()[0] == std::vector<float>(4, 0.0f));
    }
    std::printf("selftest OK\n");
    return 0;
}
#endif

} // namespace

int main(int argc, char** argv) {
    bool fused = false;
    const char* pluginPath = nullptr;
    const char* casePath = nullptr;
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
#ifndef RERANK_WITH_REFERENCE
        if (arg == "--selftest") return selftest();
#endif
        if (arg == "--fused") fused = true;
        else if (arg == "--plugin" && i + 1 < argc) pluginPath = argv[++i];
        else casePath = argv[i];
    }
    if (!casePath) { std::fprintf(stderr, "usage: rerank_shell_test [--fused] [--plugin <lib>] <cases> | --selftest\n"); return 2; }
    Reader rd;
    {
        FILE* f = std::fopen(casePath, "rb");
        if (!f) return 2;
        std::fseek(f, 0, SEEK_END);
        rd.bytes.resize(static_cast<size_t>(std::ftell(f)));
        std::fseek(f, 0, SEEK_SET);
        const size_t got = std::fread(rd.bytes.data(), 1, rd.bytes.size(), f);
        std::fclose(f);
        if (got != rd.bytes.size()) return 2;
    }
#ifdef RERANK_WITH_REFERENCE
    (void)fused; (void)pluginPath;
    ReferenceImpl ref;
    std::printf("probe -\n");
#else
    std::shared_ptr<yams::accel::Plugin> plugin;
    std::unique_ptr<AccelColbertReranker> shell;
    if (pluginPath) {
        auto p = yams::accel::Plugin::load(pluginPath, "{\"device\":0}");
        if (!p.has_value()) { std::fprintf(stderr, "plugin: %s\n", p.error().message.c_str()); return 3; }
        plugin = p.value();
        auto s = AccelColbertReranker::create(plugin, hostOf(fused ? 1u : 0u));
        if (!s.has_value()) return 3;
        shell = std::move(s.value());
    } else {
        shell = AccelColbertReranker::over(&g_standin, hostOf(fused ? 1u : 0u));
    }
    std::printf("probe %s\n", !shell->form() ? "neither" : *shell->form() == DotForm::Fused ? "fused" : "separate");
#endif
    const std::uint32_t count = rd.u32();
    for (std::uint32_t c = 0; c < count; ++c) {
        const std::uint32_t kind = rd.u32();
        std::vector<float> out;
        if (kind == 0) {
            const std::uint32_t dq = rd.u32(), tq = rd.u32(), dd = rd.u32(), nDocs = rd.u32();
            const ColbertEmbeddings query = rd.tokens(tq, dq);
            std::vector<ColbertEmbeddings> docs;
            for (std::uint32_t d = 0; d < nDocs; ++d) {
                const std::uint32_t len = rd.u32();
                docs.push_back(rd.tokens(len, dd));
            }
#ifdef RERANK_WITH_REFERENCE
            for (const auto& docEmb : docs) out.push_back(ref.computeMaxSim(query, docEmb));
#else
            out = shell->scoreDocuments(query, docs);
#endif
        } else {
            const std::uint32_t dim = rd.u32(), nDocs = rd.u32();
            std::vector<ColbertEmbeddings> docs;
            for (std::uint32_t d = 0; d < nDocs; ++d) {
                const std::uint32_t len = rd.u32();
                docs.push_back(rd.tokens(len, dim));
            }
#ifdef RERANK_WITH_REFERENCE
            for (const auto& doc : docs) {
                auto pooled = ref.maxPoolEmbeddings(doc, dim);
                ref.normalizeEmbedding(pooled);
                out.insert(out.end(), pooled.begin(), pooled.end());
            }
#else
            const auto pooled = shell->poolAndNormalize(docs, dim);
            if (!pooled.has_value()) { std::fprintf(stderr, "case %u: %s\n", c, pooled.error().message.c_str()); return 4; }
            for (const auto& v : pooled.value()) out.insert(out.end(), v.begin(), v.end());
#endif
        }
        printCase(c, out);
    }
#ifndef RERANK_WITH_REFERENCE
    if (!pluginPath && shell->hostScores() != 0) { std::fprintf(stderr, "the stand-in run fell back to the host function\n"); return 5; }
    if (pluginPath && shell->hostScores() != 0) { std::fprintf(stderr, "the plugin refused a call: the host function served it\n"); return 5; }
#endif
    return 0;
}
