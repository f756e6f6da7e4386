// features_shell_test — drives include/yams_accel/topology_features.hpp (AccelTopologyFeatures) on a case file
// (tests/_features_oracle.py write_cases) and prints, per case, the bits of every output vector.
//   features_shell_test [--fused] <cases>                 the shell over a stand-in table (the restatement of
//                                                         features_oracle.cpp): runs anywhere, also under ASan / UBSan
//   features_shell_test [--fused] --plugin <lib> <cases>  the same through the real topology_features_v1
//   features_shell_test --selftest                        the shell's own rules over the stand-in: admissions, early returns,
//                                                         the NaN variance, the probe's three answers, refusals
//   built with -DFEATURES_WITH_REFERENCE, the reference's own topology_input_extractor.cpp on the include path: the
//   REFERENCE'S functions are called instead of the shell (tests/golden/make_features_golden.py makes the golden file from
//   that build; it prints `probe -` and the generator judges the form from the recorded samples).
// Output: `probe <separate|fused|neither|->`, then per case a line `case` and one line `vec <hex of the floats' bytes>` per
// output vector (`vec -` for an empty one).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#ifdef FEATURES_WITH_REFERENCE
#include "topology_input_extractor.cpp"      // the reference's translation unit, as it is (found on the include path)
#else
#include <yams_accel/topology_features.hpp>
#include "features_oracle.cpp"
#endif

namespace {

struct Reader {
    std::vector<unsigned char> bytes; size_t at = 0;
    bool done() const { return at >= bytes.size(); }
    std::uint32_t u32() { std::uint32_t v; std::memcpy(&v, bytes.data() + at, 4); at += 4; return v; }
    float f32() { float v; std::memcpy(&v, bytes.data() + at, 4); at += 4; return v; }
    std::vector<float> floats() { std::vector<float> v(u32()); if (!v.empty()) std::memcpy(v.data(), bytes.data() + at, v.size() * 4); at += v.size() * 4; return v; }
    std::vector<std::uint32_t> words() { std::vector<std::uint32_t> v(u32()); if (!v.empty()) std::memcpy(v.data(), bytes.data() + at, v.size() * 4); at += v.size() * 4; return v; }
};

void printVec(const std::vector<float>& v) {
    if (v.empty()) { std::printf("vec -\n"); return; }
    std::printf("vec ");
    for (const float x : v) {
        unsigned char b[4];
        std::memcpy(b, &x, 4);
        std::printf("%02x%02x%02x%02x", b[0], b[1], b[2], b[3]);
    }
    std::printf("\n");
}

struct AggregateCase { std::vector<std::vector<std::pair<std::uint32_t, std::vector<float>>>> docs; };
struct VarianceCase { std::uint32_t target; std::vector<std::vector<float>> sample; };
struct ComposeCase {
    std::uint32_t entity, matryoshka, target, minhash, sketchDim; float alphaE, alphaM;
    std::vector<float> weights; std::vector<std::vector<float>> dense, entitySig; std::vector<std::vector<std::uint32_t>> sig;
};

#ifndef FEATURES_WITH_REFERENCE
using yams::topology::AccelTopologyFeatures;
using yams::topology::VarianceForm;

int g_calls = 0;
bool g_refuse = false;

// the stand-in table: the flat entries' limits and statuses, the restatement's arithmetic
yams_status_t standin_aggregate(void*, const float* rows, uint64_t n_records, uint32_t dim, const uint64_t* off, const uint32_t* records,
                                uint64_t n_docs, float* out, uint32_t* out_counts) {
    ++g_calls;
    if (g_refuse) return YAMS_ERR_RESOURCE_EXHAUSTED;
    if (dim > YAMS_FEATURES_MAX_DIM || n_records >= (1ull << 31) || n_docs >= (1ull << 31)) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0) return YAMS_ERR_INVALID_ARG;
    if (n_docs == 0) return YAMS_OK;
    if (!off || !out || !out_counts || off[0] != 0) return YAMS_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < n_docs; ++i)
        if (off[i + 1] < off[i]) return YAMS_ERR_INVALID_ARG;
    if (off[n_docs] && (!rows || !records)) return YAMS_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < off[n_docs]; ++i)
        if (records[i] >= n_records) return YAMS_ERR_INVALID_ARG;
    features_aggregate_oracle(rows, dim, off, records, n_docs, out, out_counts);
    return YAMS_OK;
}
yams_status_t standin_variance(void*, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select, uint32_t form,
                               double* out_mean, double* out_var) {
    ++g_calls;
    if (g_refuse) return YAMS_ERR_RESOURCE_EXHAUSTED;
    const uint64_t m = select ? n_select : n;
    if (dim > YAMS_FEATURES_MAX_DIM || n >= (1ull << 31) || m >= (1ull << 32)) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0 || form > YAMS_RESIDUAL_FUSED) return YAMS_ERR_INVALID_ARG;
    if (m == 0) return YAMS_OK;
    if (!rows || !out_mean || !out_var) return YAMS_ERR_INVALID_ARG;
    for (uint64_t i = 0; select && i < m; ++i)
        if (select[i] >= n) return YAMS_ERR_INVALID_ARG;
    features_variance_oracle(rows, dim, select, m, form == YAMS_RESIDUAL_FUSED, out_mean, out_var);
    return YAMS_OK;
}
yams_status_t standin_compose(void*, const float* dense, uint64_t n, uint32_t dim, const float* weights, const float* entity, uint32_t k,
                              const uint8_t* entity_on, const uint32_t* sig, uint32_t sig_len, const uint8_t* sketch_on, uint32_t sketch_dim,
                              float alpha_e, float alpha_m, float* out, uint32_t out_stride, uint32_t* out_dims) {
    ++g_calls;
    if (g_refuse) return YAMS_ERR_RESOURCE_EXHAUSTED;
    if (dim > YAMS_FEATURES_MAX_DIM || k > YAMS_FEATURES_MAX_DIM || sketch_dim > YAMS_FEATURES_MAX_DIM || sig_len > YAMS_FEATURES_MAX_SIG_LEN ||
        n >= (1ull << 31))
        return YAMS_ERR_UNSUPPORTED;
    if (dim == 0) return YAMS_ERR_INVALID_ARG;
    if (n == 0) return YAMS_OK;
    if (!dense || !out_dims || (out_stride && !out) || (entity && k && !entity_on) || (sig && sig_len && sketch_dim && !sketch_on))
        return YAMS_ERR_INVALID_ARG;
    std::vector<float> tmp(static_cast<size_t>(n) * out_stride);
    std::vector<uint32_t> dims(n);
    const uint32_t longest = features_compose_oracle(dense, n, dim, weights, entity, k, entity_on, sig, sig_len, sketch_on, sketch_dim, alpha_e,
                                                     alpha_m, tmp.data(), out_stride, dims.data());
    if (out_stride < longest) return YAMS_ERR_INVALID_ARG;
    if (!tmp.empty()) std::memcpy(out, tmp.data(), tmp.size() * 4);
    std::memcpy(out_dims, dims.data(), dims.size() * 4);
    return YAMS_OK;
}
yams_topology_features_v1 g_standin = {YAMS_IFACE_TOPOLOGY_FEATURES_V1_VERSION, nullptr, standin_aggregate, standin_variance, standin_compose};

// computeVarianceWeights restated over the oracle: what a host of the given form returns
std::vector<float> oracleWeights(const std::vector<std::vector<float>>& sample, std::size_t target, int fused) {
    if (sample.empty() || target == 0 || target >= sample.front().size()) return {};
    const std::size_t dim = sample.front().size();
    std::vector<float> rows;
    uint64_t m = 0;
    for (const auto& e : sample)
        if (e.size() == dim) { rows.insert(rows.end(), e.begin(), e.end()); ++m; }
    std::vector<double> mean(dim), var(dim);
    features_variance_oracle(rows.data(), static_cast<uint32_t>(dim), nullptr, m, fused, mean.data(), var.data());
    std::vector<float> w(dim);
    if (features_weights_oracle(var.data(), static_cast<uint32_t>(dim), static_cast<uint32_t>(target), w.data())) return {};
    return w;
}

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
    std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

bool sameBits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * 4) == 0);
}

int selftest() {
    using yams::topology::FeatureCompositionView;
    using yams::topology::FeatureRecord;
    auto shell = AccelTopologyFeatures::over(&g_standin, VarianceForm::Separate);
    const std::vector<float> a = {-0.0f, 1.0f, 2.0f}, b = {-0.0f, 3.0f, 5.0f}, c = {9.0f, 9.0f}, none;
    // aggregate: the admissions
    g_calls = 0;
    {
        const std::vector<std::vector<FeatureRecord>> docs = {
            {},
            {{false, a}},
            {{false, a}, {false, b}},
            {{false, a}, {true, c}, {false, b}},       // a document-level record short-circuits
            {{false, a}, {true, none}, {false, b}},    // an empty one does not
            {{false, none}, {false, a}, {false, c}, {false, b}},
            {{false, none}, {true, none}}};
        const auto r = shell->aggregateEmbeddings(docs);
        CHECK(r.has_value() && g_calls == 1, "calls %d", g_calls);
        const auto& v = r.value();
        CHECK(v[0].empty() && v[6].empty(), "documents without a contributing record");
        CHECK(sameBits(v[1], a), "one record is assigned: -0.0f stays");
        CHECK(sameBits(v[2], {-0.0f, 2.0f, 3.5f}), "two records");
        CHECK(sameBits(v[3], c), "the short-circuit");
        CHECK(sameBits(v[4], v[2]) && sameBits(v[5], v[2]), "empty and ragged records are skipped");
        g_calls = 0;
        const std::vector<std::vector<FeatureRecord>> two = {{{false, a}}, {{false, c}, {false, c}}};      // two sizes: two calls
        const auto r2 = shell->aggregateEmbeddings(two);
        CHECK(r2.has_value() && g_calls == 2 && sameBits(r2.value()[0], a) && sameBits(r2.value()[1], c), "one call per size");
        g_calls = 0;
        CHECK(shell->aggregateEmbeddings({}).value().empty() && g_calls == 0, "no documents, no call");
    }
    // the sample cap
    {
        std::vector<std::vector<float>> docs(5000, std::vector<float>{1.0f});
        docs[3].clear();
        const auto s = AccelTopologyFeatures::collectVarianceSample(docs);
        CHECK(s.size() == AccelTopologyFeatures::kVarianceSampleCap, "cap %zu", s.size());
    }
    // computeVarianceWeights: the early returns reach no table
    const std::vector<std::vector<float>> sample = {{1.f, 5.f, 2.f, 7.f}, {2.f, 1.f, 2.f, 9.5f}, {4.f, 4.f}, {0.f, 3.f, 2.f, 8.f}};
    g_calls = 0;
    CHECK(shell->computeVarianceWeights({}, 2).value().empty(), "no embeddings");
    CHECK(shell->computeVarianceWeights(sample, 0).value().empty(), "target 0");
    CHECK(shell->computeVarianceWeights(sample, 4).value().empty() && shell->computeVarianceWeights(sample, 9).value().empty(), "target >= dim");
    CHECK(g_calls == 0, "an early return called the table %d times", g_calls);
    {
        const auto w = shell->computeVarianceWeights(sample, 2);
        CHECK(w.has_value() && g_calls == 1 && sameBits(w.value(), oracleWeights(sample, 2, 0)), "weights");
        CHECK(w.value()[0] == 0.0f && w.value()[1] > 0.0f && w.value()[2] == 0.0f && w.value()[3] > 0.0f, "the kept dimensions");
        const std::vector<std::vector<float>> flat = {{1.f, 2.f, 2.f, 3.f}, {2.f, 2.f, 2.f, 3.f}, {0.f, 2.f, 2.f, 3.f}};
        const auto z = shell->computeVarianceWeights(flat, 2);      // a zero variance inside the top 2: its weight is 0
        CHECK(z.has_value() && z.value()[0] > 0.0f && z.value()[1] == 0.0f && z.value()[2] == 0.0f && z.value()[3] == 0.0f, "zero variance inside the target");
        std::vector<std::vector<float>> bad = sample;
        bad[1][3] = INFINITY;      // inf - inf: a NaN variance
        const auto n = shell->computeVarianceWeights(bad, 2);
        CHECK(!n.has_value() && n.error().code == yams::ErrorCode::InvalidArgument, "a NaN variance is sorted");
    }
    // the probe: each form, and a host that is neither
    const auto sep = AccelTopologyFeatures::probeVarianceForm([](const std::vector<std::vector<float>>& s, std::size_t t) { return oracleWeights(s, t, 0); });
    const auto fus = AccelTopologyFeatures::probeVarianceForm([](const std::vector<std::vector<float>>& s, std::size_t t) { return oracleWeights(s, t, 1); });
    const auto non = AccelTopologyFeatures::probeVarianceForm([](const std::vector<std::vector<float>>&, std::size_t) { return std::vector<float>{}; });
    const auto mix = AccelTopologyFeatures::probeVarianceForm([n = 0](const std::vector<std::vector<float>>& s, std::size_t t) mutable {
        return oracleWeights(s, t, n++ == 0 ? 0 : 1);
    });
    CHECK(sep.has_value() && sep.value() == VarianceForm::Separate, "separate probe");
    CHECK(fus.has_value() && fus.value() == VarianceForm::Fused, "fused probe");
    CHECK(!non.has_value() && non.error().code == yams::ErrorCode::NotSupported && !mix.has_value(), "neither");
    for (int k = 0; k < yams::topology::features_probe::kCases; ++k) {      // the recorded answers are the restatement's, and differ
        std::vector<std::vector<float>> s(3, std::vector<float>(2));
        for (int r = 0; r < 3; ++r) std::memcpy(s[r].data(), &yams::topology::features_probe::kRows[k][2 * r], 8);
        for (int f = 0; f < 2; ++f) {
            const auto w = oracleWeights(s, 1, f);
            CHECK(w.size() == 2 && std::memcmp(w.data(), yams::topology::features_probe::kWeights[k][f], 8) == 0, "probe case %d form %d", k, f);
        }
        CHECK(std::memcmp(yams::topology::features_probe::kWeights[k][0], yams::topology::features_probe::kWeights[k][1], 8) != 0, "case %d tells nothing", k);
        auto fusedShell = AccelTopologyFeatures::over(&g_standin, VarianceForm::Fused);
        CHECK(sameBits(fusedShell->computeVarianceWeights(s, 1).value(), oracleWeights(s, 1, 1)) &&
              sameBits(shell->computeVarianceWeights(s, 1).value(), oracleWeights(s, 1, 0)), "the shell asks for its form");
    }
    // compose: the conditions
    {
        const std::vector<std::vector<float>> dense = {{3.f, 0.f, 4.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        FeatureCompositionView cfg;
        g_calls = 0;
        const auto plain = shell->composeFeatureVectors(dense, {}, {}, {}, cfg);
        CHECK(plain.has_value() && g_calls == 1 && sameBits(plain.value()[0], {0.6f, 0.f, 0.8f, 0.f}) && sameBits(plain.value()[1], dense[1]), "normalised");
        cfg.enableMatryoshkaCoarseView = true;
        cfg.matryoshkaTargetDim = 2;
        const std::vector<float> w = {2.f, 0.f, 1.f, 0.f}, wrong = {1.f, 1.f};
        const auto coarse = shell->composeFeatureVectors(dense, w, {}, {}, cfg);
        CHECK(coarse.has_value() && coarse.value()[0].size() == 2 && coarse.value()[1].size() == 2, "kept 2");
        g_calls = 0;
        const auto raw = shell->composeFeatureVectors(dense, wrong, {}, {}, cfg);      // :169-171: un-normalised, no call
        CHECK(raw.has_value() && g_calls == 0 && sameBits(raw.value()[0], dense[0]), "weights of another size");
        cfg.enableEntityFusion = true;
        const std::vector<std::vector<float>> ent = {{1.f, 0.f}, {}};
        const auto mixed = shell->composeFeatureVectors(dense, wrong, ent, {}, cfg);
        CHECK(!mixed.has_value() && mixed.error().code == yams::ErrorCode::NotImplemented, "weights of another size with a part on");
        cfg.matryoshkaTargetDim = 4;      // :353-354: target >= dim: matryoshka off, dense normalised
        const auto fusedRow = shell->composeFeatureVectors(dense, w, ent, {}, cfg);
        CHECK(fusedRow.has_value() && fusedRow.value()[0].size() == 6 && fusedRow.value()[1].size() == 4, "entity on one row");
        CHECK(sameBits(fusedRow.value()[0], {0.6f * 0.75f, 0.f, 0.8f * 0.75f, 0.f, 0.25f, 0.f}), "the concatenation");
        cfg.enableMinHashSketch = true;
        cfg.minhashSketchDim = 3;
        const std::vector<std::vector<std::uint32_t>> sig = {{}, {0u, 3u, 6u, 1u}};
        const auto both = shell->composeFeatureVectors(dense, w, ent, sig, cfg);
        CHECK(both.has_value() && both.value()[0].size() == 6 && both.value()[1].size() == 7, "sketch on the other row");
        CHECK(shell->composeFeatureVectors({}, w, {}, {}, cfg).value().empty(), "no rows");
        CHECK(!shell->composeFeatureVectors({{1.f}, {1.f, 2.f}}, {}, {}, {}, cfg).has_value(), "ragged dense");
    }
    // refusals come back as Errors
    g_refuse = true;
    const auto refused = shell->computeVarianceWeights(sample, 2);
    const auto refusedAgg = shell->aggregateEmbeddings({{{false, a}}});
    g_refuse = false;
    CHECK(!refused.has_value() && refused.error().code == yams::ErrorCode::ResourceExhausted && !refusedAgg.has_value(), "refusal");
    g_calls = 0;
    const std::vector<std::vector<float>> wide(2, std::vector<float>(YAMS_FEATURES_MAX_DIM + 1, 1.0f));
    const auto beyond = shell->computeVarianceWeights(wide, 3);
    CHECK(!beyond.has_value() && beyond.error().code == yams::ErrorCode::NotImplemented && g_calls == 0, "beyond the range");
    std::printf("selftest ok\n");
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
#ifndef FEATURES_WITH_REFERENCE
        if (arg == "--selftest") return selftest();
#endif
        if (arg == "--fused") fused = true;
        else if (arg == "--plugin" && i + 1 < argc) pluginPath = argv[++i];
        else casePath = argv[i];
    }
    if (!casePath) { std::fprintf(stderr, "usage: features_shell_test [--fused] [--plugin <lib>] <cases> | --selftest\n"); return 2; }
    Reader rd;
    {
        FILE* f = std::fopen(casePath, "rb");
        if (!f) return 2;
        std::fseek(f, 0, SEEK_END);
        rd.bytes.resize(static_cast<size_t>(std::ftell(f)));
        std::fseek(f, 0, SEEK_SET);
        if (!rd.bytes.empty() && std::fread(rd.bytes.data(), 1, rd.bytes.size(), f) != rd.bytes.size()) return 2;
        std::fclose(f);
    }
#ifdef FEATURES_WITH_REFERENCE
    (void)fused; (void)pluginPath;
    std::printf("probe -\n");
#else
    const VarianceForm form = fused ? VarianceForm::Fused : VarianceForm::Separate;
    std::shared_ptr<yams::accel::Plugin> plugin;
    std::unique_ptr<AccelTopologyFeatures> shell;
    if (pluginPath) {
        auto p = yams::accel::Plugin::load(pluginPath, "{\"device\":0}");
        if (!p.has_value()) { std::fprintf(stderr, "plugin: %s\n", p.error().message.c_str()); return 3; }
        plugin = p.value();
        auto s = AccelTopologyFeatures::create(plugin, form);
        if (!s.has_value()) return 3;
        shell = std::move(s.value());
    } else {
        shell = AccelTopologyFeatures::over(&g_standin, form);
    }
    // the function behind the values is the shell itself: its form is what the probe must report
    const auto probe = AccelTopologyFeatures::probeVarianceForm([&](const std::vector<std::vector<float>>& s, std::size_t t) {
        const auto r = shell->computeVarianceWeights(s, t);
        return r.has_value() ? r.value() : std::vector<float>{};
    });
    std::printf("probe %s\n", !probe.has_value() ? "neither" : (probe.value() == VarianceForm::Fused ? "fused" : "separate"));
#endif
    while (!rd.done()) {
        const std::uint32_t kind = rd.u32();
        std::printf("case\n");
        if (kind == 'A') {
            AggregateCase ac;
            ac.docs.resize(rd.u32());
            for (auto& doc : ac.docs) {
                doc.resize(rd.u32());
                for (auto& rec : doc) { rec.first = rd.u32(); rec.second = rd.floats(); }
            }
#ifdef FEATURES_WITH_REFERENCE
            for (const auto& doc : ac.docs) {
                std::vector<yams::vector::VectorRecord> records(doc.size());
                for (size_t i = 0; i < doc.size(); ++i) {
                    records[i].level = doc[i].first ? yams::vector::EmbeddingLevel::DOCUMENT : yams::vector::EmbeddingLevel::CHUNK;
                    records[i].embedding = doc[i].second;
                }
                printVec(yams::topology::aggregateEmbedding(records));
            }
#else
            std::vector<std::vector<yams::topology::FeatureRecord>> docs(ac.docs.size());
            for (size_t d = 0; d < ac.docs.size(); ++d)
                for (const auto& rec : ac.docs[d]) docs[d].push_back({rec.first != 0, rec.second});
            const auto r = shell->aggregateEmbeddings(docs);
            if (!r.has_value()) { std::fprintf(stderr, "aggregate: %s\n", r.error().message.c_str()); return 4; }
            for (const auto& v : r.value()) printVec(v);
#endif
        } else if (kind == 'V') {
            VarianceCase vc;
            vc.target = rd.u32();
            vc.sample.resize(rd.u32());
            for (auto& e : vc.sample) e = rd.floats();
#ifdef FEATURES_WITH_REFERENCE
            printVec(yams::topology::computeVarianceWeights(vc.sample, vc.target));
#else
            const auto r = shell->computeVarianceWeights(vc.sample, vc.target);
            if (!r.has_value()) { std::fprintf(stderr, "variance: %s\n", r.error().message.c_str()); return 4; }
            printVec(r.value());
#endif
        } else if (kind == 'C') {
            ComposeCase cc;
            cc.entity = rd.u32(); cc.matryoshka = rd.u32(); cc.target = rd.u32(); cc.minhash = rd.u32(); cc.sketchDim = rd.u32();
            cc.alphaE = rd.f32(); cc.alphaM = rd.f32();
            cc.weights = rd.floats();
            const std::uint32_t n = rd.u32();
            for (std::uint32_t i = 0; i < n; ++i) {
                cc.dense.push_back(rd.floats());
                cc.entitySig.push_back(rd.floats());
                cc.sig.push_back(rd.words());
            }
#ifdef FEATURES_WITH_REFERENCE
            yams::topology::FeatureComposition cfg;
            cfg.enableEntityFusion = cc.entity != 0;
            cfg.entityFusionAlpha = cc.alphaE;
            cfg.enableMatryoshkaCoarseView = cc.matryoshka != 0;
            cfg.matryoshkaTargetDim = cc.target;
            cfg.enableMinHashSketch = cc.minhash != 0;
            cfg.minhashSketchDim = cc.sketchDim;
            cfg.minhashAlpha = cc.alphaM;
            for (std::uint32_t i = 0; i < n; ++i) {
                std::vector<float> sketch;      // extract, :676-690
                if (cfg.enableMinHashSketch && cfg.minhashSketchDim > 0 && !cc.sig[i].empty())
                    sketch = yams::topology::bucketCountSketch(cc.sig[i], cfg.minhashSketchDim);
                printVec(yams::topology::composeFeatureVector(cc.dense[i], cc.weights, cc.entitySig[i], sketch, cfg));
            }
#else
            yams::topology::FeatureCompositionView cfg;
            cfg.enableEntityFusion = cc.entity != 0;
            cfg.entityFusionAlpha = cc.alphaE;
            cfg.enableMatryoshkaCoarseView = cc.matryoshka != 0;
            cfg.matryoshkaTargetDim = cc.target;
            cfg.enableMinHashSketch = cc.minhash != 0;
            cfg.minhashSketchDim = cc.sketchDim;
            cfg.minhashAlpha = cc.alphaM;
            const auto r = shell->composeFeatureVectors(cc.dense, cc.weights, cc.entitySig, cc.sig, cfg);
            if (!r.has_value()) { std::fprintf(stderr, "compose: %s\n", r.error().message.c_str()); return 4; }
            for (const auto& v : r.value()) printVec(v);
#endif
        } else {
            std::fprintf(stderr, "unknown case kind %u\n", kind);
            return 2;
        }
    }
    return 0;
}
