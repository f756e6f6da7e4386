// persistence_shell_test — drives include/yams_accel/topological_quality.hpp (AccelTopologicalQuality) on case files
// (tests/_persistence_oracle.py write_case: uint32 m, uint32 dim, m * dim floats) and prints, per case, the bits of the value
// from both overloads.
//   persistence_shell_test [--fused] <case>...                 the shell over a stand-in table (the restatement of
//                                                              persistence_oracle.cpp): runs anywhere, also under ASan / UBSan
//   persistence_shell_test [--fused] --plugin <lib> <case>...  the same through the real topology_quality_v1
//   persistence_shell_test --selftest                          the shell's own rules over the stand-in: early returns, ragged
//                                                              rows, the probe's three answers, a refusal
//   built with -DPERSISTENCE_WITH_REFERENCE and linked with the reference's own topological_quality.cpp: the REFERENCE'S
//   computePersistenceH0 is called instead of the shell, and the chain form its build has is probed and printed.
//   tests/golden/make_persistence_golden.py makes the golden file from that build.
// The first line of output is `probe <separate|fused|neither>`: the form of the function that computes the values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <yams_accel/topological_quality.hpp>
#ifdef PERSISTENCE_WITH_REFERENCE
#include <yams/search/topological_quality.h>
#endif

#include "persistence_oracle.cpp"

using yams::search::AccelTopologicalQuality;
using yams::search::ChainForm;

namespace {

int g_calls = 0;
bool g_refuse = false;

// the stand-in table: the flat entry's limits and statuses, the restatement's arithmetic
yams_status_t standin_h0(void* self, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select, uint32_t form,
                         yams_persistence_h0_t* out, double** out_distances, double** out_merge_weights) {
    (void)self;
    ++g_calls;
    if (g_refuse) return YAMS_ERR_RESOURCE_EXHAUSTED;
    const uint64_t m = select ? n_select : n;
    if (m > YAMS_QUALITY_MAX_POINTS || dim > YAMS_CLUSTER_MAX_DIM || n >= (1ull << 31)) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0 || !out || (m && !rows) || form > YAMS_RESIDUAL_FUSED) return YAMS_ERR_INVALID_ARG;
    std::vector<float> points(static_cast<size_t>(m) * dim);
    for (uint64_t i = 0; i < m; ++i) {
        const uint64_t row = select ? select[i] : i;
        if (row >= n) return YAMS_ERR_INVALID_ARG;
        std::memcpy(points.data() + i * dim, rows + row * dim, static_cast<size_t>(dim) * 4);
    }
    for (const float v : points)
        if (!(v - v == 0.0f)) return YAMS_ERR_INVALID_ARG;
    *out = yams_persistence_h0_t{};
    out->n_points = static_cast<uint32_t>(m);
    out->n_edges = m < 2 ? 0 : m * (m - 1) / 2;
    out->n_merges = static_cast<uint32_t>(persistence_oracle(points.data(), m, dim, form == YAMS_RESIDUAL_FUSED, nullptr, nullptr, &out->norm,
                                                             &out->norm_index, &out->value));
    if (out_distances) *out_distances = nullptr;
    if (out_merge_weights) *out_merge_weights = nullptr;
    return YAMS_OK;
}
void standin_free(void*, double* a, double* b) { std::free(a); std::free(b); }
yams_topology_quality_v1 g_standin = {YAMS_IFACE_TOPOLOGY_QUALITY_V1_VERSION, nullptr, standin_h0, standin_free};

double oracleValue(std::span<const float> e, std::size_t count, std::size_t dim, int fused) {
    double norm, value; std::uint64_t idx;
    persistence_oracle(e.data(), count, static_cast<std::uint32_t>(dim), fused, nullptr, nullptr, &norm, &idx, &value);
    return value;
}
std::uint64_t bitsOf(double v) { std::uint64_t b; std::memcpy(&b, &v, 8); return b; }

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
    std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int selftest() {
    auto shell = AccelTopologicalQuality::over(&g_standin, ChainForm::Separate);
    const std::vector<float> six = {0.f, 0.f, 3.f, 4.f, 6.f, 8.5f};
    // the early returns: no call reaches the table
    g_calls = 0;
    CHECK(shell->computePersistenceH0(std::span<const float>(six), 1, 2).value() == 0.0, "count 1");
    CHECK(shell->computePersistenceH0(std::span<const float>(six), 0, 2).value() == 0.0, "count 0");
    CHECK(shell->computePersistenceH0(std::span<const float>(six), 3, 0).value() == 0.0, "dim 0");
    CHECK(shell->computePersistenceH0(std::span<const float>(six), 4, 2).value() == 0.0, "a span shorter than count * dim");
    CHECK(shell->computePersistenceH0(std::vector<std::vector<float>>{}).value() == 0.0, "empty outer vector");
    CHECK(shell->computePersistenceH0(std::vector<std::vector<float>>{{}, {}}).value() == 0.0, "rows of size 0");
    CHECK(shell->computePersistenceH0(std::vector<std::vector<float>>{{0.f, 0.f}, {3.f, 4.f}, {6.f}}).value() == 0.0, "ragged rows");
    CHECK(shell->computePersistenceH0(std::vector<std::vector<float>>{{1.f, 2.f}}).value() == 0.0, "one row");
    CHECK(g_calls == 0, "an early return called the table %d times", g_calls);
    // three points: 5, 5.85..., 10.59...; value = 5 / the middle distance
    const auto flat = shell->computePersistenceH0(std::span<const float>(six), 3, 2);
    const auto nested = shell->computePersistenceH0(std::vector<std::vector<float>>{{0.f, 0.f}, {3.f, 4.f}, {6.f, 8.5f}});
    CHECK(flat.has_value() && nested.has_value() && g_calls == 2, "calls %d", g_calls);
    CHECK(bitsOf(flat.value()) == bitsOf(oracleValue(six, 3, 2, 0)) && bitsOf(nested.value()) == bitsOf(flat.value()), "value");
    CHECK(flat.value() > 0.0 && flat.value() < 1.0, "value %g", flat.value());
    // a span longer than count * dim is read up to count * dim
    CHECK(bitsOf(shell->computePersistenceH0(std::span<const float>(six), 2, 2).value()) == bitsOf(0.0), "two points");
    // the probe: each form, and a host that is neither
    const auto sep = AccelTopologicalQuality::probeChainForm([](std::span<const float> e, std::size_t c, std::size_t d) { return oracleValue(e, c, d, 0); });
    const auto fus = AccelTopologicalQuality::probeChainForm([](std::span<const float> e, std::size_t c, std::size_t d) { return oracleValue(e, c, d, 1); });
    const auto non = AccelTopologicalQuality::probeChainForm([](std::span<const float> e, std::size_t c, std::size_t d) {
        return static_cast<double>(static_cast<float>(oracleValue(e, c, d, 0)));      // a float build: neither
    });
    const auto mix = AccelTopologicalQuality::probeChainForm([n = 0](std::span<const float> e, std::size_t c, std::size_t d) mutable {
        return oracleValue(e, c, d, n++ == 0 ? 0 : 1);      // one case one way, the others the other way: neither
    });
    CHECK(sep.has_value() && sep.value() == ChainForm::Separate, "separate probe");
    CHECK(fus.has_value() && fus.value() == ChainForm::Fused, "fused probe");
    CHECK(!non.has_value() && non.error().code == yams::ErrorCode::NotSupported, "a float build is taken");
    CHECK(!mix.has_value(), "a mixed build is taken");
    for (int k = 0; k < yams::search::quality_probe::kCases; ++k) {      // the recorded answers are the restatement's
        float p[6];
        std::memcpy(p, yams::search::quality_probe::kPoints[k], sizeof p);
        for (int f = 0; f < 2; ++f)
            CHECK(bitsOf(oracleValue(std::span<const float>(p, 6), 3, 2, f)) == yams::search::quality_probe::kValue[k][f], "probe case %d form %d", k, f);
        CHECK(yams::search::quality_probe::kValue[k][0] != yams::search::quality_probe::kValue[k][1], "probe case %d tells nothing", k);
    }
    // refusals come back as Errors
    g_refuse = true;
    const auto refused = shell->computePersistenceH0(std::span<const float>(six), 3, 2);
    g_refuse = false;
    CHECK(!refused.has_value() && refused.error().code == yams::ErrorCode::ResourceExhausted, "refusal");
    std::vector<float> bad = six;
    bad[3] = INFINITY;
    const auto nonfinite = shell->computePersistenceH0(std::span<const float>(bad), 3, 2);
    CHECK(!nonfinite.has_value() && nonfinite.error().code == yams::ErrorCode::InvalidArgument, "non-finite");
    g_calls = 0;
    const std::vector<float> wide(static_cast<size_t>(YAMS_QUALITY_MAX_POINTS) + 1, 1.0f);
    const auto many = shell->computePersistenceH0(std::span<const float>(wide), wide.size(), 1);
    CHECK(!many.has_value() && many.error().code == yams::ErrorCode::NotImplemented && g_calls == 0, "beyond the range");
    // the fused shell asks for the fused form
    auto fusedShell = AccelTopologicalQuality::over(&g_standin, ChainForm::Fused);
    float p[6];
    std::memcpy(p, yams::search::quality_probe::kPoints[0], sizeof p);
    CHECK(bitsOf(fusedShell->computePersistenceH0(std::span<const float>(p, 6), 3, 2).value()) == yams::search::quality_probe::kValue[0][1], "fused shell");
    CHECK(bitsOf(shell->computePersistenceH0(std::span<const float>(p, 6), 3, 2).value()) == yams::search::quality_probe::kValue[0][0], "separate shell");
    std::printf("selftest ok\n");
    return 0;
}

} // namespace

int main(int argc, char** argv) {
    bool fused = false;
    const char* pluginPath = nullptr;
    std::vector<const char*> cases;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--selftest") return selftest();
        if (a == "--fused") fused = true;
        else if (a == "--plugin" && i + 1 < argc) pluginPath = argv[++i];
        else cases.push_back(argv[i]);
    }
    if (cases.empty()) { std::fprintf(stderr, "usage: persistence_shell_test [--fused] [--plugin <lib>] <case>... | --selftest\n"); return 2; }
    const ChainForm form = fused ? ChainForm::Fused : ChainForm::Separate;
#ifdef PERSISTENCE_WITH_REFERENCE
    (void)form; (void)pluginPath;
    const auto probe = AccelTopologicalQuality::probeChainForm(
        [](std::span<const float> e, std::size_t c, std::size_t d) { return yams::search::computePersistenceH0(e, c, d); });
#else
    std::shared_ptr<yams::accel::Plugin> plugin;
    std::unique_ptr<AccelTopologicalQuality> shell;
    if (pluginPath) {
        auto p = yams::accel::Plugin::load(pluginPath, "{\"device\":0}");
        if (!p.has_value()) { std::fprintf(stderr, "plugin: %s\n", p.error().message.c_str()); return 3; }
        plugin = p.value();
        auto s = AccelTopologicalQuality::create(plugin, form);
        if (!s.has_value()) return 3;
        shell = std::move(s.value());
    } else {
        shell = AccelTopologicalQuality::over(&g_standin, form);
    }
    // the function behind the values is the shell itself: its form is what the probe must report
    const auto probe = AccelTopologicalQuality::probeChainForm([&](std::span<const float> e, std::size_t c, std::size_t d) {
        const auto r = shell->computePersistenceH0(e, c, d);
        return r.has_value() ? r.value() : -1.0;
    });
#endif
    std::printf("probe %s\n", !probe.has_value() ? "neither" : (probe.value() == ChainForm::Fused ? "fused" : "separate"));
    for (const char* path : cases) {
        FILE* f = std::fopen(path, "rb");
        if (!f) return 2;
        uint32_t shape[2];
        if (std::fread(shape, 4, 2, f) != 2) return 2;
        std::vector<float> x(static_cast<size_t>(shape[0]) * shape[1]);
        if (!x.empty() && std::fread(x.data(), 4, x.size(), f) != x.size()) return 2;
        std::fclose(f);
        std::vector<std::vector<float>> nested(shape[0]);
        for (uint32_t i = 0; i < shape[0]; ++i) nested[i].assign(x.begin() + static_cast<size_t>(i) * shape[1], x.begin() + static_cast<size_t>(i + 1) * shape[1]);
#ifdef PERSISTENCE_WITH_REFERENCE
        const double a = yams::search::computePersistenceH0(std::span<const float>(x), shape[0], shape[1]);
        const double b = yams::search::computePersistenceH0(nested);
#else
        const auto ra = shell->computePersistenceH0(std::span<const float>(x), shape[0], shape[1]);
        const auto rb = shell->computePersistenceH0(nested);
        if (!ra.has_value() || !rb.has_value()) { std::fprintf(stderr, "%s: %s\n", path, (ra.has_value() ? rb : ra).error().message.c_str()); return 4; }
        const double a = ra.value(), b = rb.value();
#endif
        std::printf("value %016llx %016llx\n", static_cast<unsigned long long>(bitsOf(a)), static_cast<unsigned long long>(bitsOf(b)));
    }
    return 0;
}
