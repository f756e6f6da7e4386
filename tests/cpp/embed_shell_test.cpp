// embed_shell_test — drives include/yams_accel/embedding_pool.hpp (AccelEmbeddingPooler) on a case file
// (tests/_embed_oracle.py write_cases) and prints, per case, the bits of its output.
//   embed_shell_test <cases>                   the shell over a stand-in table (the restatement of embed_oracle.cpp): runs
//                                              anywhere, also under ASan / UBSan
//   embed_shell_test --plugin <lib> <cases>    the same through the real embedding_pool_v1
//   embed_shell_test --host-loop <cases>       the loop the shell carries for what the device refuses (hostPool, hostNormalize),
//                                              alone: held to the golden file like every other door
//   embed_shell_test --selftest                the shell's own rules over the stand-in: ragged masks and a MEAN weight above 1
//                                              reach the host loop, everything else the table; result shape; error mapping
//   built with -DEMBED_WITH_REFERENCE and embed_ref_rank3.inc / embed_ref_rank2.inc on the include path (the reference's own
//   rank-3 batch block and rank-2 block, cut by tests/golden/make_embed_golden.py into its temporary directory): the
//   REFERENCE'S loops run instead of the shell.
// Output: per case one line `case <index> <hex of the floats' bytes>` (the rows one after the other), then `device_calls <n>`
// and `host_calls <n>`.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#ifdef EMBED_WITH_REFERENCE
namespace {
enum class Pooling { MEAN, CLS, MAX };      // the names the cut blocks use
std::vector<std::vector<float>> referenceRank3(const float* data, size_t B, size_t SS, size_t DD, const std::vector<std::vector<int32_t>>& masks,
                                               Pooling pooling_mode_, bool normalize_) {
    const size_t hidden_dim = DD;
    std::vector<std::vector<float>> result;
#include "embed_ref_rank3.inc"      // the reference's text
    return result;
}
std::vector<std::vector<float>> referenceRank2(const float* data, size_t B, size_t DD, bool normalize_) {
    std::vector<std::vector<float>> result;
#include "embed_ref_rank2.inc"      // the reference's text
    return result;
}
} // namespace
#else
#include <yams_accel/embedding_pool.hpp>
#include "embed_oracle.cpp"
using yams::embed::AccelEmbeddingPooler;
using yams::embed::HiddenStates;
using yams::embed::Pooling;
#endif

namespace {

struct Reader {
    std::vector<unsigned char> bytes; size_t at = 0;
    std::uint32_t u32() { std::uint32_t v; std::memcpy(&v, bytes.data() + at, 4); at += 4; return v; }
    template <typename T> std::vector<T> array(size_t n) {
        std::vector<T> v(n);
        if (n) std::memcpy(v.data(), bytes.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

void printCase(std::uint32_t index, const std::vector<std::vector<float>>& rows) {
    std::printf("case %u ", index);
    for (const auto& r : rows)
        for (const float x : r) {
            unsigned char b[4];
            std::memcpy(b, &x, 4);
            std::printf("%02x%02x%02x%02x", b[0], b[1], b[2], b[3]);
        }
    std::printf("\n");
}

Pooling poolingOf(std::uint32_t mode) { return mode == 0u ? Pooling::CLS : mode == 1u ? Pooling::MAX : Pooling::MEAN; }

#ifndef EMBED_WITH_REFERENCE
int g_calls = 0;
yams_status_t g_answer = YAMS_OK;      // what the stand-in says instead of serving

// the stand-in table: the flat entries' limits and statuses, the restatement's arithmetic
yams_status_t standin_pool(void*, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask, uint32_t mask_len,
                           uint32_t mode, uint32_t flags, float* out, yams_embed_diag_t* diag) {
    ++g_calls;
    if (g_answer != YAMS_OK) return g_answer;
    if (dim > YAMS_EMBED_MAX_DIM || seq > YAMS_EMBED_MAX_SEQ || batch > YAMS_EMBED_MAX_ROWS || batch * seq > YAMS_EMBED_MAX_ROWS) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0 || seq == 0 || mode > YAMS_EMBED_POOL_MEAN || (flags & ~YAMS_EMBED_NORMALIZE)) return YAMS_ERR_INVALID_ARG;
    if (batch == 0) return YAMS_OK;
    if (!hidden || !out || (!mask && mode != YAMS_EMBED_POOL_CLS && mask_len)) return YAMS_ERR_INVALID_ARG;
    if (mode == YAMS_EMBED_POOL_CLS) mask = nullptr;
    if (mask && mode == YAMS_EMBED_POOL_MEAN)
        for (uint64_t b = 0; b < batch; ++b)
            for (uint32_t i = 0; i < std::min(seq, mask_len); ++i)
                if (mask[b * mask_len + i] > 1) return YAMS_ERR_UNSUPPORTED;
    uint64_t counts[2];
    embed_oracle_pool(hidden, batch, seq, dim, mask, mask_len, mode, flags & YAMS_EMBED_NORMALIZE, nullptr, out, counts);
    if (diag) *diag = yams_embed_diag_t{mode, flags, batch, seq, dim, counts[0], counts[1], 64u, 0u};
    return YAMS_OK;
}
yams_status_t standin_normalize(void*, const float* rows, uint64_t batch, uint32_t dim, float* out) {
    ++g_calls;
    if (g_answer != YAMS_OK) return g_answer;
    if (dim > YAMS_EMBED_MAX_DIM || batch > YAMS_EMBED_MAX_ROWS) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0) return YAMS_ERR_INVALID_ARG;
    if (batch == 0) return YAMS_OK;
    if (!rows || !out) return YAMS_ERR_INVALID_ARG;
    embed_oracle_normalize(rows, batch, dim, out);
    return YAMS_OK;
}
yams_embedding_pool_v1 g_standin = {YAMS_IFACE_EMBEDDING_POOL_V1_VERSION, nullptr, standin_pool, standin_normalize, standin_pool, standin_normalize};

std::uint32_t bitsOf(float x) { std::uint32_t b; std::memcpy(&b, &x, 4); return b; }
bool sameRows(const std::vector<std::vector<float>>& a, const std::vector<std::vector<float>>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i].size() != b[i].size()) return false;
        for (size_t d = 0; d < a[i].size(); ++d)
            if (bitsOf(a[i][d]) != bitsOf(b[i][d]) && !(a[i][d] != a[i][d] && b[i][d] != b[i][d])) return false;
    }
    return true;
}
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "selftest: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

std::vector<float> ramp(std::size_t n, float seed) {
    std::vector<float> v(n);
    for (std::size_t i = 0; i < n; ++i) v[i] = std::sin(seed + 0.37f * static_cast<float>(i)) * (1.0f + static_cast<float>(i % 7));
    return v;
}

// what the flat restatement gives for uniform masks
std::vector<std::vector<float>> restated(const std::vector<float>& x, size_t B, size_t SS, size_t DD, const std::vector<std::vector<int32_t>>& masks,
                                         Pooling mode, bool normalize) {
    std::vector<int32_t> flat;
    for (const auto& m : masks) flat.insert(flat.end(), m.begin(), m.end());
    std::vector<float> out(B * DD);
    embed_oracle_pool(x.data(), B, static_cast<uint32_t>(SS), static_cast<uint32_t>(DD), flat.empty() ? nullptr : flat.data(),
                      static_cast<uint32_t>(masks.empty() ? 0 : masks[0].size()), AccelEmbeddingPooler::modeOf(mode), normalize, nullptr, out.data(),
                      nullptr);
    std::vector<std::vector<float>> rows(B);
    for (size_t b = 0; b < B; ++b) rows[b].assign(out.begin() + static_cast<std::ptrdiff_t>(b * DD), out.begin() + static_cast<std::ptrdiff_t>((b + 1) * DD));
    return rows;
}

int selftest() {
    const size_t B = 3, SS = 5, DD = 7;
    const std::vector<float> x = ramp(B * SS * DD, 0.5f);
    const std::vector<std::vector<int32_t>> uniform = {{1, 0, 1, 1, 0}, {0, 1, 1, 1, 1}, {1, 1, 1, 0, 0}};
    auto s = AccelEmbeddingPooler::over(&g_standin);
    // ---- everything uniform reaches the table, in every mode; the result's shape is [B][DD] ----
    for (const Pooling mode : {Pooling::MEAN, Pooling::CLS, Pooling::MAX})
        for (const bool normalize : {false, true}) {
            g_calls = 0;
            const auto before = s->hostCalls();
            const auto got = s->pool(x.data(), B, SS, DD, uniform, mode, normalize);
            CHECK(got.has_value() && g_calls == 1 && s->hostCalls() == before);
            CHECK(got.value().size() == B && got.value()[0].size() == DD && got.value()[2].size() == DD);
            CHECK(sameRows(got.value(), restated(x, B, SS, DD, uniform, mode, normalize)));
            CHECK(sameRows(got.value(), AccelEmbeddingPooler::hostPool(x.data(), B, SS, DD, uniform, mode, normalize)));
            CHECK(s->lastDiag().batch == B && s->lastDiag().dim == DD);
        }
    // ---- ragged masks: the host loop, no call to the table; CLS reads no mask and still reaches it ----
    const std::vector<std::vector<int32_t>> ragged = {{1, 0, 1, 1, 0}, {0, 1, 1}, {1, 1, 1, 0, 0, 1, 1}};
    for (const Pooling mode : {Pooling::MEAN, Pooling::MAX}) {
        g_calls = 0;
        const auto before = s->hostCalls();
        const auto got = s->pool(x.data(), B, SS, DD, ragged, mode, true);
        CHECK(got.has_value() && g_calls == 0 && s->hostCalls() == before + 1);
        for (size_t b = 0; b < B; ++b) {      // text by text against the flat restatement, each with its own mask length
            const std::vector<float> one(x.begin() + static_cast<std::ptrdiff_t>(b * SS * DD), x.begin() + static_cast<std::ptrdiff_t>((b + 1) * SS * DD));
            CHECK(sameRows({got.value()[b]}, restated(one, 1, SS, DD, {ragged[b]}, mode, true)));
        }
        CHECK(got.value().size() == B && got.value()[1].size() == DD);
    }
    g_calls = 0;
    CHECK(s->pool(x.data(), B, SS, DD, ragged, Pooling::CLS, true).has_value() && g_calls == 1);
    // ---- a MEAN weight above 1 inside the considered tokens: the host loop; past them, or for MAX: the table ----
    std::vector<std::vector<int32_t>> heavy = uniform;
    heavy[1][4] = 2;
    g_calls = 0;
    auto before = s->hostCalls();
    auto got = s->pool(x.data(), B, SS, DD, heavy, Pooling::MEAN, false);
    CHECK(got.has_value() && g_calls == 0 && s->hostCalls() == before + 1);
    CHECK(sameRows(got.value(), restated(x, B, SS, DD, heavy, Pooling::MEAN, false)));      // (this driver is built without contraction, as the restatement)
    CHECK(s->pool(x.data(), B, SS, DD, heavy, Pooling::MAX, false).has_value() && g_calls == 1);
    std::vector<std::vector<int32_t>> longer = uniform;
    for (auto& m : longer) m.push_back(2);      // position SS: not considered
    g_calls = 0;
    got = s->pool(x.data(), B, SS, DD, longer, Pooling::MEAN, true);
    CHECK(got.has_value() && g_calls == 1 && sameRows(got.value(), restated(x, B, SS, DD, uniform, Pooling::MEAN, true)));
    // ---- error mapping: UNSUPPORTED is the host loop's, every other refusal an Error of the mapped code ----
    g_answer = YAMS_ERR_UNSUPPORTED;
    before = s->hostCalls();
    got = s->pool(x.data(), B, SS, DD, uniform, Pooling::MEAN, true);
    CHECK(got.has_value() && s->hostCalls() == before + 1 && sameRows(got.value(), restated(x, B, SS, DD, uniform, Pooling::MEAN, true)));
    g_answer = YAMS_ERR_RESOURCE_EXHAUSTED;
    got = s->pool(x.data(), B, SS, DD, uniform, Pooling::MEAN, true);
    CHECK(!got.has_value() && got.error().code == yams::ErrorCode::ResourceExhausted);
    g_answer = YAMS_ERR_INVALID_ARG;
    CHECK(s->pool(x.data(), B, SS, DD, uniform, Pooling::MAX, true).error().code == yams::ErrorCode::InvalidArgument);
    CHECK(s->normalizeRows(x.data(), B, DD, true).error().code == yams::ErrorCode::InvalidArgument);
    // a device-resident tensor has no host loop behind it: NotImplemented
    g_answer = YAMS_ERR_UNSUPPORTED;
    got = s->pool(HiddenStates::onDevice(x.data()), B, SS, DD, uniform, Pooling::MEAN, true);
    CHECK(!got.has_value() && got.error().code == yams::ErrorCode::NotImplemented);
    CHECK(s->pool(HiddenStates::onDevice(x.data()), B, SS, DD, ragged, Pooling::MEAN, true).error().code == yams::ErrorCode::NotImplemented);
    g_answer = YAMS_OK;
    got = s->pool(HiddenStates::onDevice(x.data()), B, SS, DD, uniform, Pooling::MEAN, true);      // (the stand-in's "device" is host memory)
    CHECK(got.has_value() && sameRows(got.value(), restated(x, B, SS, DD, uniform, Pooling::MEAN, true)));
    // ---- limits and empties ----
    CHECK(s->pool(x.data(), 0, SS, DD, uniform, Pooling::MEAN, true).value().empty());
    CHECK(s->pool(nullptr, B, SS, DD, uniform, Pooling::MEAN, true).error().code == yams::ErrorCode::InvalidArgument);
    CHECK(s->pool(x.data(), B, SS, DD, {}, Pooling::MEAN, true).error().code == yams::ErrorCode::InvalidArgument);
    for (const Pooling mode : {Pooling::MEAN, Pooling::CLS, Pooling::MAX}) {      // an empty tensor: the flat entry's verdict, no loop runs
        g_calls = 0;
        before = s->hostCalls();
        CHECK(s->pool(x.data(), B, 0, DD, uniform, mode, true).error().code == yams::ErrorCode::InvalidArgument);
        CHECK(s->pool(x.data(), B, SS, 0, uniform, mode, true).error().code == yams::ErrorCode::InvalidArgument);
        CHECK(s->pool(HiddenStates::onDevice(x.data()), B, 0, DD, uniform, mode, true).error().code == yams::ErrorCode::InvalidArgument);
        CHECK(g_calls == 0 && s->hostCalls() == before);
    }
    CHECK(s->normalizeRows(x.data(), B, 0, true).error().code == yams::ErrorCode::InvalidArgument);
    g_calls = 0;
    got = s->pool(x.data(), B, SS, DD, {{}, {}, {}}, Pooling::MEAN, true);      // empty masks: zeros, served by the table
    CHECK(got.has_value() && g_calls == 1 && got.value()[0] == std::vector<float>(DD, 0.0f));
    // the rank-2 output
    const auto rows = s->normalizeRows(x.data(), B, DD, true);
    std::vector<float> want(B * DD);
    embed_oracle_normalize(x.data(), B, static_cast<uint32_t>(DD), want.data());
    CHECK(rows.has_value() && rows.value().size() == B && rows.value()[1] == std::vector<float>(want.begin() + DD, want.begin() + 2 * DD));
    const auto copied = s->normalizeRows(x.data(), B, DD, false);
    CHECK(copied.has_value() && copied.value()[2] == std::vector<float>(x.begin() + 2 * DD, x.begin() + 3 * DD));
    std::printf("selftest OK\n");
    return 0;
}
#endif

} // namespace

int main(int argc, char** argv) {
    const char* pluginPath = nullptr;
    const char* casePath = nullptr;
    bool hostLoop = false;
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
#ifndef EMBED_WITH_REFERENCE
        if (arg == "--selftest") return selftest();
#endif
        if (arg == "--host-loop") hostLoop = true;
        else if (arg == "--plugin" && i + 1 < argc) pluginPath = argv[++i];
        else casePath = argv[i];
    }
    if (!casePath) { std::fprintf(stderr, "usage: embed_shell_test [--plugin <lib>] <cases> | --selftest\n"); return 2; }
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
#ifdef EMBED_WITH_REFERENCE
    (void)pluginPath; (void)hostLoop;
#else
    std::shared_ptr<yams::accel::Plugin> plugin;
    std::unique_ptr<AccelEmbeddingPooler> shell;
    if (pluginPath) {
        auto p = yams::accel::Plugin::load(pluginPath, "{\"device\":0}");
        if (!p.has_value()) { std::fprintf(stderr, "plugin: %s\n", p.error().message.c_str()); return 3; }
        plugin = p.value();
        auto s = AccelEmbeddingPooler::create(plugin);
        if (!s.has_value()) return 3;
        shell = std::move(s.value());
    } else {
        shell = AccelEmbeddingPooler::over(&g_standin);
    }
#endif
    const std::uint32_t count = rd.u32();
    for (std::uint32_t c = 0; c < count; ++c) {
        const std::uint32_t kind = rd.u32();
        std::vector<std::vector<float>> out;
        if (kind == 0) {
            const std::uint32_t B = rd.u32(), SS = rd.u32(), DD = rd.u32(), mode = rd.u32(), normalize = rd.u32(), maskLen = rd.u32();
            std::vector<std::vector<int32_t>> masks;
            for (std::uint32_t b = 0; b < B; ++b) masks.push_back(rd.array<int32_t>(maskLen));
            const std::vector<float> hidden = rd.array<float>(static_cast<size_t>(B) * SS * DD);
#ifdef EMBED_WITH_REFERENCE
            out = referenceRank3(hidden.data(), B, SS, DD, masks, poolingOf(mode), normalize != 0);
#else
            auto r = hostLoop ? yams::Result<std::vector<std::vector<float>>>(AccelEmbeddingPooler::hostPool(hidden.data(), B, SS, DD, masks, poolingOf(mode), normalize != 0))
                              : shell->pool(hidden.data(), B, SS, DD, masks, poolingOf(mode), normalize != 0);
            if (!r.has_value()) { std::fprintf(stderr, "case %u: %s\n", c, r.error().message.c_str()); return 4; }
            out = std::move(r.value());
#endif
        } else {
            const std::uint32_t B = rd.u32(), DD = rd.u32(), normalize = rd.u32();
            const std::vector<float> rows = rd.array<float>(static_cast<size_t>(B) * DD);
#ifdef EMBED_WITH_REFERENCE
            out = referenceRank2(rows.data(), B, DD, normalize != 0);
#else
            auto r = shell->normalizeRows(rows.data(), B, DD, normalize != 0);
            if (hostLoop) {      // the shell's own normalisation, row by row
                std::vector<std::vector<float>> own(B);
                for (std::uint32_t b = 0; b < B; ++b) {
                    own[b].assign(rows.begin() + static_cast<std::ptrdiff_t>(b * DD), rows.begin() + static_cast<std::ptrdiff_t>((b + 1) * DD));
                    AccelEmbeddingPooler::hostNormalize(own[b]);
                }
                r = own;
            }
            if (!r.has_value()) { std::fprintf(stderr, "case %u: %s\n", c, r.error().message.c_str()); return 4; }
            out = std::move(r.value());
#endif
        }
        printCase(c, out);
    }
#ifndef EMBED_WITH_REFERENCE
    std::printf("device_calls %llu\nhost_calls %llu\n", static_cast<unsigned long long>(shell->deviceCalls()),
                static_cast<unsigned long long>(shell->hostCalls()));
#endif
    return 0;
}
