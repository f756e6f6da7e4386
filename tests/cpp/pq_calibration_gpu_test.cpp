// pq_calibration_gpu_test.cpp — the adapters' side of the PQ sum-order probe, on the device through the plugin: calibratePq /
// calibratePqOnTable / setPqSum / pqSum / pqUncalibratedSearches and the default flag word of the PQ searches.
// Compiled against the reference's headers (-DYAMS_ACCEL_USE_HOST_TYPES) it drives AccelExactScanBackend; without them it
// drives AccelVectorTable, the object the backend forwards to.  Built by tests/_pq_calib_build.py, run by
// tests/test_pq_calibration_gpu.py:  pq_calibration_gpu_test <plugin.so>
//
// The corpus: 3000 indexed rows, m = 44 (8 lanes leave a tail of 4), tables with equal rows across j, and a family of 300
// codes that are permutations of one base code whose bytes name the largest centroids: in exact arithmetic the family ties
// at the top, so with approxK = 100 the ORDER of the fp32 additions alone decides which members come back (rerank factor 1,
// no threshold: every shortlisted row is returned).  The expected SET under a definition is computed here from the header's
// adcSum (held to the numpy restatement by the CPU suite) and the reference's comparator (score desc, stableStringKey asc).
#ifdef YAMS_ACCEL_USE_HOST_TYPES
#include <yams/vector/vector_store.h>
#endif

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#ifdef YAMS_ACCEL_USE_HOST_TYPES
#include "yams_accel/exact_scan_backend.hpp"
#else
#include "yams_accel/vector_index.hpp"
#endif

using namespace yams;
namespace pq = yams::vector::accel_pq;
static int failures = 0, checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static constexpr size_t kDim = 8, kN = 3000, kFamily = 300, kK = 100;

struct Store {          // one face for the two adapters
#ifdef YAMS_ACCEL_USE_HOST_TYPES
    vector::AccelExactScanBackend s;
    explicit Store(std::shared_ptr<accel::Plugin> p) : s(std::move(p)) {}
    bool open() { return s.initialize(":memory:").has_value() && s.createTables(kDim).has_value(); }
    Result<void> setIndex(const std::vector<uint8_t>& codes, size_t m, const std::vector<std::string>& ids) { return s.setSimeonPqIndex(kDim, codes, m, ids); }
    Result<std::vector<vector::VectorRecord>> search(const std::vector<float>& q, const std::vector<float>& lut) { return s.searchSimeonPq(q, lut, kK, -1.0f, 1); }
    Result<std::vector<vector::VectorRecord>> search(const std::vector<float>& q, const std::vector<float>& lut, uint32_t flags) {
        return s.searchSimeonPq(q, lut, kK, -1.0f, 1, nullptr, flags);
    }
    static const char* kind() { return "backend"; }
#else
    vector::AccelVectorTable s;
    explicit Store(std::shared_ptr<accel::Plugin> p) : s(std::move(p)) {}
    bool open() { return true; }
    Result<void> setIndex(const std::vector<uint8_t>& codes, size_t m, const std::vector<std::string>& ids) { return s.setPqIndex(kDim, codes, m, ids); }
    Result<std::vector<vector::VectorRecord>> search(const std::vector<float>& q, const std::vector<float>& lut) {
        auto r = s.searchPqBatch({q}, {lut}, kK, -1.0f, 1);
        if (!r) return r.error();
        return std::move(r.value().front());
    }
    Result<std::vector<vector::VectorRecord>> search(const std::vector<float>& q, const std::vector<float>& lut, uint32_t flags) {
        auto r = s.searchPqBatch({q}, {lut}, kK, -1.0f, 1, nullptr, flags);
        if (!r) return r.error();
        return std::move(r.value().front());
    }
    static const char* kind() { return "table"; }
#endif
};

struct Corpus {
    size_t m;
    std::vector<std::string> ids;
    std::vector<vector::VectorRecord> recs;
    std::vector<uint8_t> codes;
    std::vector<float> query, lut;
};

static Corpus makeCorpus(size_t m, uint32_t seed) {
    Corpus c;
    c.m = m;
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    float v[256];
    for (int i = 0; i < 256; ++i) {
        const bool hot = i >= 192;                                        // positive, the upper three binades
        const float mant = 0.5f + static_cast<float>(rng() & 0x7FFFFF) / 16777216.0f;
        const int e = hot ? static_cast<int>(rng() % 3) : static_cast<int>(rng() % 6) - 3;
        v[i] = ((hot || (rng() & 1)) ? 1.0f : -1.0f) * std::ldexp(mant, e);
    }
    c.lut.resize(m * 256);
    for (size_t j = 0; j < m; ++j) std::memcpy(&c.lut[j * 256], v, sizeof v);
    c.codes.resize(kN * m);
    for (auto& b : c.codes) b = static_cast<uint8_t>(rng() & 255u);
    std::vector<uint8_t> base(m);
    for (auto& b : base) b = static_cast<uint8_t>(192 + rng() % 64);
    for (size_t f = 0; f < kFamily; ++f) {
        const size_t i = 5 + f * 9;                                       // spread over the index
        std::shuffle(base.begin(), base.end(), rng);
        std::copy(base.begin(), base.end(), c.codes.begin() + i * m);
    }
    for (size_t i = 0; i < kN; ++i) {
        char b[32];
        std::snprintf(b, sizeof b, "c%05zu", (i * 7919u) % 100003u);
        c.ids.push_back(b);
        vector::VectorRecord r;
        r.chunk_id = b; r.document_hash = "d" + std::to_string(i / 7); r.content = "x";
        r.embedding.resize(kDim);
        for (auto& x : r.embedding) x = nd(rng);
        c.recs.push_back(std::move(r));
    }
    c.query.resize(kDim);
    for (auto& x : c.query) x = nd(rng);
    return c;
}

// the chunk ids of the best kK codes by (adcSum desc, stableStringKey asc, index asc): what rerank factor 1 returns, as a set
static std::set<std::string> expectedSet(const Corpus& c, uint32_t flags) {
    struct S { float s; uint64_t key; size_t i; };
    std::vector<S> all;
    for (size_t i = 0; i < kN; ++i) {
        uint64_t h = 1469598103934665603ULL;
        for (const unsigned char b : c.ids[i]) { h ^= b; h *= 1099511628211ULL; }
        all.push_back({pq::adcSum(flags, c.lut.data(), &c.codes[i * c.m], c.m), h, i});
    }
    std::sort(all.begin(), all.end(), [](const S& a, const S& b) { return a.s != b.s ? a.s > b.s : (a.key != b.key ? a.key < b.key : a.i < b.i); });
    std::set<std::string> out;
    for (size_t r = 0; r < kK; ++r) out.insert(c.ids[all[r].i]);
    return out;
}
static std::set<std::string> idsOf(const std::vector<vector::VectorRecord>& v) {
    std::set<std::string> s;
    for (const auto& r : v) s.insert(r.chunk_id);
    return s;
}
static bool sameHits(const std::vector<vector::VectorRecord>& a, const std::vector<vector::VectorRecord>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].chunk_id != b[i].chunk_id || std::memcmp(&a[i].relevance_score, &b[i].relevance_score, 4) != 0) return false;
    return true;
}

int main(int argc, char** argv) {
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    if (argc < 2) { std::printf("usage: %s <plugin.so>\n", argv[0]); return 2; }
    auto loaded = accel::Plugin::load(argv[1], "{\"device\":0}");
    if (!loaded.has_value()) { std::printf("plugin load failed\n"); return 1; }
    auto plugin = loaded.value();
    std::printf("[kind] %s\n", Store::kind());
    const uint32_t kHalvesTail = YAMS_PQ_SUM_X8 | YAMS_PQ_SUM_COMBINE_HALVES | YAMS_PQ_SUM_TAIL_SCALAR;
    const Corpus c = makeCorpus(44, 11);
    // the corpus discriminates: the expected sets of the orders used below differ pairwise
    const auto wantSeq = expectedSet(c, YAMS_PQ_SUM_SEQUENTIAL), wantHt = expectedSet(c, kHalvesTail), wantX4 = expectedSet(c, YAMS_PQ_SUM_X4);
    CHECK(wantSeq != wantHt && wantSeq != wantX4 && wantHt != wantX4);
    CHECK(wantHt != expectedSet(c, YAMS_PQ_SUM_X8 | YAMS_PQ_SUM_COMBINE_HALVES));      // (the tail bit matters at m = 44)

    Store st(plugin);
    CHECK(st.open());
    // no index yet: there is no m to probe at
    const pq::PqScoreFn hostHt = [&](const float* t, const uint8_t* code, size_t m, float* out) { *out = pq::adcSum(kHalvesTail, t, code, m); return true; };
    { auto r = st.s.calibratePq(hostHt); CHECK(!r.has_value() && r.error().code == ErrorCode::InvalidArgument); }
    { auto r = st.s.calibratePqOnTable(c.lut, [](const uint8_t*, float*) { return true; }); CHECK(!r.has_value() && r.error().code == ErrorCode::InvalidArgument); }
    CHECK(st.s.insertVectorsBatch(c.recs).has_value());
    CHECK(st.setIndex(c.codes, c.m, c.ids).has_value());

    // 1. uncalibrated: the sequential sum, counted
    CHECK(st.s.pqUncalibratedSearches() == 0 && !st.s.pqSum().calibrated);
    auto seq = st.search(c.query, c.lut, YAMS_PQ_SUM_SEQUENTIAL);
    auto def0 = st.search(c.query, c.lut);
    CHECK(seq.has_value() && def0.has_value());
    if (!seq.has_value() || !def0.has_value()) { std::printf("FAILED (%d failures)\n", failures + 1); return 1; }
    CHECK(seq.value().size() == kK && sameHits(seq.value(), def0.value()) && idsOf(seq.value()) == wantSeq);
    CHECK(st.s.pqUncalibratedSearches() == 1);                      // (the explicit word is not counted)
    (void)st.search(c.query, c.lut);
    CHECK(st.s.pqUncalibratedSearches() == 2);

    // 2. calibrated with the header's x8_halves_tail as the host: the default word is that order
    auto cal = st.s.calibratePq(hostHt);
    CHECK(cal.has_value() && cal.value().matched && cal.value().flags == kHalvesTail && cal.value().matching.size() == 1 && cal.value().m == 44);
    CHECK(st.s.pqSum().calibrated && st.s.pqSum().matched && st.s.pqSum().flags == kHalvesTail);
    auto ht = st.search(c.query, c.lut, kHalvesTail);
    auto def1 = st.search(c.query, c.lut);
    CHECK(ht.has_value() && def1.has_value() && sameHits(ht.value(), def1.value()));
    CHECK(ht.has_value() && idsOf(ht.value()) == wantHt && idsOf(ht.value()) != idsOf(seq.value()));
    CHECK(st.s.pqUncalibratedSearches() == 2);

    // 3. a host whose order is not served: the default word is refused, an explicit one still served
    auto bad = st.s.calibratePq([](const float* t, const uint8_t* code, size_t m, float* out) {
        volatile float s = 0.0f;
        for (size_t j = m; j-- > 0;) s = s + t[j * 256 + code[j]];
        *out = s; return true; });
    CHECK(bad.has_value() && !bad.value().matched && bad.value().matching.empty());
    CHECK(st.s.pqSum().calibrated && !st.s.pqSum().matched);
    auto refused = st.search(c.query, c.lut);
    CHECK(!refused.has_value() && refused.error().code == ErrorCode::NotSupported);
    auto still = st.search(c.query, c.lut, kHalvesTail);
    CHECK(still.has_value() && sameHits(still.value(), ht.value()));

    // 4. pinned by hand; a word the device would refuse is refused here
    CHECK(st.s.setPqSum(YAMS_PQ_SUM_X4).has_value());
    auto x4 = st.search(c.query, c.lut);
    CHECK(x4.has_value() && idsOf(x4.value()) == wantX4);
    { auto r = st.s.setPqSum(YAMS_PQ_SUM_TAIL_SCALAR); CHECK(!r.has_value() && r.error().code == ErrorCode::InvalidArgument); }
    CHECK(st.s.pqSum().flags == YAMS_PQ_SUM_X4);

    // 5. the fixed-table shape: the host scores codes against ITS table
    auto onTable = st.s.calibratePqOnTable(c.lut, [&](const uint8_t* code, float* out) { *out = pq::adcSum(kHalvesTail, c.lut.data(), code, c.m); return true; });
    CHECK(onTable.has_value() && onTable.value().matched && onTable.value().flags == kHalvesTail);
    auto def2 = st.search(c.query, c.lut);
    CHECK(def2.has_value() && sameHits(def2.value(), ht.value()));
    { auto r = st.s.calibratePqOnTable(std::vector<float>(7), [](const uint8_t*, float*) { return true; }); CHECK(!r.has_value() && r.error().code == ErrorCode::InvalidArgument); }

    // 6. a later index with another m: the kept function is asked again (at m = 32 the tail bit changes nothing: x8_halves)
    CHECK(st.s.calibratePq(hostHt).has_value());
    const Corpus c32 = makeCorpus(32, 12);
    CHECK(st.setIndex(c32.codes, c32.m, c.ids).has_value());
    CHECK(st.s.pqSum().calibrated && st.s.pqSum().matched && st.s.pqSum().m == 32);
    CHECK(st.s.pqSum().flags == (YAMS_PQ_SUM_X8 | YAMS_PQ_SUM_COMBINE_HALVES));
    auto d32 = st.search(c.query, c32.lut);
    auto e32 = st.search(c.query, c32.lut, kHalvesTail);
    CHECK(d32.has_value() && e32.has_value() && sameHits(d32.value(), e32.value()));
    CHECK(d32.has_value() && idsOf(d32.value()) == expectedSet(c32, kHalvesTail));

    std::printf("%s (%d failures, %d checks)\n", failures ? "FAILED" : "OK", failures, checks);
    return failures ? 1 : 0;
}
