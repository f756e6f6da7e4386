// pq_calibration.hpp — in which ORDER does the HOST's product-quantiser add a code's table entries?  Asked of the host's own
// scoring function.
//
// The product-quantised engine scores a row with approxScore = sum over j of lut[j][code[j]] in fp32
// (SqliteVecBackend::Impl::simeonPqSearchUnlocked, src/vector/sqlite_vec_backend.cpp:3965-3977).  The sum itself is
// simeon::PQInnerProductQuery::inner_product, and third_party/simeon is ABSENT from the reference checkout: NOTHING about
// its arithmetic is pinned here.  Two orders of the same additions differ in the last bits, and at the approxK cut that
// decides which rows are re-ranked at all — so the host must not guess, and this library must not guess for it.  It serves
// the shapes a table sum takes when a compiler or a person vectorises it (YAMS_PQ_SUM_* in yams_mi355x_accel.h):
//   lanes     1 (a scalar loop), or 4 / 8 / 16 partial sums, element j -> lane j % L          (SSE / AVX / AVX-512 registers)
//   combine   how the L partial sums become one: left to right (a store + scalar loop), HALVES (extract-high + add, then
//             movehl / shuffle), PAIRS (hadd), HALVES4_PAIRS (extract-high down to 4 lanes, then movehdup + movehl)
//   tail      the m % L elements after the last full vector: into the lanes (a masked / padded load), or added one by one
//             AFTER the reduction (YAMS_PQ_SUM_TAIL_SCALAR: the usual remainder loop)
// 1 + 3 * 4 * 2 = 25 definitions.  calibratePq() runs the host's function on crafted (table, code) pairs OF THE INDEX'S OWN m
// and reports which definitions reproduce every probe bit for bit.  One, or several that coincide at this m (the tail bit
// when m % L == 0, 4 lanes under PAIRS and HALVES4_PAIRS, ...): use the first.  None: the host's build does something
// else (2 or 32 lanes, a pairwise tree over elements, fp64 partials, ...) and the engine must be REFUSED
// (ErrorCode::NotSupported) rather than served with a shortlist that differs from the host's own — see
// AccelVectorIndex::calibratePq / AccelExactScanBackend::calibratePq.
//
// What is asked of the host: ONE of
//   PqScoreFn      score an ARBITRARY table: bool(const float* table /*[m][256]*/, const uint8_t* code, size_t m, float* out)
//   PqCodeScoreFn  score a code against the table of a PQInnerProductQuery the host built from a real query:
//                  bool(const uint8_t* code, float* out), plus that table (pqQuery.table())
//
// Header-only, std-only, no device: calibration is host arithmetic.  adcSum() below is what the device kernels implement
// (pq_kernels.hip); the test suite holds both to an independent numpy restatement (tests/_pq_sum.py).
#pragma once
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../yams_mi355x_accel.h"

namespace yams::vector::accel_pq {

// "the order calibration settled": the default sumFlags of the adapters' PQ searches.  Outside YAMS_PQ_SUM_ORDER_MASK, never
// sent to the device.
inline constexpr uint32_t kPqSumCalibrated = 0x80000000u;

inline size_t lanes(uint32_t flags) {
    switch (flags & YAMS_PQ_SUM_MASK) {
        case YAMS_PQ_SUM_X4: return 4;
        case YAMS_PQ_SUM_X8: return 8;
        case YAMS_PQ_SUM_X16: return 16;
        default: return 1;
    }
}
// a flag word the device accepts: with one lane there is nothing to combine and no vector tail
inline bool valid(uint32_t flags) { return lanes(flags) > 1 || (flags & YAMS_PQ_SUM_ORDER_MASK & ~YAMS_PQ_SUM_MASK) == 0; }

// One definition, on the host.  volatile keeps a compiler with -ffast-math / -fassociative-math from re-associating what
// is being DEFINED here (each sum rounds on its own, in this order).  With one lane the combine and tail bits mean nothing.
inline float adcSum(uint32_t flags, const float* table /*[m][256]*/, const uint8_t* code, size_t m) {
    const size_t L = lanes(flags);
    const uint32_t comb = L > 1 ? (flags & YAMS_PQ_SUM_COMBINE_MASK) : YAMS_PQ_SUM_COMBINE_LTR;
    const size_t body = (L > 1 && (flags & YAMS_PQ_SUM_TAIL_SCALAR)) ? m - m % L : m;
    volatile float p[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t j = 0; j < body; ++j) p[j % L] = p[j % L] + table[j * 256 + code[j]];
    volatile float s = 0.0f;
    if (L == 1) {
        s = p[0];
    } else if (comb == YAMS_PQ_SUM_COMBINE_HALVES) {
        for (size_t w = L / 2; w >= 1; w /= 2)
            for (size_t l = 0; l < w; ++l) p[l] = p[l] + p[l + w];
        s = p[0];
    } else if (comb == YAMS_PQ_SUM_COMBINE_PAIRS) {
        for (size_t w = L; w > 1; w /= 2)
            for (size_t l = 0; l < w / 2; ++l) p[l] = p[2 * l] + p[2 * l + 1];
        s = p[0];
    } else if (comb == YAMS_PQ_SUM_COMBINE_HALVES4_PAIRS) {
        for (size_t w = L / 2; w >= 4; w /= 2)
            for (size_t l = 0; l < w; ++l) p[l] = p[l] + p[l + w];
        p[0] = p[0] + p[1];
        p[2] = p[2] + p[3];
        s = p[0] + p[2];
    } else {
        for (size_t l = 0; l < L; ++l) s = s + p[l];
    }
    for (size_t j = body; j < m; ++j) s = s + table[j * 256 + code[j]];
    return s;
}

// The 25 flag words in preference order: fewer lanes first, then the combine (left to right first), then no tail bit first.
inline constexpr size_t kNumDefinitions = 25;
inline const std::array<uint32_t, kNumDefinitions>& definitions() {
    static const std::array<uint32_t, kNumDefinitions> d = [] {
        std::array<uint32_t, kNumDefinitions> a{};
        size_t n = 0;
        a[n++] = YAMS_PQ_SUM_SEQUENTIAL;
        for (uint32_t l : {YAMS_PQ_SUM_X4, YAMS_PQ_SUM_X8, YAMS_PQ_SUM_X16})
            for (uint32_t c : {YAMS_PQ_SUM_COMBINE_LTR, YAMS_PQ_SUM_COMBINE_HALVES, YAMS_PQ_SUM_COMBINE_PAIRS, YAMS_PQ_SUM_COMBINE_HALVES4_PAIRS})
                for (uint32_t t : {0u, YAMS_PQ_SUM_TAIL_SCALAR}) a[n++] = l | c | t;
        return a;
    }();
    return d;
}
// "seq", "x8", "x8_halves", "x16_halves4_pairs_tail", ...
inline std::string name(uint32_t flags) {
    const size_t L = lanes(flags);
    if (L == 1) return "seq";
    std::string s = "x" + std::to_string(L);
    switch (flags & YAMS_PQ_SUM_COMBINE_MASK) {
        case YAMS_PQ_SUM_COMBINE_HALVES: s += "_halves"; break;
        case YAMS_PQ_SUM_COMBINE_PAIRS: s += "_pairs"; break;
        case YAMS_PQ_SUM_COMBINE_HALVES4_PAIRS: s += "_halves4_pairs"; break;
        default: break;
    }
    if (flags & YAMS_PQ_SUM_TAIL_SCALAR) s += "_tail";
    return s;
}

// The host's scoring: true and *out = the fp32 score, or false when the call failed.
using PqScoreFn = std::function<bool(const float* table, const uint8_t* code, size_t m, float* out)>;
using PqCodeScoreFn = std::function<bool(const uint8_t* code, float* out)>;

struct Probe {
    std::shared_ptr<const std::vector<float>> table; // [m][256]
    std::vector<uint8_t> code;                       // [m]
};

// The probes: kProbeTables tables of the given m with kCodesPerTable codes each, deterministic (a 64-bit LCG, no <random>:
// the same bits on every standard library).  Table magnitudes are spread over six binades so that reductions of different
// shape round differently.  The draws, in order: per table, per entry (one for the mantissa, one for the binade); then per
// code of that table, per byte.
inline constexpr size_t kProbeTables = 8, kCodesPerTable = 16, kProbes = kProbeTables * kCodesPerTable;
struct Lcg {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<uint32_t>(s >> 33); }
};
inline std::vector<Probe> probes(size_t m) {
    std::vector<Probe> v;
    Lcg g{0x9E3779B97F4A7C15ull ^ (static_cast<uint64_t>(m) * 0xD1B54A32D192ED03ull)};
    for (size_t t = 0; t < kProbeTables; ++t) {
        auto tab = std::make_shared<std::vector<float>>(m * 256);
        for (float& x : *tab) {
            const float u = static_cast<float>(g.next() & 0xFFFFFF) / 16777216.0f - 0.5f;
            x = u * std::ldexp(1.0f, static_cast<int>(g.next() % 6) - 3);
        }
        for (size_t c = 0; c < kCodesPerTable; ++c) {
            Probe p;
            p.table = tab;
            p.code.resize(m);
            for (uint8_t& b : p.code) b = static_cast<uint8_t>(g.next() & 255u);
            v.push_back(std::move(p));
        }
    }
    return v;
}
// the fixed-table form: only the codes are generated (kProbes of them; another stream than probes(m))
inline std::vector<std::vector<uint8_t>> probeCodes(size_t m) {
    std::vector<std::vector<uint8_t>> v(kProbes, std::vector<uint8_t>(m));
    Lcg g{0xC2B2AE3D27D4EB4Full ^ (static_cast<uint64_t>(m) * 0xD1B54A32D192ED03ull)};
    for (auto& code : v)
        for (uint8_t& b : code) b = static_cast<uint8_t>(g.next() & 255u);
    return v;
}

inline uint32_t bitsOf(float f) {
    uint32_t b;
    static_assert(sizeof b == sizeof f, "fp32");
    std::memcpy(&b, &f, 4);
    return b;
}

// (on the bits: x != x is folded away under -ffinite-math-only, and a host may build with -ffast-math)
inline bool isNan(float f) { return (bitsOf(f) & 0x7fffffffu) > 0x7f800000u; }

// pairwise: how many probes of this m give different fp32 sums under definitions x and y (0: the two coincide at this m and
// either serves)
inline size_t separating(uint32_t x, uint32_t y, size_t m) {
    size_t n = 0;
    for (const Probe& p : probes(m))
        n += bitsOf(adcSum(x, p.table->data(), p.code.data(), m)) != bitsOf(adcSum(y, p.table->data(), p.code.data(), m));
    return n;
}
// every pair of definitions is either told apart by at least `minSeparating` probes or not at all (asserted by the tests for
// the m a product quantiser has; calibration itself needs ONE separating probe per distinct pair)
inline bool distinguishing(size_t m, size_t minSeparating = 3) {
    const auto P = probes(m);
    const auto& D = definitions();
    std::vector<std::vector<uint32_t>> got(D.size(), std::vector<uint32_t>(P.size()));
    for (size_t d = 0; d < D.size(); ++d)
        for (size_t i = 0; i < P.size(); ++i) got[d][i] = bitsOf(adcSum(D[d], P[i].table->data(), P[i].code.data(), m));
    for (size_t a = 0; a < D.size(); ++a)
        for (size_t b = a + 1; b < D.size(); ++b) {
            size_t n = 0;
            for (size_t i = 0; i < P.size(); ++i) n += got[a][i] != got[b][i];
            if (n != 0 && n < minSeparating) return false;
        }
    return true;
}

struct PqCalibration {
    bool matched = false;               // at least one definition reproduced every probe bit for bit
    uint32_t flags = 0;                 // the first of them in preference order: YAMS_PQ_SUM_* for yams_scan_pq_params_t::flags
    std::vector<uint32_t> matching;     // all of them (they coincide on every probe of this m)
    size_t m = 0, probes = 0, failedCalls = 0, nanResults = 0;
    std::array<size_t, kNumDefinitions> agreed{}; // per definition (definitions() order): probes it reproduced
    std::string detail;                 // one line for the log
};

namespace impl {
// `score(i, table, code, out)` is the host's answer on probe i
template <typename Score>
inline PqCalibration run(size_t m, const std::vector<const float*>& tables, const std::vector<const uint8_t*>& codes, Score&& score,
                         const char* what) {
    PqCalibration c;
    c.m = m;
    c.probes = codes.size();
    const auto& D = definitions();
    for (size_t i = 0; i < codes.size(); ++i) {
        float got = 0.0f;
        if (!score(tables[i], codes[i], &got)) { ++c.failedCalls; continue; }
        bool finite = true; // (a NaN from the host on a probe whose every served sum is a number: the host does something else)
        for (size_t d = 0; d < D.size(); ++d) {
            const float want = adcSum(D[d], tables[i], codes[i], m);
            finite = finite && !isNan(want);
            c.agreed[d] += bitsOf(want) == bitsOf(got);
        }
        if (isNan(got) && finite) ++c.nanResults;
    }
    for (size_t d = 0; d < D.size(); ++d)
        if (c.failedCalls == 0 && c.nanResults == 0 && c.probes != 0 && c.agreed[d] == c.probes) c.matching.push_back(D[d]);
    c.matched = !c.matching.empty();
    if (c.matched) c.flags = c.matching.front();
    c.detail = std::string(c.matched ? "host PQ sum " : "host PQ sum matches NO served order ") + "(" + what + ") at m " + std::to_string(m);
    if (c.matched) {
        c.detail += " = " + name(c.flags);
        if (c.matching.size() > 1) {
            c.detail += " (coincides here with";
            for (size_t i = 1; i < c.matching.size(); ++i) c.detail += " " + name(c.matching[i]);
            c.detail += ")";
        }
    } else {
        size_t best = 0;
        for (size_t d = 1; d < D.size(); ++d) if (c.agreed[d] > c.agreed[best]) best = d;
        c.detail += "; closest " + name(D[best]) + " with " + std::to_string(c.agreed[best]);
    }
    c.detail += " of " + std::to_string(c.probes) + " probes";
    if (c.failedCalls) c.detail += ", failed calls " + std::to_string(c.failedCalls);
    if (c.nanResults) c.detail += ", NaN results " + std::to_string(c.nanResults);
    return c;
}
} // namespace impl

// `m`: the sub-quantiser count of the index the host serves (the probes have it).
inline PqCalibration calibratePq(const PqScoreFn& fn, size_t m) {
    if (!fn || m == 0) {
        PqCalibration c;
        c.m = m;
        c.detail = !fn ? "no scoring function given" : "m == 0";
        return c;
    }
    const auto P = probes(m);
    std::vector<const float*> tables;
    std::vector<const uint8_t*> codes;
    for (const Probe& p : P) { tables.push_back(p.table->data()); codes.push_back(p.code.data()); }
    return impl::run(m, tables, codes, [&](const float* t, const uint8_t* c, float* out) { return fn(t, c, m, out); }, "arbitrary tables");
}
// `table`: the [m][256] table the host's query object holds (any real query's; it must be finite); `codeFn` scores a code
// against THAT table.  A real table spreads its magnitudes less than the crafted ones, so orders are told apart by fewer
// probes each — which is why every code is a probe here too.
inline PqCalibration calibratePqOnTable(const float* table, size_t m, const PqCodeScoreFn& codeFn) {
    if (!codeFn || !table || m == 0) {
        PqCalibration c;
        c.m = m;
        c.detail = !codeFn ? "no scoring function given" : (!table ? "no table given" : "m == 0");
        return c;
    }
    const auto C = probeCodes(m);
    std::vector<const float*> tables(C.size(), table);
    std::vector<const uint8_t*> codes;
    for (const auto& c : C) codes.push_back(c.data());
    return impl::run(m, tables, codes, [&](const float*, const uint8_t* c, float* out) { return codeFn(c, out); }, "the host's table");
}

} // namespace yams::vector::accel_pq
