// pq_calibration_test.cpp — include/yams_accel/pq_calibration.hpp on the CPU (plain g++, AddressSanitizer + UBSan, its own main).
// Driven by tests/test_pq_calibration_cpu.py, which holds what is printed here to the numpy restatement (tests/_pq_sum.py):
//   classes <m>          every definition plays the host, through both host shapes: "<host> <shape> <matched> <flags> <matching...>"
//   refused <m>          hosts whose order is NOT served: "<host> <matched> <detail>"
//   avx2 <m>             two -mavx2 translation units (pq_host_avx2_a.cpp / _b.cpp) play the host: the same line
//   distinguishing <m>   "1" when every pair of definitions is told apart by >= 3 probes or by none
//   --dump <m>           adcSum of every definition on every probe, as hex: "<probe> <definition> <bits>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "yams_accel/pq_calibration.hpp"

namespace pq = yams::vector::accel_pq;

extern "C" float pq_host_avx2_halves(const float* table, const uint8_t* code, size_t m);
extern "C" float pq_host_avx2_halves4_pairs(const float* table, const uint8_t* code, size_t m);

static std::vector<float> values(const float* table, const uint8_t* code, size_t m) {
    std::vector<float> v(m);
    for (size_t j = 0; j < m; ++j) v[j] = table[j * 256 + code[j]];
    return v;
}
static float pairwise(const float* v, size_t n) {   // a recursive pairwise sum over ELEMENTS (split at n / 2)
    if (n == 1) return v[0];
    volatile float a = pairwise(v, n / 2), b = pairwise(v + n / 2, n - n / 2);
    volatile float s = a + b;
    return s;
}
static float lanesLtr(const float* v, size_t m, size_t L) {   // L round-robin lanes, added left to right
    std::vector<float> p(L, 0.0f);
    for (size_t j = 0; j < m; ++j) { volatile float s = p[j % L] + v[j]; p[j % L] = s; }
    volatile float acc = 0.0f;
    for (size_t l = 0; l < L; ++l) acc = acc + p[l];
    return acc;
}

static void printCalibration(const char* host, const char* shape, const pq::PqCalibration& c) {
    std::printf("%s %s %d %s", host, shape, c.matched ? 1 : 0, c.matched ? pq::name(c.flags).c_str() : "-");
    for (uint32_t f : c.matching) std::printf(" %s", pq::name(f).c_str());
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: %s classes|refused|avx2|distinguishing|--dump <m>\n", argv[0]); return 2; }
    const std::string mode = argv[1];
    const size_t m = static_cast<size_t>(std::atoi(argv[2]));
    if (mode == "classes") {
        const auto P = pq::probes(m);
        const std::vector<float>& fixed = *P[0].table;          // the "host's own" table of the fixed-table shape
        for (uint32_t d : pq::definitions()) {
            const auto c1 = pq::calibratePq([d](const float* t, const uint8_t* c, size_t mm, float* out) { *out = pq::adcSum(d, t, c, mm); return true; }, m);
            printCalibration(pq::name(d).c_str(), "table", c1);
            const auto c2 = pq::calibratePqOnTable(fixed.data(), m, [&](const uint8_t* c, float* out) { *out = pq::adcSum(d, fixed.data(), c, m); return true; });
            printCalibration(pq::name(d).c_str(), "code", c2);
        }
        return 0;
    }
    if (mode == "refused") {
        struct Host { const char* name; pq::PqScoreFn fn; };
        const std::vector<Host> hosts = {
            {"reverse", [](const float* t, const uint8_t* c, size_t mm, float* out) {
                 volatile float s = 0.0f;
                 for (size_t j = mm; j-- > 0;) s = s + t[j * 256 + c[j]];
                 *out = s; return true; }},
            {"pairwise", [](const float* t, const uint8_t* c, size_t mm, float* out) { const auto v = values(t, c, mm); *out = pairwise(v.data(), mm); return true; }},
            {"x2", [](const float* t, const uint8_t* c, size_t mm, float* out) { const auto v = values(t, c, mm); *out = lanesLtr(v.data(), mm, 2); return true; }},
            {"x32", [](const float* t, const uint8_t* c, size_t mm, float* out) { const auto v = values(t, c, mm); *out = lanesLtr(v.data(), mm, 32); return true; }},
            {"f64", [](const float* t, const uint8_t* c, size_t mm, float* out) {
                 volatile double s = 0.0;
                 for (size_t j = 0; j < mm; ++j) s = s + static_cast<double>(t[j * 256 + c[j]]);
                 *out = static_cast<float>(s); return true; }},
            {"fails", [](const float*, const uint8_t*, size_t, float*) { return false; }},
            {"nan", [](const float*, const uint8_t*, size_t, float* out) { *out = std::numeric_limits<float>::quiet_NaN(); return true; }},
        };
        int bad = 0;
        for (const Host& h : hosts) {
            const auto c = pq::calibratePq(h.fn, m);
            std::printf("%s %d %s\n", h.name, c.matched ? 1 : 0, c.detail.c_str());
            bad += c.matched || !c.matching.empty();
            // the same host behind the fixed-table shape
            const auto P = pq::probes(m);
            const float* tab = P[0].table->data();
            const auto c2 = pq::calibratePqOnTable(tab, m, [&](const uint8_t* code, float* out) { return h.fn(tab, code, m, out); });
            std::printf("%s/code %d %s\n", h.name, c2.matched ? 1 : 0, c2.detail.c_str());
            bad += c2.matched;
        }
        // no function, no table, m == 0: no match, no crash
        bad += pq::calibratePq(nullptr, m).matched + pq::calibratePq(hosts[0].fn, 0).matched + pq::calibratePqOnTable(nullptr, m, nullptr).matched;
        return bad ? 1 : 0;
    }
    if (mode == "avx2") {
        const auto a = pq::calibratePq([](const float* t, const uint8_t* c, size_t mm, float* out) { *out = pq_host_avx2_halves(t, c, mm); return true; }, m);
        printCalibration("halves", "table", a);
        const auto b = pq::calibratePq([](const float* t, const uint8_t* c, size_t mm, float* out) { *out = pq_host_avx2_halves4_pairs(t, c, mm); return true; }, m);
        printCalibration("halves4_pairs", "table", b);
        return 0;
    }
    if (mode == "distinguishing") {
        std::printf("%d\n", pq::distinguishing(m) ? 1 : 0);
        // separating() agrees with it on a pair that differs and on one that coincides (the tail bit at m % 4 == 0)
        if (m % 4 == 0 && pq::separating(YAMS_PQ_SUM_X4, YAMS_PQ_SUM_X4 | YAMS_PQ_SUM_TAIL_SCALAR, m) != 0) return 1;
        if (m >= 8 && pq::separating(YAMS_PQ_SUM_SEQUENTIAL, YAMS_PQ_SUM_X4 | YAMS_PQ_SUM_COMBINE_HALVES, m) < 3) return 1;
        return 0;
    }
    if (mode == "--dump") {
        const auto P = pq::probes(m);
        for (size_t i = 0; i < P.size(); ++i)
            for (uint32_t d : pq::definitions())
                std::printf("%zu %s %08x\n", i, pq::name(d).c_str(), pq::bitsOf(pq::adcSum(d, P[i].table->data(), P[i].code.data(), m)));
        const auto C = pq::probeCodes(m);
        for (size_t i = 0; i < C.size(); ++i) {
            std::printf("code %zu", i);
            for (uint8_t b : C[i]) std::printf(" %u", static_cast<unsigned>(b));
            std::printf("\n");
        }
        return 0;
    }
    std::printf("unknown mode %s\n", mode.c_str());
    return 2;
}
