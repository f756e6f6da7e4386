// xcd_deal_test — the deal of the int8 sweep's units to the XCDs (yams_amd/csrc/xcd_deal.h: the header the kernels inline),
// on the CPU.  Plain C++ with its own main, built with AddressSanitizer + UBSan by tests/_xcd_deal_build.py: every table is a
// heap array of exactly its contracted length.
//
//   xcd_deal_test <equal|clamps|one_min|random|feedback>      exit status 0 = every case held; prints the number of cases
#include "../../yams_amd/csrc/xcd_deal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

using namespace yams_accel;

static int failures = 0;
#define CHECK(cond, ...)                                                                                  \
    do {                                                                                                  \
        if (!(cond)) {                                                                                    \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                  \
            std::printf(__VA_ARGS__);                                                                     \
            std::printf("\n");                                                                            \
            if (++failures > 20) std::exit(1);                                                            \
        }                                                                                                 \
    } while (0)

static const uint32_t kUnits[] = {0, 1, 7, 8, 95, 96, 97, 12019};
static const uint32_t kStreamsX[] = {1, 4, 16};

// every unit of [0, n_units) exactly once over all streams; stream lengths as the header says; with `equal` the lengths of
// the former rule `stream + j * n_streams`; never more than the clamp beyond the equal share
static void check_deal(const uint32_t* w, uint32_t n_units, uint32_t streams_x, bool equal, const char* what) {
    std::unique_ptr<uint32_t[]> off(new uint32_t[XCD_DEAL_XCDS + 1]);
    xcd_deal_offsets(w, n_units, streams_x, off.get());
    CHECK(off[0] == 0 && off[XCD_DEAL_XCDS] == n_units, "%s n=%u sx=%u: off[0]=%u off[8]=%u", what, n_units, streams_x, off[0], off[XCD_DEAL_XCDS]);
    for (uint32_t x = 0; x < XCD_DEAL_XCDS; ++x) CHECK(off[x] <= off[x + 1], "%s n=%u sx=%u: off[] not monotonic at %u", what, n_units, streams_x, x);
    std::unique_ptr<uint8_t[]> seen(new uint8_t[n_units ? n_units : 1]);
    std::memset(seen.get(), 0, n_units ? n_units : 1);
    const uint32_t n_streams = streams_x * XCD_DEAL_XCDS;
    const uint32_t most = xcd_deal_max_stream_length(n_units, streams_x);
    uint64_t total = 0;
    for (uint32_t x = 0; x < XCD_DEAL_XCDS; ++x) {
        // an XCD's share: its equal share + at most 8 % of an eighth of the units + one unit of rounding
        const uint64_t eq = xcd_deal_equal_count(n_units, streams_x, x);
        const uint64_t cnt = off[x + 1] - off[x];
        CHECK(cnt <= eq + static_cast<uint64_t>(n_units) * XCD_DEAL_CLAMP / (8ull * XCD_DEAL_ONE) + 1, "%s n=%u sx=%u: XCD %u has %llu units, equal share %llu",
              what, n_units, streams_x, x, (unsigned long long)cnt, (unsigned long long)eq);
        if (equal) CHECK(cnt == eq, "%s n=%u sx=%u: XCD %u has %llu units under equal weights, not %llu", what, n_units, streams_x, x,
                         (unsigned long long)cnt, (unsigned long long)eq);
        for (uint32_t st = 0; st < streams_x; ++st) {
            uint32_t len = 0;
            for (uint32_t j = 0;; ++j) {
                const uint32_t u = xcd_deal_unit(off[x], off[x + 1], streams_x, st, j);
                if (u == 0xffffffffu) break;
                CHECK(u < n_units, "%s n=%u sx=%u: unit %u out of range", what, n_units, streams_x, u);
                if (u >= n_units) break;
                CHECK(!seen[u], "%s n=%u sx=%u: unit %u dealt twice", what, n_units, streams_x, u);
                seen[u] = 1;
                ++len;
            }
            // past the end stays past the end
            CHECK(xcd_deal_unit(off[x], off[x + 1], streams_x, st, len + 1) == 0xffffffffu && xcd_deal_unit(off[x], off[x + 1], streams_x, st, 0xffffffffu) == 0xffffffffu,
                  "%s n=%u sx=%u: stream (%u, %u) comes back after its end", what, n_units, streams_x, st, x);
            CHECK(len == xcd_deal_stream_length(off[x], off[x + 1], streams_x, st), "%s n=%u sx=%u: stream (%u, %u) length %u", what, n_units, streams_x, st, x, len);
            CHECK(len <= most, "%s n=%u sx=%u: stream (%u, %u) has %u units, the bound is %u", what, n_units, streams_x, st, x, len, most);
            // the former rule: stream s = st * 8 + x owned s, s + n_streams, ...
            const uint32_t s = st * XCD_DEAL_XCDS + x;
            const uint32_t old_len = n_units > s ? (n_units - s + n_streams - 1) / n_streams : 0;
            if (equal) CHECK(len == old_len, "%s n=%u sx=%u: stream (%u, %u) has %u units under equal weights, the former rule gave %u", what, n_units, streams_x, st, x, len, old_len);
            // no stream exceeds its (former, equal) share by more than the clamp: 8 % + the rounding of the XCD's count over its streams
            CHECK(len <= old_len + (static_cast<uint64_t>(old_len) * XCD_DEAL_CLAMP + XCD_DEAL_ONE - 1) / XCD_DEAL_ONE + 2, "%s n=%u sx=%u: stream (%u, %u) has %u units, equal share %u",
                  what, n_units, streams_x, st, x, len, old_len);
            total += len;
        }
    }
    CHECK(total == n_units, "%s n=%u sx=%u: %llu units dealt", what, n_units, streams_x, (unsigned long long)total);
    for (uint32_t u = 0; u < n_units; ++u) CHECK(seen[u], "%s n=%u sx=%u: unit %u not dealt", what, n_units, streams_x, u);
}

int main(int argc, char** argv) {
    const std::string kind = argc > 1 ? argv[1] : "equal";
    const uint32_t lo = XCD_DEAL_ONE - XCD_DEAL_CLAMP, hi = XCD_DEAL_ONE + XCD_DEAL_CLAMP;
    std::vector<std::vector<uint32_t>> sets;
    if (kind == "equal") {
        sets.push_back(std::vector<uint32_t>(8, XCD_DEAL_ONE));
        sets.push_back(std::vector<uint32_t>(8, 1u));            // equal is equal at any scale
        sets.push_back(std::vector<uint32_t>(8, 0xffffffffu));
        sets.push_back(std::vector<uint32_t>(8, 0u));            // no information: equal
    } else if (kind == "clamps") {                               // every weight at a clamp (and beyond: clamped)
        sets.push_back({lo, hi, lo, hi, lo, hi, lo, hi});
        sets.push_back({hi, lo, hi, lo, hi, lo, hi, lo});
        sets.push_back({hi, hi, hi, hi, lo, lo, lo, lo});
        sets.push_back({1u, 0xffffffffu, 1u, 0xffffffffu, 1u, 0xffffffffu, 1u, 0xffffffffu});
        sets.push_back({hi, lo, lo, lo, lo, lo, lo, lo});
        sets.push_back({lo, hi, hi, hi, hi, hi, hi, hi});
    } else if (kind == "one_min") {
        for (uint32_t x = 0; x < 8; ++x) { std::vector<uint32_t> w(8, XCD_DEAL_ONE); w[x] = lo; sets.push_back(w); }
        for (uint32_t x = 0; x < 8; ++x) { std::vector<uint32_t> w(8, XCD_DEAL_ONE); w[x] = 0u; sets.push_back(w); }
    } else if (kind == "random") {
        std::mt19937 rng(20261020u);
        for (int i = 0; i < 200; ++i) {
            std::vector<uint32_t> w(8);
            for (auto& v : w) v = i % 4 == 0 ? rng() : (i % 4 == 1 ? lo + rng() % (hi - lo + 1) : (i % 4 == 2 ? XCD_DEAL_ONE - 20000 + rng() % 40001 : rng() % 3));
            sets.push_back(w);
        }
    } else if (kind == "feedback") {
        // the running average: stays inside the clamp whatever the times, equal paces keep equal weights, a slow XCD loses
        // weight monotonically down to the clamp, a launch with an idle XCD or a nonsensical time teaches nothing
        std::mt19937 rng(7u);
        int cases = 0;
        for (int trial = 0; trial < 200; ++trial) {
            std::unique_ptr<uint32_t[]> w(new uint32_t[8]), n(new uint32_t[8]);
            std::unique_ptr<int64_t[]> t(new int64_t[8]);
            for (int x = 0; x < 8; ++x) w[x] = XCD_DEAL_ONE;
            for (int round = 0; round < 40; ++round) {
                for (int x = 0; x < 8; ++x) {
                    n[x] = 1 + rng() % 4000;
                    t[x] = trial % 3 == 0 ? static_cast<int64_t>(n[x]) * 500 : 1 + static_cast<int64_t>(rng() % 1000000);
                }
                if (trial % 3 == 1) t[3] = static_cast<int64_t>(n[3]) * 100000; // XCD 3 crawls
                xcd_deal_feedback(w.get(), n.get(), t.get());
                for (int x = 0; x < 8; ++x) CHECK(w[x] >= lo && w[x] <= hi, "feedback: weight %u of XCD %d outside the clamp", w[x], x);
                if (trial % 3 == 0) for (int x = 0; x < 8; ++x) CHECK(w[x] == XCD_DEAL_ONE, "feedback: equal paces moved XCD %d to %u", x, w[x]);
                ++cases;
            }
            // (a quarter of the way per launch, rounded to whole Q16 steps: the average stops moving within two steps of its target)
            if (trial % 3 == 1) CHECK(w[3] <= lo + 2, "feedback: the crawling XCD kept weight %u", w[3]);
            uint32_t before[8];
            for (int x = 0; x < 8; ++x) before[x] = w[x];
            n[5] = 0; xcd_deal_feedback(w.get(), n.get(), t.get());
            n[5] = 9; t[2] = 0; xcd_deal_feedback(w.get(), n.get(), t.get());
            t[2] = -5; xcd_deal_feedback(w.get(), n.get(), t.get());
            for (int x = 0; x < 8; ++x) CHECK(w[x] == before[x], "feedback: a launch without a usable time moved XCD %d", x);
            for (uint32_t nu : kUnits) for (uint32_t sx : kStreamsX) check_deal(w.get(), nu, sx, false, "feedback");
        }
        std::printf("%s: %d cases, %d failures\n", kind.c_str(), cases, failures);
        return failures ? 1 : 0;
    } else {
        std::printf("unknown kind %s\n", kind.c_str());
        return 2;
    }
    int cases = 0;
    for (const auto& w : sets) {
        std::unique_ptr<uint32_t[]> wh(new uint32_t[8]);
        for (int x = 0; x < 8; ++x) wh[x] = w[x];
        // the moves: inside the clamp, never a net gain
        std::unique_ptr<int32_t[]> e(new int32_t[8]);
        xcd_deal_moves(wh.get(), e.get());
        int64_t sum = 0;
        for (int x = 0; x < 8; ++x) { CHECK(e[x] >= -XCD_DEAL_CLAMP && e[x] <= XCD_DEAL_CLAMP, "%s: move %d of XCD %d", kind.c_str(), e[x], x); sum += e[x]; }
        CHECK(sum <= 8 && sum >= -8, "%s: the moves sum to %lld", kind.c_str(), (long long)sum);
        for (uint32_t nu : kUnits)
            for (uint32_t sx : kStreamsX) { check_deal(wh.get(), nu, sx, kind == "equal", kind.c_str()); ++cases; }
    }
    if (kind == "one_min") { // the XCD at the minimum gets fewer units than any other, 8 % fewer than equal at most
        std::unique_ptr<uint32_t[]> wh(new uint32_t[8]), off(new uint32_t[9]);
        for (int x = 0; x < 8; ++x) wh[x] = XCD_DEAL_ONE;
        wh[2] = lo;
        xcd_deal_offsets(wh.get(), 12019, 4, off.get());
        const uint32_t c2 = off[3] - off[2], eq = xcd_deal_equal_count(12019, 4, 2);
        CHECK(c2 < eq && c2 + 12019u * 8u / 100u / 8u + 2 >= eq, "one_min: XCD 2 has %u units, equal %u", c2, eq);
        for (int x = 0; x < 8; ++x) if (x != 2) CHECK(off[x + 1] - off[x] > c2, "one_min: XCD %d has no more than the slow one", x);
    }
    std::printf("%s: %d cases, %d failures\n", kind.c_str(), cases, failures);
    return failures ? 1 : 0;
}
