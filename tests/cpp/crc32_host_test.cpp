// crc32_host_test.cpp — yams_amd/csrc/crc32_host.h on the CPU (plain g++, AddressSanitizer + UBSan, own main): the table
// generator, x^(8 len), the GF(2) multiply, combine, and the segment plan.  The plan is exercised by walking a segment the
// way a wave of crc32_segments_kernel does — 64 lanes, granules lane + 64 t, the stride operator, one final shift per lane,
// xor — over heap blocks that hold EXACTLY the 16-byte granules the message touches, so a read outside them ends the run.
// The check is an independent bit-at-a-time loop (the stored-object form, compressed_storage_engine.cpp:49-59).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../yams_amd/csrc/crc32_host.h"

namespace cr = yams_accel::crc32;
constexpr uint32_t S = 4096;
constexpr uint32_t P = cr::kPolyCrc32;
using Tables = cr::Tables<S>;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: %s — ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static uint32_t bitwise_crc(const uint8_t* p, size_t n) {
    uint32_t crc = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int b = 0; b < 8; ++b) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}
static uint32_t bitwise_pure(const uint8_t* p, size_t n) {
    uint32_t crc = 0;
    for (size_t i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int b = 0; b < 8; ++b) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return crc;
}

static uint64_t load64(const uint8_t* p) { uint64_t v; std::memcpy(&v, p, 8); return v; }   // (little-endian host, as the device)

static uint32_t pure16(const Tables& t, uint64_t lo, uint64_t hi) {
    uint8_t b[16];
    std::memcpy(b, &lo, 8); std::memcpy(b + 8, &hi, 8);
    return cr::pure_update(t, 0, b, 16);
}
static uint32_t times_stride(const Tables& t, uint32_t r) {
    return t.stride[0][r & 255] ^ t.stride[1][(r >> 8) & 255] ^ t.stride[2][(r >> 16) & 255] ^ t.stride[3][r >> 24];
}
static void mask_head(uint32_t head, uint64_t& lo, uint64_t& hi) {
    const uint32_t hb = 8 * head;
    if (hb >= 64) { lo = 0; hi &= ~0ull << (hb - 64); } else lo &= ~0ull << hb;
}

// One segment as a wave computes it.  `gran` points at the granule that holds the segment's first byte.
static uint32_t wave_segment(const Tables& t, const uint8_t* gran, uint64_t addr, uint32_t len) {
    if (len == 0) return 0;
    const cr::Granules g = cr::granules_of(addr, len);
    uint32_t total = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        uint32_t reg = 0;
        for (uint32_t step = 0; step < 4; ++step) {
            const uint32_t k = step * 64 + lane;
            if (k >= g.body) continue;
            uint64_t lo = load64(gran + 16 * k), hi = load64(gran + 16 * k + 8);
            if (k == 0 && g.head) mask_head(g.head, lo, hi);
            reg = times_stride(t, reg) ^ pure16(t, lo, hi);
        }
        const uint32_t m = cr::lane_final_shift(g, lane);
        CHECK(m < cr::kSmallShifts, "lane shift %u", m);
        reg = cr::mulmod<P>(reg, t.small[m]);
        if (g.tail && lane == (g.body & 63)) {
            uint64_t lo = load64(gran + 16 * g.body), hi = load64(gran + 16 * g.body + 8);
            if (g.body == 0 && g.head) mask_head(g.head, lo, hi);
            const uint32_t sh = 8 * (16 - g.tail);
            if (sh >= 64) { hi = lo << (sh - 64); lo = 0; } else { hi = (hi << sh) | (lo >> (64 - sh)); lo <<= sh; }
            reg ^= pure16(t, lo, hi);
        }
        total ^= reg;
    }
    return total;
}

// A message of `len` bytes at byte `head` of a heap block of exactly the granules it touches; segments + fold.
static uint32_t planned_crc(const Tables& t, const std::vector<uint8_t>& msg, uint32_t head) {
    const size_t len = msg.size();
    const size_t grans = len ? (head + len + 15) / 16 : 0;
    uint8_t* block = grans ? static_cast<uint8_t*>(std::aligned_alloc(16, grans * 16)) : nullptr;
    if (grans) { std::memset(block, 0xA5, grans * 16); std::memcpy(block + head, msg.data(), len); }
    const uint64_t base = 0x7000000000ull;   // a 16-aligned pretend address of the block
    const uint64_t nseg = cr::segments_of(len, S);
    std::vector<uint32_t> pure(nseg);
    for (uint64_t j = 0; j < nseg; ++j) {
        const uint64_t at = j * S;
        const uint32_t sl = static_cast<uint32_t>(len - at < S ? len - at : S);
        const uint64_t addr = base + head + at;
        pure[j] = wave_segment(t, block + ((addr - base) & ~15ull), addr, sl);
        if (sl) CHECK(pure[j] == bitwise_pure(msg.data() + at, sl), "segment %llu of len %zu head %u", (unsigned long long)j, len, head);
    }
    std::free(block);
    return cr::fold<P, S>(t, pure.data(), len);
}

int main() {
    auto* tp = new Tables;
    cr::make_tables<P, S>(*tp);
    const Tables& t = *tp;
    std::mt19937_64 rng(20240611);

    // known answers
    CHECK(cr::crc(t, nullptr, 0) == 0, "empty");
    CHECK(cr::crc(t, reinterpret_cast<const uint8_t*>("123456789"), 9) == 0xCBF43926u, "check value");
    CHECK(cr::crc(t, reinterpret_cast<const uint8_t*>("a"), 1) == 0xE8B7BE43u, "a");
    { std::vector<uint8_t> z(32, 0), f(32, 0xFF), z4(4096, 0);
      CHECK(cr::crc(t, z.data(), 32) == 0x190A55ADu, "32 x 00"); CHECK(cr::crc(t, f.data(), 32) == 0xFF6CAB0Bu, "32 x FF");
      CHECK(cr::crc(t, z4.data(), 4096) == 0xC71C0011u, "4096 x 00"); }

    // the multiply: identity, commutativity, x^(8 n) against n zero bytes through the register
    for (int i = 0; i < 200; ++i) {
        const uint32_t a = static_cast<uint32_t>(rng()), b = static_cast<uint32_t>(rng());
        CHECK(cr::mulmod<P>(a, cr::kOne) == a && cr::mulmod<P>(cr::kOne, a) == a, "identity");
        CHECK(cr::mulmod<P>(a, b) == cr::mulmod<P>(b, a), "commutes");
        CHECK(cr::times_segment(t, a) == cr::shift_bytes<P>(t.pow2, a, S), "segment operator");
        CHECK(times_stride(t, a) == cr::shift_bytes<P>(t.pow2, a, cr::kStride), "stride operator");
    }
    { uint32_t r = cr::kOne;
      for (uint32_t n = 0; n < 5000; ++n) {
          CHECK(cr::x_pow_8n<P>(t.pow2, n) == r, "x^(8*%u)", n);
          if (n < cr::kSmallShifts) CHECK(t.small[n] == r, "small[%u]", n);
          r = cr::feed_byte<P>(r, 0);
      } }

    // slicing against the bit loop, every length 0..300 at every start 0..7
    { std::vector<uint8_t> buf(400);
      for (auto& b : buf) b = static_cast<uint8_t>(rng());
      for (size_t s = 0; s < 8; ++s)
          for (size_t n = 0; n <= 300; ++n) CHECK(cr::crc(t, buf.data() + s, n) == bitwise_crc(buf.data() + s, n), "slicing %zu+%zu", s, n); }

    // combine
    { std::vector<uint8_t> buf(3 * S + 100);
      for (auto& b : buf) b = static_cast<uint8_t>(rng());
      const size_t lens_b[] = {0, 1, 2, S - 1, S, S + 1, 2 * S + 7};
      for (size_t lb : lens_b)
          for (size_t la : {size_t(0), size_t(1), size_t(S), size_t(S + 93)}) {
              const uint32_t ca = bitwise_crc(buf.data(), la), cb = bitwise_crc(buf.data() + la, lb);
              CHECK(cr::combine<P>(t.pow2, ca, cb, lb) == bitwise_crc(buf.data(), la + lb), "combine %zu + %zu", la, lb);
          } }
    // ... and of lengths no buffer has: crc(A || 0^n) by combine equals crc(A) shifted, split two ways
    for (uint64_t n : {1ull << 32, (1ull << 40) - 1, 1ull << 40}) {
        const uint32_t ca = 0xCBF43926u;
        const uint64_t h = n / 3;
        // crc(0^h) for huge h from the register: ~(FFFFFFFF * x^(8h))
        const uint32_t z1 = ~cr::shift_bytes<P>(t.pow2, 0xFFFFFFFFu, h), z2 = ~cr::shift_bytes<P>(t.pow2, 0xFFFFFFFFu, n - h);
        const uint32_t zn = ~cr::shift_bytes<P>(t.pow2, 0xFFFFFFFFu, n);
        CHECK(cr::combine<P>(t.pow2, z1, z2, n - h) == zn, "zeros %llu", (unsigned long long)n);
        CHECK(cr::combine<P>(t.pow2, cr::combine<P>(t.pow2, ca, z1, h), z2, n - h) == cr::combine<P>(t.pow2, ca, zn, n), "assoc %llu", (unsigned long long)n);
    }

    // the segment plan: geometry ...
    CHECK(cr::segments_of(0, S) == 1 && cr::segments_of(1, S) == 1 && cr::segments_of(S, S) == 1 && cr::segments_of(S + 1, S) == 2, "segments_of");
    for (uint32_t head = 0; head < 16; ++head)
        for (uint32_t len = 1; len <= S; ++len) {
            const cr::Granules g = cr::granules_of(head, len);
            CHECK(g.body <= 256 && g.body * 16 + g.tail == head + len, "granules %u %u", head, len);
            for (uint32_t lane : {0u, 1u, 31u, 62u, 63u}) CHECK(cr::lane_final_shift(g, lane) < cr::kSmallShifts, "shift %u %u %u", head, len, lane);
        }
    // ... every alignment x lengths 0..80, the segment edges at heads 0, 1, 15, random long ones
    for (uint32_t head = 0; head < 16; ++head)
        for (size_t len = 0; len <= 80; ++len) {
            std::vector<uint8_t> m(len);
            for (auto& b : m) b = static_cast<uint8_t>(rng());
            CHECK(planned_crc(t, m, head) == bitwise_crc(m.data(), len), "plan head %u len %zu", head, len);
        }
    for (uint32_t head : {0u, 1u, 15u})
        for (size_t len : {size_t(S - 1), size_t(S), size_t(S + 1), size_t(2 * S - 1), size_t(2 * S), size_t(2 * S + 1), size_t(3 * S + 5), size_t(65 * S + 17)}) {
            std::vector<uint8_t> m(len);
            for (auto& b : m) b = static_cast<uint8_t>(rng());
            CHECK(planned_crc(t, m, head) == bitwise_crc(m.data(), len), "plan head %u len %zu", head, len);
            std::vector<uint8_t> z(len, 0);
            CHECK(planned_crc(t, z, head) == bitwise_crc(z.data(), len), "zeros head %u len %zu", head, len);
        }
    for (int i = 0; i < 60; ++i) {
        std::vector<uint8_t> m(rng() % (5 * S));
        for (auto& b : m) b = static_cast<uint8_t>(rng());
        const uint32_t head = static_cast<uint32_t>(rng() % 16);
        CHECK(planned_crc(t, m, head) == bitwise_crc(m.data(), m.size()), "plan random %zu at %u", m.size(), head);
    }
    delete tp;
    std::printf("crc32_host_test: %s (%d failures)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
