// crc32_host.h — the arithmetic of the batched CRC-32 that needs no device: the table generator, x^(8 len) mod P, the
// GF(2) multiply, combine, and the segment plan.  Plain C++17, no HIP call, no global: the kernels (crc32_kernels.hip), the
// C ABI (crc32_api.cpp) and tests/cpp/crc32_host_test.cpp all include it.
//
// Representation (the reflected one every table-driven CRC-32 uses): bit 31 of a register is the coefficient of x^0, bit 0
// that of x^31; one zero byte fed to the register multiplies it by x^8 mod P.  POLY is the reflected polynomial
// (0xEDB88320 for the standard CRC-32: compression_utils.cpp:31-52, compressed_storage_engine.cpp:49-59).
//
// pure(M) is the register after M starting from 0 with no final xor: pure(A || B) = pure(A) * x^(8|B|) ^ pure(B), and the
// finalised CRC is crc(M) = ~(0xFFFFFFFF * x^(8|M|) ^ pure(M)): the initial value is a prefix of the Horner chain.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YAMS_CRC_HD __host__ __device__
#else
#define YAMS_CRC_HD
#endif

namespace yams_accel {
namespace crc32 {

constexpr uint32_t kPolyCrc32 = 0xEDB88320u;
constexpr uint32_t kOne = 0x80000000u;          // x^0
constexpr uint32_t kStride = 1024;              // bytes one wave reads per step: 64 lanes x 16
constexpr uint32_t kSmallShifts = 1024;         // x^(8 m) is tabulated for m < kSmallShifts (a lane's final shift inside a segment)
constexpr uint32_t kSmallShiftBits = 10;
constexpr uint32_t kPow2 = 64;                  // x^(2^k) for k < kPow2

// a * x mod P
template <uint32_t POLY> YAMS_CRC_HD constexpr uint32_t times_x(uint32_t a) { return (a >> 1) ^ (POLY & (0u - (a & 1u))); }

// a * b mod P (zlib's multmodp, branch-free: the device runs it once per lane and segment)
template <uint32_t POLY> YAMS_CRC_HD constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = times_x<POLY>(b);
    }
    return p;
}

// One byte through the register (the bit-at-a-time loop of compressed_storage_engine.cpp:49-59, on a raw register).
template <uint32_t POLY> constexpr uint32_t feed_byte(uint32_t reg, uint8_t b) {
    reg ^= b;
    for (int i = 0; i < 8; ++i) reg = times_x<POLY>(reg);
    return reg;
}

// Everything the kernels look up.  slice[k][b] = pure(b followed by k zero bytes): slicing-by-8.  stride[k][b] /
// segment[k][b] = (b in byte k of a register) * x^(8 kStride) resp. x^(8 S): the two fixed shift operators.
// small[m] = x^(8 m); pow2[k] = x^(2^k).
template <uint32_t SEG> struct Tables {
    uint32_t slice[8][256];
    uint32_t stride[4][256];
    uint32_t segment[4][256];
    uint32_t small[kSmallShifts];
    uint32_t pow2[kPow2];
};

// x^(8 len) mod P by square-and-multiply over pow2 (lengths up to 2^61).
template <uint32_t POLY> constexpr uint32_t x_pow_8n(const uint32_t* pow2, uint64_t len) {
    uint32_t p = kOne;
    for (uint32_t k = 3; len; len >>= 1, ++k)
        if (len & 1) p = mulmod<POLY>(pow2[k], p);
    return p;
}

template <uint32_t POLY> constexpr void fill_shift_operator(uint32_t (*op)[256], uint32_t factor) {
    uint32_t basis[32] = {};
    for (int bit = 0; bit < 32; ++bit) basis[bit] = mulmod<POLY>(1u << bit, factor);
    for (int k = 0; k < 4; ++k)
        for (uint32_t b = 0; b < 256; ++b) {
            uint32_t v = 0;
            for (int i = 0; i < 8; ++i)
                if (b & (1u << i)) v ^= basis[8 * k + i];
            op[k][b] = v;
        }
}

template <uint32_t POLY, uint32_t SEG> constexpr void make_tables(Tables<SEG>& t) {
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t r = feed_byte<POLY>(0, static_cast<uint8_t>(b));
        for (int k = 0; k < 8; ++k) { t.slice[k][b] = r; r = feed_byte<POLY>(r, 0); }
    }
    t.pow2[0] = kOne >> 1;     // x^1
    for (uint32_t k = 1; k < kPow2; ++k) t.pow2[k] = mulmod<POLY>(t.pow2[k - 1], t.pow2[k - 1]);
    t.small[0] = kOne;
    for (uint32_t m = 1; m < kSmallShifts; ++m) t.small[m] = feed_byte<POLY>(t.small[m - 1], 0);
    fill_shift_operator<POLY>(t.stride, x_pow_8n<POLY>(t.pow2, kStride));
    fill_shift_operator<POLY>(t.segment, x_pow_8n<POLY>(t.pow2, SEG));
}

// reg * x^(8 len)
template <uint32_t POLY> constexpr uint32_t shift_bytes(const uint32_t* pow2, uint32_t reg, uint64_t len) {
    return len == 0 || reg == 0 ? reg : mulmod<POLY>(x_pow_8n<POLY>(pow2, len), reg);
}

// CRC-32 of A || B from the finalised crc(A), crc(B) and |B| (updateCRC32 by linearity: the initial and final xors of
// the two halves cancel; zlib's crc32_combine).
template <uint32_t POLY> constexpr uint32_t combine(const uint32_t* pow2, uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return shift_bytes<POLY>(pow2, crc_a, len_b) ^ crc_b;
}

// Slicing-by-8 over host memory: pure(M) continued from `reg`.
template <uint32_t SEG> inline uint32_t pure_update(const Tables<SEG>& t, uint32_t reg, const uint8_t* p, size_t n) {
    while (n >= 8) {
        const uint32_t w0 = (static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 |
                             static_cast<uint32_t>(p[3]) << 24) ^ reg;
        reg = t.slice[7][w0 & 255] ^ t.slice[6][(w0 >> 8) & 255] ^ t.slice[5][(w0 >> 16) & 255] ^ t.slice[4][w0 >> 24] ^
              t.slice[3][p[4]] ^ t.slice[2][p[5]] ^ t.slice[1][p[6]] ^ t.slice[0][p[7]];
        p += 8; n -= 8;
    }
    for (; n; --n, ++p) reg = t.slice[0][(reg ^ *p) & 255] ^ (reg >> 8);
    return reg;
}
template <uint32_t SEG> inline uint32_t crc(const Tables<SEG>& t, const uint8_t* p, size_t n) {
    return ~pure_update(t, 0xFFFFFFFFu, p, n);
}

// reg * x^(8 SEG) through the segment operator (the fold pass's Horner step)
template <uint32_t SEG> constexpr uint32_t times_segment(const Tables<SEG>& t, uint32_t reg) {
    return t.segment[0][reg & 255] ^ t.segment[1][(reg >> 8) & 255] ^ t.segment[2][(reg >> 16) & 255] ^ t.segment[3][reg >> 24];
}

// ---- the segment plan -------------------------------------------------------------------------------------------------
// A message of `len` bytes is cut into segments of SEG bytes, the last one partial; an empty message still owns ONE
// (empty) segment, so that the segment -> message walk of the kernel advances by exactly one message at a time.
YAMS_CRC_HD constexpr uint64_t segments_of(uint64_t len, uint32_t seg) { return len == 0 ? 1 : (len + seg - 1) / seg; }

// How one segment [addr, addr + len) lies over 16-byte granules: `head` bytes of granule 0 in front of it, `body` whole
// granules that end at or before its end (granule 0 counts when the segment reaches its end), `tail` bytes (0..15) in one
// more granule.  Only these body + (tail ? 1 : 0) granules are read.
struct Granules { uint32_t head, body, tail; };
YAMS_CRC_HD constexpr Granules granules_of(uint64_t addr, uint32_t len) {
    const uint32_t head = static_cast<uint32_t>(addr & 15u);
    return Granules{head, (head + len) >> 4, (head + len) & 15u};
}
// Lane `lane` of the wave owns body granules lane, lane + 64, ...; after its last one the register still has to travel
// 16 * (body - 1 - last) + tail bytes to the segment's end: always below kSmallShifts.
YAMS_CRC_HD constexpr uint32_t lane_final_shift(const Granules& g, uint32_t lane) {
    if (lane >= g.body) return 0;
    const uint32_t last = lane + ((g.body - 1 - lane) & ~63u);
    return 16u * (g.body - 1 - last) + g.tail;
}

// The fold pass as the host computes it: the finalised CRC of a message from the pure values of its segments.
template <uint32_t POLY, uint32_t SEG> inline uint32_t fold(const Tables<SEG>& t, const uint32_t* seg_pure, uint64_t len) {
    uint32_t reg = 0xFFFFFFFFu;
    const uint64_t full = len / SEG;
    for (uint64_t j = 0; j < full; ++j) reg = times_segment(t, reg) ^ seg_pure[j];
    const uint64_t rest = len - full * SEG;
    if (rest) reg = shift_bytes<POLY>(t.pow2, reg, rest) ^ seg_pure[full];
    return ~reg;
}

} // namespace crc32
} // namespace yams_accel
