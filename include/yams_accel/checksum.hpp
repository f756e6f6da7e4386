// checksum.hpp — the compressed store's checksum over the content_checksum_v1 vtable:
//   * calculateCRC32 / updateCRC32 carry the signatures of yams::compression (include/yams/compression/
//     compression_utils.h:16, 24; src/compression/compression_utils.cpp:31-52): the standard CRC-32, and its continuation
//     from a finalised value — computed here as combine(crc, CRC-32(data), |data|), which is what feeding `data` to the
//     running register gives, by linearity.
//   * calculateMany / verifyMany are the batched forms a device needs: header.uncompressedCRC32 of every new chunk of a
//     batch (compressed_storage_engine.cpp:524) in one call, and the read side's comparison (:594-627,
//     storage_engine.cpp:102-120) for a list of objects.
// The reference's functions return a bare uint32_t; a call the plugin does not serve (no device: YAMS_ERR_UNSUPPORTED) goes
// to the host's own function given at construction, and throws std::runtime_error where there is none.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <span>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "plugin.hpp"

namespace yams::compression {

class AccelCrc32 {
public:
    using HostCrc32 = std::function<uint32_t(std::span<const std::byte>)>;   // e.g. yams::compression::calculateCRC32
    AccelCrc32(std::shared_ptr<accel::Plugin> plugin, yams_content_checksum_v1* vt, HostCrc32 hostCrc = nullptr)
        : plugin_(std::move(plugin)), vt_(vt), hostCrc_(std::move(hostCrc)) {}

    [[nodiscard]] uint32_t calculateCRC32(std::span<const std::byte> data) {
        uint32_t out = 0;
        const yams_status_t st = vt_->crc32(vt_->self, reinterpret_cast<const uint8_t*>(data.data()), data.size(), &out);
        if (st == YAMS_OK) return out;
        if (st == YAMS_ERR_UNSUPPORTED && hostCrc_) return hostCrc_(data);
        throw std::runtime_error("content_checksum_v1.crc32 failed with status " + std::to_string(static_cast<int>(st)));
    }
    [[nodiscard]] uint32_t updateCRC32(uint32_t crc, std::span<const std::byte> data) {
        return combine(crc, calculateCRC32(data), data.size());
    }
    // CRC-32 of every buffer, one device pass
    [[nodiscard]] Result<std::vector<uint32_t>> calculateMany(const std::vector<std::span<const std::byte>>& buffers) {
        std::vector<uint32_t> out(buffers.size());
        if (buffers.empty()) return out;
        std::vector<const uint8_t*> ptrs; std::vector<size_t> lens;
        for (const auto& b : buffers) { ptrs.push_back(reinterpret_cast<const uint8_t*>(b.data())); lens.push_back(b.size()); }
        const yams_status_t st = vt_->crc32_many(vt_->self, ptrs.data(), lens.data(), buffers.size(), out.data());
        if (st == YAMS_ERR_UNSUPPORTED && hostCrc_) {
            for (size_t i = 0; i < buffers.size(); ++i) out[i] = hostCrc_(buffers[i]);
            return out;
        }
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "content_checksum_v1.crc32_many failed"};
        return out;
    }
    // valid[i] = (CRC-32 of buffers[i].first == buffers[i].second): the read side's check for a list of objects
    [[nodiscard]] Result<std::vector<bool>> verifyMany(const std::vector<std::pair<std::span<const std::byte>, uint32_t>>& buffers) {
        std::vector<bool> out(buffers.size());
        if (buffers.empty()) return out;
        std::vector<const uint8_t*> ptrs; std::vector<size_t> lens; std::vector<uint32_t> expected;
        for (const auto& b : buffers) {
            ptrs.push_back(reinterpret_cast<const uint8_t*>(b.first.data())); lens.push_back(b.first.size()); expected.push_back(b.second);
        }
        std::vector<uint8_t> valid(buffers.size(), 0);
        const yams_status_t st = vt_->verify_many(vt_->self, ptrs.data(), lens.data(), expected.data(), buffers.size(), valid.data());
        if (st == YAMS_ERR_UNSUPPORTED && hostCrc_) {
            for (size_t i = 0; i < buffers.size(); ++i) out[i] = hostCrc_(buffers[i].first) == buffers[i].second;
            return out;
        }
        if (st != YAMS_OK) return Error{accel::mapStatus(st), "content_checksum_v1.verify_many failed"};
        for (size_t i = 0; i < buffers.size(); ++i) out[i] = valid[i] != 0;
        return out;
    }

    // CRC-32 of A || B from crc(A), crc(B) and |B| (what yams_crc32_combine of the flat ABI computes; restated here so
    // that the shell needs nothing but the vtable).  Registers are reflected: bit 31 is x^0.
    [[nodiscard]] static uint32_t combine(uint32_t crcA, uint32_t crcB, uint64_t lenB) {
        if (lenB == 0) return crcA ^ crcB;       // (crc of the empty message is 0)
        uint32_t power = 0x80000000u >> 1, shift = 0x80000000u;    // x^1 -> x^(2^k); x^(8 lenB)
        power = mul(power, power); power = mul(power, power); power = mul(power, power);    // x^8
        for (; lenB; lenB >>= 1, power = mul(power, power))
            if (lenB & 1) shift = mul(shift, power);
        return mul(crcA, shift) ^ crcB;
    }

private:
    static uint32_t mul(uint32_t a, uint32_t b) {       // a * b mod the CRC-32 polynomial
        uint32_t p = 0;
        for (int i = 0; i < 32; ++i) {
            if (a & 0x80000000u) p ^= b;
            a <<= 1;
            b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u);
        }
        return p;
    }
    std::shared_ptr<accel::Plugin> plugin_;
    yams_content_checksum_v1* vt_;
    HostCrc32 hostCrc_;
};

} // namespace yams::compression
