// checksum_shell_test.cpp — driver of include/yams_accel/checksum.hpp: AccelCrc32 over the plugin's content_checksum_v1
// (dlopen of the library named by argv[1]; needs a device).  The check is a bit-at-a-time loop written here.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "yams_accel/checksum.hpp"

static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, what); } } while (0)

static uint32_t bitwise(uint32_t crc, const std::vector<std::byte>& d) {    // updateCRC32's loop, one bit at a time
    crc ^= 0xFFFFFFFFu;
    for (std::byte b : d) {
        crc ^= static_cast<uint8_t>(b);
        for (int i = 0; i < 8; ++i) crc = (crc >> 1) ^ ((crc & 1u) ? 0xEDB88320u : 0u);
    }
    return crc ^ 0xFFFFFFFFu;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: checksum_shell_test <libyams_mi355x_accel.so>\n"); return 2; }
    auto plugin = yams::accel::Plugin::load(argv[1]);
    if (!plugin) { std::printf("plugin load failed: %s\n", plugin.error().message.c_str()); return 2; }
    auto vt = plugin.value()->getInterface<yams_content_checksum_v1>(YAMS_IFACE_CONTENT_CHECKSUM_V1, YAMS_IFACE_CONTENT_CHECKSUM_V1_VERSION);
    if (!vt) { std::printf("content_checksum_v1 not served\n"); return 2; }
    CHECK(vt.value()->abi_version == 1, "version");
    yams::compression::AccelCrc32 crc(plugin.value(), vt.value());

    const char* check = "123456789";
    std::vector<std::byte> nine(9);
    std::memcpy(nine.data(), check, 9);
    CHECK(crc.calculateCRC32(nine) == 0xCBF43926u, "check value");
    CHECK(crc.calculateCRC32({}) == 0u, "empty");

    std::mt19937_64 rng(7);
    std::vector<std::vector<std::byte>> bufs;
    for (size_t len : {size_t(0), size_t(1), size_t(15), size_t(16), size_t(17), size_t(4095), size_t(4096), size_t(4097), size_t(3 * 4096 + 5), size_t(300000)}) {
        std::vector<std::byte> b(len);
        for (auto& x : b) x = static_cast<std::byte>(rng());
        bufs.push_back(std::move(b));
    }
    std::vector<std::span<const std::byte>> spans(bufs.begin(), bufs.end());
    auto many = crc.calculateMany(spans);
    CHECK(many.has_value(), "calculateMany");
    if (many)
        for (size_t i = 0; i < bufs.size(); ++i) CHECK(many.value()[i] == bitwise(0, bufs[i]), "calculateMany value");
    // updateCRC32 continues a finalised value: the CRC of the concatenation
    for (size_t i = 0; i + 1 < bufs.size(); ++i) {
        const uint32_t a = bitwise(0, bufs[i]);
        CHECK(crc.updateCRC32(a, bufs[i + 1]) == bitwise(a, bufs[i + 1]), "updateCRC32");
    }
    std::vector<std::pair<std::span<const std::byte>, uint32_t>> list;
    for (size_t i = 0; i < bufs.size(); ++i) list.emplace_back(spans[i], bitwise(0, bufs[i]) ^ (i % 3 == 1 ? 0x10u : 0u));
    auto valid = crc.verifyMany(list);
    CHECK(valid.has_value(), "verifyMany");
    if (valid)
        for (size_t i = 0; i < bufs.size(); ++i) CHECK(valid.value()[i] == (i % 3 != 1), "verifyMany value");
    std::printf("checksum_shell_test: %s (%d failures)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
