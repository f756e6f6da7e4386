// arg_checks.h — the argument checks of the C ABI's entries that need neither the device nor a context: pure host code over
// plain pointers (no HIP header), so that a host-only test can hold them to their definitions.  The caller keeps its own
// message, status code and limits.
#pragma once
#include <cstddef>
#include <cstdint>

namespace yams_accel {

// Do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte?  A null pointer or an empty range shares none.
inline bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    if (!a || !b || !a_bytes || !b_bytes) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}

// Do the offsets off[0 .. lists] of `lists` lists start at 0 and never decrease?  (Equal neighbours are an empty list.)  What a
// _host entry judges before it sizes an upload by off[lists]; the device checks give the same verdict over device offsets.
inline bool offsets_ascend(const uint64_t* off, uint64_t lists) {
    if (off[0] != 0) return false;
    for (uint64_t i = 0; i < lists; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

} // namespace yams_accel
