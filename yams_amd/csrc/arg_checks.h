// arg_checks.h — the argument checks of the C ABI's entries that need neither the device nor a context: pure host code over
// plain pointers (no HIP header), so that a host-only test can hold them to their definitions.  The caller keeps its own
// message, status code and limits.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

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

// Is every idx[0 .. count) below `limit`?  An entry equal to `sentinel` is allowed when allow_sentinel says so ("none").
inline bool indices_below(const uint32_t* idx, uint64_t count, uint64_t limit, bool allow_sentinel = false, uint32_t sentinel = 0xffffffffu) {
    for (uint64_t i = 0; i < count; ++i)
        if (idx[i] >= limit && !(allow_sentinel && idx[i] == sentinel)) return false;
    return true;
}

// packed[i] = rows[select[i]], i < m, rows of `dim` floats: what a _host entry uploads when only the selected rows travel.
// packed holds m * dim floats; every select[i] has been judged (indices_below) by the caller.
inline void gather_rows(const float* rows, uint32_t dim, const uint32_t* select, uint64_t m, float* packed) {
    for (uint64_t i = 0; i < m; ++i)
        std::memcpy(packed + static_cast<size_t>(i) * dim, rows + static_cast<size_t>(select[i]) * dim, static_cast<size_t>(dim) * 4);
}

} // namespace yams_accel
