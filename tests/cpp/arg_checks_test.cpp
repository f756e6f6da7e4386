// arg_checks_test.cpp — yams_amd/csrc/arg_checks.h (the argument checks that need neither the device nor a context) held to its
// definitions on the CPU.  A stand-alone program: plain g++ with AddressSanitizer and UBSan, no ROCm include path.  The offsets
// arrays live on the heap with exactly lists + 1 entries, the index lists, rows and packed rows with exactly their contracted
// lengths, so a read or write past one ends the run.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../yams_amd/csrc/arg_checks.h"

using yams_accel::gather_rows;
using yams_accel::indices_below;
using yams_accel::offsets_ascend;
using yams_accel::overlaps;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// the expression sgc_api.cpp used before it took overlaps(): two ranges of equal length
static bool equal_length_overlap(const void* rows, const void* out, size_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(rows), b = reinterpret_cast<uintptr_t>(out);
    return a < b + bytes && b < a + bytes;
}

static void test_overlaps() {
    std::vector<unsigned char> buf(64);
    unsigned char* p = buf.data();
    // adjacent: one ends where the other begins
    CHECK(!overlaps(p, 16, p + 16, 16));
    CHECK(!overlaps(p + 16, 16, p, 16));
    // one byte shared at either end
    CHECK(overlaps(p, 17, p + 16, 16));
    CHECK(overlaps(p + 16, 16, p, 17));
    CHECK(overlaps(p + 15, 16, p, 16));
    CHECK(overlaps(p, 16, p + 15, 16));
    // a range inside the other, and a range against itself
    CHECK(overlaps(p, 64, p + 20, 4));
    CHECK(overlaps(p + 20, 4, p, 64));
    CHECK(overlaps(p + 20, 1, p + 20, 1));
    // apart
    CHECK(!overlaps(p, 8, p + 40, 8));
    // a null pointer never overlaps, whatever the lengths; nor does an empty range, even inside the other
    CHECK(!overlaps(nullptr, 64, p, 64));
    CHECK(!overlaps(p, 64, nullptr, 64));
    CHECK(!overlaps(nullptr, 64, nullptr, 64));
    CHECK(!overlaps(p + 8, 0, p, 64));
    CHECK(!overlaps(p, 64, p + 8, 0));
    CHECK(!overlaps(p, 0, p, 0));
    // equal lengths: the verdict of the expression sgc_api.cpp had, at every pair of starts and every length that fits
    for (size_t bytes = 1; bytes <= 24; ++bytes)
        for (size_t i = 0; i + bytes <= 64; ++i)
            for (size_t j = 0; j + bytes <= 64; ++j)
                CHECK(overlaps(p + i, bytes, p + j, bytes) == equal_length_overlap(p + i, p + j, bytes));
}

// the verdict over a heap array of exactly off.size() entries (lists = off.size() - 1)
static bool ascend(const std::vector<uint64_t>& off) {
    std::unique_ptr<uint64_t[]> heap(new uint64_t[off.size()]);
    for (size_t i = 0; i < off.size(); ++i) heap[i] = off[i];
    return offsets_ascend(heap.get(), off.size() - 1);
}

static void test_offsets() {
    CHECK(ascend({0, 3, 3, 7, 12}));
    // a first offset that is not 0
    CHECK(!ascend({1, 3, 3, 7, 12}));
    CHECK(!ascend({5, 5}));
    // a decrease at the first pair (only a start that is not 0 can decrease there), the first pair after it, a middle and
    // the last pair
    CHECK(!ascend({4, 3, 7, 12}));
    CHECK(!ascend({0, 4, 3, 7, 12}));
    CHECK(!ascend({0, 3, 8, 7, 12}));
    CHECK(!ascend({0, 3, 3, 7, 6}));
    CHECK(!ascend({0, 1ull << 63, (1ull << 63) - 1}));      // (compared as unsigned 64-bit values)
    // equal neighbours are empty lists
    CHECK(ascend({0, 0, 0, 0}));
    CHECK(ascend({0, 5, 5, 5, 9, 9}));
    // a single list, empty or not; no list at all
    CHECK(ascend({0, 0}));
    CHECK(ascend({0, 11}));
    CHECK(ascend({0}));
    CHECK(!ascend({2}));
    CHECK(ascend({0, ~0ull}));
}

// a heap copy of exactly v.size() entries (an allocation of no bytes for an empty list: any read of it ends the run)
template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> heap(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) heap[i] = v[i];
    return heap;
}

static bool below(const std::vector<uint32_t>& idx, uint64_t limit, bool allow_sentinel = false) {
    return indices_below(exact(idx).get(), idx.size(), limit, allow_sentinel);
}

static void test_indices() {
    // an empty list holds no index that could be out of range, whatever the limit
    CHECK(below({}, 0));
    CHECK(below({}, 5, true));
    CHECK(indices_below(nullptr, 0, 0));
    CHECK(below({0, 4, 2, 4}, 5));
    // the last index equal to the limit; the first; one past it
    CHECK(!below({0, 4, 2, 5}, 5));
    CHECK(!below({5, 0}, 5));
    CHECK(!below({0, 6, 1}, 5));
    CHECK(!below({0}, 0));
    // the sentinel: allowed only when asked for, and only that value
    CHECK(below({0xffffffffu, 1, 0xffffffffu}, 2, true));
    CHECK(!below({0xffffffffu, 1}, 2, false));
    CHECK(!below({0xffffffffu, 1}, 2));
    CHECK(!below({0xfffffffeu}, 2, true));
    CHECK(!below({0xffffffffu, 2}, 2, true));
    CHECK(indices_below(exact<uint32_t>({7, 2}).get(), 2, 3, true, 7));      // (a caller's own sentinel)
    // a limit above 2^32 - 1 admits every uint32 (limits are the callers' uint64 row counts)
    CHECK(below({0xffffffffu}, 1ull << 32));
}

// gather_rows over heap arrays of exactly the contracted lengths: rows [n][dim], select [m], packed [m][dim]
static std::vector<float> gathered(const std::vector<float>& rows, uint32_t dim, const std::vector<uint32_t>& select) {
    auto r = exact(rows);
    auto s = exact(select);
    std::unique_ptr<float[]> packed(new float[select.size() * dim]);
    gather_rows(r.get(), dim, s.get(), select.size(), packed.get());
    return std::vector<float>(packed.get(), packed.get() + select.size() * dim);
}

static void test_gather() {
    const std::vector<float> rows = {0.f, 1.f, 2.f, 10.f, 11.f, 12.f, 20.f, 21.f, 22.f};      // [3][3]
    // m == 0: nothing is read, nothing is written
    CHECK(gathered(rows, 3, {}).empty());
    CHECK(gathered({}, 3, {}).empty());
    // the order of select is the order of packed; a repeated index is copied each time; the last row ends at the array's end
    CHECK((gathered(rows, 3, {2, 0, 2, 2}) == std::vector<float>{20.f, 21.f, 22.f, 0.f, 1.f, 2.f, 20.f, 21.f, 22.f, 20.f, 21.f, 22.f}));
    CHECK((gathered(rows, 3, {1}) == std::vector<float>{10.f, 11.f, 12.f}));
    // dim == 1: the same array as nine rows of one value
    CHECK((gathered(rows, 1, {8, 0, 8, 3}) == std::vector<float>{22.f, 0.f, 22.f, 10.f}));
}

int main() {
    test_overlaps();
    test_offsets();
    test_indices();
    test_gather();
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
