// grow_buf.h — the device buffer behind a corpus mirror (plugin.cpp): it grows in place and is never unmapped under a reader.
#pragma once
#include <algorithm>
#include <cstdio>
#include <map>
#include <mutex>
#include <vector>

#include "accel_ctx.h"

namespace yams_accel {
namespace door {

// ------------------------------------------------------------------------------------------------
// A device buffer that grows IN PLACE: one virtual range reserved up front, physical chunks mapped
// behind it as rows arrive (hipMemAddressReserve / hipMemCreate / hipMemMap / hipMemSetAccess).
// Appending to a 38 GB mirror maps a few more chunks; nothing is reallocated or copied, pointers
// handed to running searches stay valid.  (Probed on MI355X: scripts/ubench/vmm_probe.hip.)
//
// A virtual address is NEVER reused for a different mapping: scripts/ubench/vmm_stale.hip shows that
// after hipMemUnmap + a new hipMemMap at the same address, kernels read through stale translations
// (wrong data in 1-60 % of the trials, even on the stream that did the copy), while re-filling a range
// that stays mapped is always seen.  So a buffer whose corpus is destroyed is PARKED, mapping intact,
// and handed to the next corpus on that device (park / unpark below); physical memory goes back to the
// driver only when the process exits.
// Parked mappings are adopted BEST-FIT at the next buffer's first ensure() (the smallest one that holds the
// request; a mapping more than 4x larger than the request is left for a corpus that needs it, a fresh range is
// reserved instead).  Physical memory goes back to the driver (a) when a device allocation fails while
// mappings are parked (evict_parked: unmap + RETIRE the range — it stays reserved and is never mapped
// again, so no stale translation can be hit), and (b) at yams_plugin_shutdown, when no kernel can still be
// reading through the translations.  Only address space is spent on retired ranges.
// Falls back to allocate-copy-free growth if the driver refuses the virtual-memory calls.
// ------------------------------------------------------------------------------------------------
#ifdef YAMS_ACCEL_MEASURE
#define GROW_TRACE(what, err) std::fprintf(stderr, "[yams_mi355x_accel] GrowBuf role %d: %s failed (%s); want %zu mapped %zu reserved %zu\n", role, what, hipGetErrorString(err), bytes, mapped, reserved)
#else
#define GROW_TRACE(what, err) ((void)0)
#endif
struct GrowBuf {
    int device = 0;
    int role = 0;               // which array of a shard this is (buffers are parked and reused per role)
    unsigned char* base = nullptr;
    size_t reserved = 0, mapped = 0;
    bool plain = false; // fallback mode: `base` is a hipMalloc allocation of `mapped` bytes
    std::vector<size_t> chunk_end; // end offset of every physical chunk mapped so far

    static constexpr size_t kGran = 2ull << 20;
    template <typename T> T* as() const { return reinterpret_cast<T*>(base); }

    // reserve_bytes: the size of the virtual range if this is the buffer's first use (per role: a fixed
    // fraction of the device's memory, so parked buffers fit every later corpus)
    bool ensure(size_t bytes, size_t reserve_bytes) {
        if (bytes <= mapped) return true;
        (void)hipSetDevice(device);
        if (!plain && !base) adopt(bytes); // a parked mapping of this (device, role) that fits, if there is one
        if (bytes <= mapped) return true;
        if (!plain && !base) {
            size_t want = std::max(reserve_bytes, bytes);
            want = (want + kGran - 1) / kGran * kGran;
            void* va = nullptr;
            if (hipMemAddressReserve(&va, want, 0, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); plain = true; }
            else { base = static_cast<unsigned char*>(va); reserved = want; }
        }
        if (!plain && bytes > reserved) { GROW_TRACE("beyond reservation", hipSuccess); return false; } // (sized to the device's memory)
        if (!plain) {
            // geometric chunks: at least 32 MiB (small side arrays: 2 MiB), at least a quarter of what is mapped
            size_t add = std::max<size_t>(bytes - mapped, std::max<size_t>(reserved >= (1ull << 30) ? 32ull << 20 : kGran, mapped / 4));
            add = (add + kGran - 1) / kGran * kGran;
            if (mapped + add > reserved) add = reserved - mapped;
            hipMemAllocationProp prop{};
            prop.type = hipMemAllocationTypePinned;
            prop.location.type = hipMemLocationTypeDevice;
            prop.location.id = device;
            hipMemGenericAllocationHandle_t h;
            hipError_t e = yams_accel::ya_mem_create(&h, add, &prop);
            if (e != hipSuccess && evict_parked(device)) { // parked mirrors of destroyed corpora give their memory back first
                (void)hipGetLastError();
                if (mapped + (bytes - mapped + kGran - 1) / kGran * kGran <= reserved) add = (bytes - mapped + kGran - 1) / kGran * kGran;
                e = yams_accel::ya_mem_create(&h, add, &prop);
            }
            if (e != hipSuccess) { GROW_TRACE("hipMemCreate", e); (void)hipGetLastError(); return false; }
            hipMemAccessDesc acc{};
            acc.location = prop.location;
            acc.flags = hipMemAccessFlagsProtReadWrite;
            e = hipMemMap(base + mapped, add, 0, h, 0);
            // access is set over the WHOLE mapped range: on a sub-range that starts at a later chunk the call
            // returns "invalid argument" as soon as chunk sizes differ (scripts/ubench/vmm_map.hip)
            const bool was_mapped = e == hipSuccess;
            if (e == hipSuccess) e = hipMemSetAccess(base, mapped + add, &acc, 1);
            if (e != hipSuccess && was_mapped) (void)hipMemUnmap(base + mapped, add); // never touched: safe to unmap
            if (e != hipSuccess) { GROW_TRACE("hipMemMap/SetAccess", e); (void)hipGetLastError(); (void)hipMemRelease(h); return false; }
            (void)hipMemRelease(h); // the mapping keeps the memory alive; it is never unmapped (see above)
            mapped += add;
            chunk_end.push_back(mapped);
            return true;
        }
        // fallback: allocate, copy, free
        const size_t want = std::max(bytes, mapped + mapped / 2);
        void* nd = nullptr;
        if (yams_accel::ya_malloc(&nd, want) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (mapped && hipMemcpy(nd, base, mapped, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(nd); return false; }
        if (base) (void)hipFree(base);
        base = static_cast<unsigned char*>(nd);
        mapped = want;
        return true;
    }
    // Host -> device copy into [off, off+bytes).  The runtime's copy wants its destination inside ONE
    // allocation, so a range that crosses physical chunks goes as one copy per chunk.
    bool h2d(size_t off, const void* src, size_t bytes, hipStream_t stream) const {
        if (off + bytes > mapped) return false;
        const unsigned char* sp = static_cast<const unsigned char*>(src);
        size_t ci = 0;
        while (bytes) {
            size_t end = off + bytes;
            if (!plain) {
                while (ci < chunk_end.size() && chunk_end[ci] <= off) ++ci;
                if (ci < chunk_end.size()) end = std::min(end, chunk_end[ci]);
            }
            if (yams_accel::staged_h2d(base + off, sp, end - off, stream) != hipSuccess) { (void)hipGetLastError(); return false; } // (pinned ring: link rate from pageable memory)
            sp += end - off; bytes -= end - off; off = end;
        }
        return true;
    }
    void release();            // parks the mapping for the next corpus (or frees a fallback allocation)
    void adopt(size_t bytes);  // takes the best-fitting parked mapping of the same (device, role), if there is one
    void unmap_and_retire();   // gives the physical memory back; the virtual range stays reserved, never mapped again
    static bool evict_parked(int device);   // all parked mappings of a device; true if anything was freed
    static void evict_all_parked();
    static uint64_t parked_bytes();         // device memory behind every parked mapping (the health call's figure)
};

// parked mappings, per (device, role), until a corpus adopts them, memory runs short or the plugin shuts down
inline std::mutex g_park_mu;
inline std::map<std::pair<int, int>, std::vector<GrowBuf>> g_parked;

inline void GrowBuf::release() {
    if (plain) { (void)hipSetDevice(device); if (base) (void)hipFree(base); }
    else if (base) {
        std::lock_guard<std::mutex> lk(g_park_mu);
        g_parked[{device, role}].push_back(*this);
    }
    base = nullptr; reserved = mapped = 0; plain = false; chunk_end.clear();
}
inline void GrowBuf::adopt(size_t bytes) {
    if (base) return;
    std::lock_guard<std::mutex> lk(g_park_mu);
    auto& v = g_parked[{device, role}];
    if (v.empty()) return;
    // best fit: the smallest parked mapping that holds the request — but not one more than 4x larger (a small
    // corpus must not pin the mirror of a destroyed 100 GB one; that one waits for a corpus of its size).
    // Nothing large enough: the largest one that is not larger than needed, it grows in place.
    size_t best = v.size();
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i].mapped >= bytes && v[i].mapped / 4 <= std::max<size_t>(bytes, 64ull << 20) && (best == v.size() || v[i].mapped < v[best].mapped)) best = i;
    if (best == v.size())
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i].mapped < bytes && v[i].reserved >= bytes && (best == v.size() || v[i].mapped > v[best].mapped)) best = i;
    if (best == v.size()) return;
    base = v[best].base; reserved = v[best].reserved; mapped = v[best].mapped; chunk_end = std::move(v[best].chunk_end);
    v.erase(v.begin() + static_cast<std::ptrdiff_t>(best));
}
inline void GrowBuf::unmap_and_retire() {
    if (plain || !base) return;
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize(); // nothing may still read through these translations
    size_t off = 0;
    for (size_t end : chunk_end) { if (hipMemUnmap(base + off, end - off) != hipSuccess) (void)hipGetLastError(); off = end; }
    // the range itself is NOT freed: a later reservation could land on it, and a mapping at an address that
    // was mapped before is read through stale translations on this driver (scripts/ubench/vmm_stale.hip)
    base = nullptr; reserved = mapped = 0; chunk_end.clear();
}
inline bool GrowBuf::evict_parked(int device) {
    std::vector<GrowBuf> victims;
    {
        std::lock_guard<std::mutex> lk(g_park_mu);
        for (auto& kv : g_parked)
            if (kv.first.first == device) { for (auto& b : kv.second) victims.push_back(std::move(b)); kv.second.clear(); }
    }
    size_t freed = 0;
    for (auto& b : victims) { freed += b.mapped; b.unmap_and_retire(); }
    return freed != 0;
}
inline void GrowBuf::evict_all_parked() {
    std::vector<int> devs;
    {
        std::lock_guard<std::mutex> lk(g_park_mu);
        for (auto& kv : g_parked) if (!kv.second.empty()) devs.push_back(kv.first.first);
    }
    for (int d : devs) (void)evict_parked(d);
}
inline uint64_t GrowBuf::parked_bytes() {
    std::lock_guard<std::mutex> lk(g_park_mu);
    uint64_t bytes = 0;
    for (auto& kv : g_parked) for (auto& b : kv.second) bytes += b.mapped;
    return bytes;
}

} // namespace door
} // namespace yams_accel
