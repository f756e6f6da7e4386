// plugin.cpp — the YAMS plugin surface of libyams_mi355x_accel.so.
//
// Exports the eight entry points of the reference's include/yams/plugins/abi.h:26-34 and serves
// fifteen interface vtables (vector_scan_v1, vector_doc_scan_v1, vector_entity_scan_v1, topology_cluster_v1,
// semantic_graph_v1, topology_smooth_v1, topology_artifacts_v1, topology_route_v1, topology_quality_v1, topology_features_v1, late_interaction_rerank_v1, embedding_pool_v1, content_hash_v1, content_checksum_v1, chunker_v1) written to the
// conventions of include/yams/plugins/model_provider_v1.h:44-49.  The host side that would load
// this file is AbiPluginLoader::load / getInterface (src/daemon/resource/abi_plugin_loader.cpp:
// 270-442, 657-681): dlopen(RTLD_LAZY|RTLD_LOCAL), yams_plugin_init(config_json, host_context),
// yams_plugin_get_manifest_json, then yams_plugin_get_interface(id, version, &vtable).
// What the door computes on the host alone (configuration, row / mask / rank dealing, hit packing, hex) is plugin_host.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include "accel_ctx.h"
#include "plugin_host.h"

// The eight entry points and their return codes are declared in include/yams_mi355x_accel.h exactly as
// the reference's include/yams/plugins/abi.h:18-34 declares them (no local restatement here).

namespace {
using namespace yams_accel::plugin_host;

// No exception may cross the C ABI (model_provider_v1.h:44-49; the reference's own plugins wrap every entry point,
// plugins/onnx/model_provider.cpp:51,94,105): every function pointer of the three vtables is the guarded form of
// its implementation — std::bad_alloc from an absurd batch size, or anything else thrown below, becomes
// YAMS_ERR_INTERNAL (void functions just return).
template <auto Fn> struct Guard;
template <typename R, typename... A, R (*Fn)(A...)> struct Guard<Fn> {
    static R call(A... a) noexcept {
        try { return Fn(a...); }
        catch (...) { if constexpr (!std::is_void_v<R>) return static_cast<R>(YAMS_ERR_INTERNAL); }
    }
};
#define GUARDED(fn) (&Guard<&fn>::call)

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
};

// parked mappings, per (device, role), until a corpus adopts them, memory runs short or the plugin shuts down
std::mutex g_park_mu;
std::map<std::pair<int, int>, std::vector<GrowBuf>> g_parked;

void GrowBuf::release() {
    if (plain) { (void)hipSetDevice(device); if (base) (void)hipFree(base); }
    else if (base) {
        std::lock_guard<std::mutex> lk(g_park_mu);
        g_parked[{device, role}].push_back(*this);
    }
    base = nullptr; reserved = mapped = 0; plain = false; chunk_end.clear();
}
void GrowBuf::adopt(size_t bytes) {
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
void GrowBuf::unmap_and_retire() {
    if (plain || !base) return;
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize(); // nothing may still read through these translations
    size_t off = 0;
    for (size_t end : chunk_end) { if (hipMemUnmap(base + off, end - off) != hipSuccess) (void)hipGetLastError(); off = end; }
    // the range itself is NOT freed: a later reservation could land on it, and a mapping at an address that
    // was mapped before is read through stale translations on this driver (scripts/ubench/vmm_stale.hip)
    base = nullptr; reserved = mapped = 0; chunk_end.clear();
}
bool GrowBuf::evict_parked(int device) {
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
void GrowBuf::evict_all_parked() {
    std::vector<int> devs;
    {
        std::lock_guard<std::mutex> lk(g_park_mu);
        for (auto& kv : g_parked) if (!kv.second.empty()) devs.push_back(kv.first.first);
    }
    for (int d : devs) (void)evict_parked(d);
}

// One shard of a corpus: the rows dealt to one device, plus their filter shadows.
struct ShardStore {
    int device = 0;
    uint64_t n_rows = 0;
    GrowBuf rows, bf16, nsq, i8, i8meta, tie, inv;
    bool has_tie = false;
    void release() { rows.release(); bf16.release(); nsq.release(); i8.release(); i8meta.release(); tie.release(); inv.release(); n_rows = 0; has_tie = false; }
    // virtual range per array if freshly reserved: a fixed share of the device's memory per role
    static size_t share(size_t dev_total, int role) {
        switch (role) {
            case 0: return dev_total;            // rows (fp32)
            case 1: return dev_total / 2;        // bf16 shadow
            case 2: return dev_total / 4;        // int8 shadow
            case 3: return dev_total / 16;       // squared norms
            case 4: return dev_total / 256;      // int8 block scales
            default: return dev_total / 16;      // tie ranks, inverse, corpus-wide ranking
        }
    }
};

// A ya_malloc'd device array with ONE owner (move-only): freed on its device when the owner goes or takes another.
template <typename T> struct DevArray {
    int device = 0;
    T* p = nullptr;
    DevArray() = default;
    DevArray(DevArray&& o) noexcept : device(o.device), p(o.p) { o.p = nullptr; }
    DevArray& operator=(DevArray&& o) noexcept { std::swap(device, o.device); std::swap(p, o.p); return *this; }
    ~DevArray() { if (p) { (void)hipSetDevice(device); (void)hipFree(p); } }
    bool alloc(int dev, size_t bytes) {          // (on an empty owner; the caller has made `dev` current)
        device = dev;
        return yams_accel::ya_malloc(reinterpret_cast<void**>(&p), bytes) == hipSuccess;
    }
    operator T*() const { return p; }
};

// The host's product-quantiser index of a corpus (SimeonPqIndexState, sqlite_vec_backend.cpp:48-62), on the corpus's device:
// codes, the rank of every code's tie-break key, and the mirror row behind every key index.
struct PqIndex {
    DevArray<uint8_t> codes; DevArray<uint32_t> tie_rank, key_row;
    uint64_t n = 0; uint32_t m = 0;
    void release() { *this = PqIndex(); }
};

// The row -> document map of a corpus (vector_doc_scan_v1.corpus_set_documents), on the corpus's device.
struct DocMap {
    std::vector<uint32_t> row_doc;   // host copy: rows appended after the map was set are NO_DOC (padded per search)
    DevArray<uint32_t> d_row_doc, d_doc_rank;
    uint64_t n_rows = 0; uint32_t n_docs = 0;
    void release() { *this = DocMap(); }
};

// The attribute columns of an entity corpus (vector_entity_scan_v1.corpus_set_attributes), on the corpus's device.  The host
// copies cover the rows set so far; rows appended later carry the "unset" values (padded per search).
struct EntityCols {
    std::vector<uint8_t> type; std::vector<uint32_t> node, doc;
    DevArray<uint8_t> d_type; DevArray<uint32_t> d_node, d_doc;
    uint64_t n_rows = 0;
    void release() { *this = EntityCols(); }
};

struct Corpus {
    uint32_t dim = 0;
    uint64_t n_rows = 0;
    int i8_flags = -1;               // layout of the int8 shadow (YAMS_SCAN_I8_*), decided at the first append; -1: not yet
    uint64_t i8_decided_rows = 0;    // rows the "auto" decision looked at (one taken from fewer than 4096 rows is taken again once they are there)
    PqIndex pq;                      // (version 2 of the vtable: pq_index_set / search_pq)
    DocMap docs;                     // (vector_doc_scan_v1)
    EntityCols ents;                 // (vector_entity_scan_v1)
    std::vector<ShardStore> sh;      // one per plugin device
    GrowBuf rank_of_row;             // device 0: the corpus-wide chunk_id ranking (cross-shard ties)
    bool has_ranks = false;
    std::shared_mutex mu;            // searches share, mutations exclude (vector_database.cpp:539,618)
};

// rows of a stripe when a corpus is dealt to several devices (config "stripe_rows", a multiple of 64;
// fixed at init: it is part of every corpus's row -> shard map)
uint32_t kStripeRows = 65536;

// A pool of N identical resources handed out to concurrent calls.
template <typename T> class Pool {
public:
    void add(T v) { std::lock_guard<std::mutex> lk(mu_); free_.push_back(v); all_.push_back(v); }
    T acquire() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !free_.empty(); });
        T v = free_.back(); free_.pop_back();
        return v;
    }
    void release(T v) { { std::lock_guard<std::mutex> lk(mu_); free_.push_back(v); } cv_.notify_one(); }
    std::vector<T> drain() { std::lock_guard<std::mutex> lk(mu_); auto a = all_; all_.clear(); free_.clear(); return a; }
    size_t size() const { return all_.size(); }
private:
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<T> free_, all_;
};
template <typename T> struct Lease {
    Pool<T>& pool; T v;
    explicit Lease(Pool<T>& p) : pool(p), v(p.acquire()) {}
    ~Lease() { pool.release(v); }
};

struct PluginState {
    std::shared_mutex mu;            // init / shutdown exclude everything else; calls share
    bool initialised = false;
    std::vector<int> devices;        // config "devices": [..] (or "device": n); rows are striped over them
    bool want_bf16 = true, want_i8 = true;
    int i8_layout = 0;               // configuration "i8_layout": 0 auto (measured at a corpus' first append), 1 plain, 2 rotated
    std::string init_error;
    // searches: ONE sharded handle over the plugin's devices (one RCCL communicator when there are several),
    // "search_slots" lanes = concurrent searches in flight, each on its own contexts / streams / worker threads;
    // the lanes of one device share a sweep gate inside the handle (sharded_api.cpp)
    yams_scan_sharded* sharded = nullptr;
    uint32_t search_slots = 0;
    uint32_t l2_acc = YAMS_SCAN_FLAG_L2_ACC_F64;   // config "l2_accumulate": "f64" | "f32" | "f32x8" | "f32x16"
    // the last corpus_append: bytes, ms spent mapping device memory / copying / building shadows (written under upload_mu,
    // read by the health call without it: atomics), and the slowest append so far with its split
    std::atomic<uint64_t> append_bytes{0}, appends{0};
    std::atomic<double> append_map_ms{0}, append_copy_ms{0}, append_shadow_ms{0};
    std::atomic<double> slow_append_ms{0}, slow_map_ms{0}, slow_copy_ms{0}, slow_shadow_ms{0};
    std::atomic<uint64_t> slow_append_bytes{0}, exhausted_appends{0};
    Pool<yams_accel_ctx*> work_ctx;          // hashing / chunking contexts on devices[0]
    std::vector<yams_accel_ctx*> upload_ctx; // one per device, used under a corpus's exclusive lock
    std::mutex upload_mu;                    // (upload contexts are shared by all corpora)
    std::mutex corpora_mu;
    std::map<uint64_t, std::shared_ptr<Corpus>> corpora;
    uint64_t next_id = 1;
    std::atomic<uint64_t> searches{0}, hashes{0}, chunk_calls{0}, refused_chains{0}, deferred_chains{0};
};
PluginState& g = *new PluginState;   // never destroyed: when a host exits without yams_plugin_shutdown, the corpora's DevArrays must
                                     // not reach hipFree from a static destructor (the runtime may have gone before them)

const char kManifest[] =
    "{\"name\":\"yams_mi355x_accel\",\"version\":\"" YAMS_ACCEL_VERSION_STRING "\",\"abi\":1,"
    "\"description\":\"MI355X (gfx950) exact vector scan, SHA-256 and content-defined chunking\","
    "\"interfaces\":[{\"id\":\"vector_scan_v1\",\"version\":1},"
    "{\"id\":\"content_hash_v1\",\"version\":1},{\"id\":\"chunker_v1\",\"version\":3}]}";

std::shared_ptr<Corpus> find_corpus(uint64_t id) {
    std::lock_guard<std::mutex> lk(g.corpora_mu);
    auto it = g.corpora.find(id);
    return it == g.corpora.end() ? nullptr : it->second;
}

#define NEED_INIT() std::shared_lock<std::shared_mutex> init_lk__(g.mu); do { if (!g.initialised) return YAMS_ERR_UNSUPPORTED; } while (0)

// Which filter shadows a corpus of this dimension has: vs_corpus_append builds exactly these and view_of hands out exactly
// these (a view naming a shadow that was never built would have the int8 tier's proof accept wrong rows in silence).
inline bool has_bf16(uint32_t dim) { return g.want_bf16 && (dim & 3u) == 0; }
inline bool has_i8(uint32_t dim) { return g.want_i8 && (dim & 63u) == 0 && dim >= 256; }

// Shard i of a corpus as its engine sees it: rows, n_rows and dim, and of the rest what the search asks for.
enum : unsigned { kViewTies = 1, kViewShadows = 2, kViewStripes = 4 };
yams_scan_corpus_t view_of(const Corpus& c, uint32_t i, unsigned what) {
    const ShardStore& s = c.sh[i];
    yams_scan_corpus_t v;
    std::memset(&v, 0, sizeof v);
    v.rows = s.rows.as<float>(); v.n_rows = s.n_rows; v.dim = c.dim;
    if ((what & kViewTies) && s.has_tie) { v.tie_rank = s.tie.as<uint32_t>(); v.rank_row = s.inv.as<uint32_t>(); }
    if ((what & kViewShadows) && has_bf16(c.dim) && s.n_rows) { v.rows_bf16 = s.bf16.as<uint16_t>(); v.rows_nsq = s.nsq.as<float>(); }
    if ((what & kViewShadows) && has_i8(c.dim) && s.n_rows) { v.rows_i8 = s.i8.as<int8_t>(); v.rows_i8_meta = s.i8meta.as<float>(); v.i8_flags = c.i8_flags > 0 ? static_cast<uint32_t>(c.i8_flags) : 0u; }
    if ((what & kViewStripes) && c.sh.size() > 1) { v.stripe_rows = kStripeRows; v.n_stripes = static_cast<uint32_t>(c.sh.size()); v.stripe_index = i; }
    return v;
}

// The malloc'd result of a search: hits[nq * max(k, 1)], every row preset to -1, and counts[max(nq, 1)], zeroed.  commit()
// hands both to the caller (who frees them through the vtable's free function); what was not committed goes with the object.
struct HitResult {
    const size_t slots;
    uint32_t* counts;
    yams_scan_hit_t* hits;
    HitResult(uint32_t nq, uint32_t k)
        : slots(static_cast<size_t>(nq) * std::max<uint32_t>(k, 1)),
          counts(static_cast<uint32_t*>(std::calloc(std::max<uint32_t>(nq, 1), sizeof(uint32_t)))),
          hits(static_cast<yams_scan_hit_t*>(std::calloc(std::max<size_t>(slots, 1), sizeof(yams_scan_hit_t)))) {
        for (size_t o = 0; hits && o < slots; ++o) hits[o].row = -1;
    }
    HitResult(const HitResult&) = delete;
    ~HitResult() { std::free(counts); std::free(hits); }
    bool ok() const { return counts && hits; }
    yams_status_t commit(yams_scan_hit_t** out_hits, uint32_t** out_counts) {
        *out_hits = hits; *out_counts = counts;
        hits = nullptr; counts = nullptr;
        return YAMS_OK;
    }
};

// The host's allow-mask (document_hash / candidate_hashes restriction, :4137-4175; tombstones), dealt like the rows: shard i's
// part goes into workspace `name` of the context (its device is current) and into the shard's view.
yams_status_t attach_row_mask(yams_accel_ctx* x, const char* name, const uint32_t* row_mask_host, uint32_t n_sh, uint32_t i,
                              yams_scan_corpus_t& v) {
    const DealtMask m = deal_row_mask(row_mask_host, v.n_rows, kStripeRows, n_sh, i);
    uint32_t* d_mask = nullptr;
    YA_TRY(yams_accel::ws_get(x, name, m.words.size() * 4, (void**)&d_mask));
    if (yams_accel_upload(x, d_mask, m.words.data(), m.words.size() * 4) != YAMS_OK) return YAMS_ERR_INTERNAL;
    v.row_mask = d_mask; v.row_mask_count = m.bits;
    return YAMS_OK;
}

// ---- vector_scan_v1 ---------------------------------------------------------------------------
yams_status_t vs_corpus_create(void*, uint32_t dim, uint64_t* out_id) {
    NEED_INIT();
    if (!out_id || dim == 0) return YAMS_ERR_INVALID_ARG;
    auto c = std::make_shared<Corpus>();
    c->dim = dim;
    c->sh.resize(g.devices.size());
    for (size_t i = 0; i < g.devices.size(); ++i) {
        auto& s = c->sh[i];
        s.device = g.devices[i];
        int role = 0;
        for (GrowBuf* b : {&s.rows, &s.bf16, &s.i8, &s.nsq, &s.i8meta, &s.tie, &s.inv}) { b->device = s.device; b->role = role++; }
    }
    c->rank_of_row.device = g.devices[0]; c->rank_of_row.role = 7; // (parked mappings are adopted at the first ensure(), best fit)
    std::lock_guard<std::mutex> lk(g.corpora_mu);
    *out_id = g.next_id++;
    g.corpora[*out_id] = c;
    return YAMS_OK;
}

// Appends rows: they take the next global ids, are dealt to the devices in stripes, copied to the end of
// each shard's growing mirror, and the shadows of the touched local ranges are (re)built.
// measure builds say where an internal error came from
// device memory behind a mirror could not be had (out of memory, or beyond the mirror's share of the address space):
// the corpus is left exactly as it was — same rows, same shadows, searches go on — and the caller can act on it
// (ErrorCode::ResourceExhausted, include/yams/core/types.h:49 of the reference)
inline yams_status_t exhausted(const char* where) {
#ifdef YAMS_ACCEL_MEASURE
    std::fprintf(stderr, "[yams_mi355x_accel] device memory exhausted at %s\n", where);
#else
    (void)where;
#endif
    return YAMS_ERR_RESOURCE_EXHAUSTED;
}
inline yams_status_t internal_error(const char* where) {
#ifdef YAMS_ACCEL_MEASURE
    std::fprintf(stderr, "[yams_mi355x_accel] internal error at %s (hip: %s)\n", where, hipGetErrorString(hipGetLastError()));
#else
    (void)where;
#endif
    return YAMS_ERR_INTERNAL;
}

yams_status_t vs_corpus_append(void*, uint64_t id, const float* rows, uint64_t n_rows) {
    NEED_INIT();
    auto c = find_corpus(id);
    if (!c) return YAMS_ERR_NOT_FOUND;
    if (n_rows == 0) return YAMS_OK;
    if (!rows) return YAMS_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> lk(c->mu);
    std::lock_guard<std::mutex> up(g.upload_mu);
    const uint32_t n_sh = static_cast<uint32_t>(c->sh.size());
    const uint64_t n0 = c->n_rows, n1 = n0 + n_rows;
    if (shard_rows(n1, kStripeRows, n_sh, 0) >= (1ull << 32)) return YAMS_ERR_UNSUPPORTED;
    const size_t rb = static_cast<size_t>(c->dim) * 4;
    const bool bf16 = has_bf16(c->dim), i8 = has_i8(c->dim);
    size_t dev_total = 0, dev_free = 0;
    const auto t_begin = std::chrono::steady_clock::now();
    for (uint32_t i = 0; i < n_sh; ++i) {
        ShardStore& s = c->sh[i];
        const uint64_t old = s.n_rows, now = shard_rows(n1, kStripeRows, n_sh, i);
        if (now == old) continue;
        (void)hipSetDevice(s.device);
        if (hipMemGetInfo(&dev_free, &dev_total) != hipSuccess || dev_total == 0) {
            (void)hipGetLastError();
            dev_total = 288ull << 30; // the reservation is address space only: size it for the part this library is written for
        }
        if (!s.rows.ensure(now * rb, ShardStore::share(dev_total, 0))) { ++g.exhausted_appends; return exhausted("append:1"); }
        if (bf16 && (!s.bf16.ensure(now * rb / 2, ShardStore::share(dev_total, 1)) || !s.nsq.ensure(now * 4, ShardStore::share(dev_total, 3)))) { ++g.exhausted_appends; return exhausted("append:2"); }
        if (i8 && (!s.i8.ensure((now + 63) / 64 * 64 * rb / 4 /* whole 64-row blocks: the shadow is stored blocked */, ShardStore::share(dev_total, 2)) || !s.i8meta.ensure(((now + 63) / 64) * 8, ShardStore::share(dev_total, 4)))) { ++g.exhausted_appends; return exhausted("append:3"); }
    }
    const auto t_mapped = std::chrono::steady_clock::now();
    // copy: runs of consecutive global rows inside one stripe are consecutive local rows
    for (uint64_t r = n0; r < n1;) {
        const uint64_t run = std::min<uint64_t>(n1 - r, n_sh == 1 ? n1 - r : kStripeRows - r % kStripeRows);
        ShardStore& s = c->sh[shard_of(r, kStripeRows, n_sh)];
        yams_accel_ctx* uc = g.upload_ctx[shard_of(r, kStripeRows, n_sh)];
        (void)hipSetDevice(s.device);
        if (!s.rows.h2d(local_of(r, kStripeRows, n_sh) * rb, rows + (r - n0) * c->dim, run * rb, uc->stream)) return internal_error("append:4");
        r += run;
    }
    for (uint32_t i = 0; i < n_sh; ++i) if (yams_accel_ctx_synchronize(g.upload_ctx[i]) != YAMS_OK) return internal_error("append:4b");
    const auto t_copied = std::chrono::steady_clock::now();
    bool relayout = false;          // the shadow is rebuilt from row 0 (the measured layout changed once enough rows were there)
    if (i8 && (c->i8_flags < 0 || (g.i8_layout == 0 && c->i8_decided_rows < 4096 && n1 >= 4096))) {
        // the layout of this corpus' int8 shadow: the configured one, or whichever quantises the rows better — measured at the
        // first append and, if that one brought fewer than 4096 rows (a host that inserts a few vectors, then searches), once
        // more when 4096 are there
        const int before = c->i8_flags;
        c->i8_flags = 0;
        c->i8_decided_rows = n1;
        if (g.i8_layout == 2) {
            if (c->dim <= 4096) c->i8_flags = static_cast<int>(YAMS_SCAN_I8_ROTATED);   // (the rotated layout exists for 256 <= dim <= 4096)
        } else if (g.i8_layout == 0) {
            for (uint32_t i = 0; i < n_sh; ++i) {
                const uint64_t now = shard_rows(n1, kStripeRows, n_sh, i);
                if (!now) continue;
                uint32_t fl = 0;
                (void)hipSetDevice(c->sh[i].device);
                if (yams_scan_choose_i8_layout_device(g.upload_ctx[i], c->sh[i].rows.as<float>(), now, c->dim, &fl, nullptr, nullptr) != YAMS_OK)
                    return internal_error("append:4c");
                c->i8_flags = static_cast<int>(fl);
                break;
            }
        }
        relayout = before >= 0 && before != c->i8_flags;
    }
    for (uint32_t i = 0; i < n_sh; ++i) {
        ShardStore& s = c->sh[i];
        const uint64_t old = s.n_rows, now = shard_rows(n1, kStripeRows, n_sh, i);
        yams_accel_ctx* uc = g.upload_ctx[i];
        if (relayout && i8 && now) {     // every block of this shard again, in the layout the rows turned out to want
            if (yams_scan_build_shadow_i8_layout_device(uc, s.rows.as<float>(), 0, old, c->dim, static_cast<uint32_t>(c->i8_flags),
                                                        s.i8.as<int8_t>(), s.i8meta.as<float>(), nullptr) != YAMS_OK)
                return internal_error("append:6b");
        }
        if (now != old) {
            if (bf16 && yams_scan_build_shadow_device(uc, s.rows.as<float>() + old * c->dim, now - old, c->dim,
                                                      s.bf16.as<uint16_t>() + old * c->dim, s.nsq.as<float>() + old) != YAMS_OK)
                return internal_error("append:5");
            if (i8 && yams_scan_build_shadow_i8_layout_device(uc, s.rows.as<float>(), old, now - old, c->dim, static_cast<uint32_t>(c->i8_flags),
                                                              s.i8.as<int8_t>(), s.i8meta.as<float>(), nullptr) != YAMS_OK)
                return internal_error("append:6");
        }
        if (yams_accel_ctx_synchronize(uc) != YAMS_OK) return internal_error("append:7");
        s.n_rows = now;
        s.has_tie = false; // appended rows invalidate a previously supplied chunk_id ranking
    }
    c->n_rows = n1;
    c->has_ranks = false;
    {   // where the call's time went (health JSON, "last_append"): fresh device memory behind the mirrors, the copy, the shadows
        const auto t_end = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        g.append_bytes = n_rows * rb; g.append_map_ms = ms(t_begin, t_mapped); g.append_copy_ms = ms(t_mapped, t_copied); g.append_shadow_ms = ms(t_copied, t_end);
        ++g.appends;
        if (ms(t_begin, t_end) > g.slow_append_ms.load()) {   // an outlier among many appends says where its time went
            g.slow_append_ms = ms(t_begin, t_end); g.slow_map_ms = ms(t_begin, t_mapped); g.slow_copy_ms = ms(t_mapped, t_copied);
            g.slow_shadow_ms = ms(t_copied, t_end); g.slow_append_bytes = n_rows * rb;
        }
    }
    return YAMS_OK;
}

yams_status_t vs_corpus_set_tie_ranks(void*, uint64_t id, const uint32_t* ranks, uint64_t n_rows) {
    NEED_INIT();
    auto c = find_corpus(id);
    if (!c) return YAMS_ERR_NOT_FOUND;
    std::unique_lock<std::shared_mutex> lk(c->mu);
    if (n_rows != c->n_rows || (!ranks && n_rows)) return YAMS_ERR_INVALID_ARG;
    if (!is_permutation_of_iota(ranks, n_rows)) return YAMS_ERR_INVALID_ARG;
    if (n_rows == 0) return YAMS_OK;
    std::lock_guard<std::mutex> up(g.upload_mu);
    const uint32_t n_sh = static_cast<uint32_t>(c->sh.size());
    for (uint32_t i = 0; i < n_sh; ++i) {
        ShardStore& s = c->sh[i];
        const uint64_t nl = s.n_rows;
        if (nl == 0) continue;
        std::vector<uint32_t> lrank, linv;
        local_tie_ranks(ranks, nl, kStripeRows, n_sh, i, lrank, linv);
        if (!s.tie.ensure(nl * 4, s.rows.reserved / 16) || !s.inv.ensure(nl * 4, s.rows.reserved / 16)) return YAMS_ERR_RESOURCE_EXHAUSTED;
        (void)hipSetDevice(s.device);
        if (!s.tie.h2d(0, lrank.data(), nl * 4, g.upload_ctx[i]->stream) || !s.inv.h2d(0, linv.data(), nl * 4, g.upload_ctx[i]->stream) ||
            yams_accel_ctx_synchronize(g.upload_ctx[i]) != YAMS_OK) return YAMS_ERR_INTERNAL;
        s.has_tie = true;
    }
    if (n_sh > 1) {
        (void)hipSetDevice(c->rank_of_row.device);
        if (!c->rank_of_row.ensure(n_rows * 4, c->sh[0].rows.reserved / 16) ||
            !c->rank_of_row.h2d(0, ranks, n_rows * 4, g.upload_ctx[0]->stream) ||
            yams_accel_ctx_synchronize(g.upload_ctx[0]) != YAMS_OK) return YAMS_ERR_INTERNAL;
    }
    c->has_ranks = true;
    return YAMS_OK;
}

void release_corpus(Corpus& c) {
    c.pq.release();
    c.docs.release();
    c.ents.release();
    for (auto& s : c.sh) s.release();
    c.rank_of_row.release();
    c.n_rows = 0; c.has_ranks = false; c.i8_flags = -1; c.i8_decided_rows = 0;
}

// The rows are gone, the mirror's memory stays mapped for the re-upload that usually follows (compaction).
yams_status_t vs_corpus_clear(void*, uint64_t id) {
    NEED_INIT();
    auto c = find_corpus(id);
    if (!c) return YAMS_ERR_NOT_FOUND;
    std::unique_lock<std::shared_mutex> lk(c->mu);
    for (auto& s : c->sh) { s.n_rows = 0; s.has_tie = false; }
    c->pq.release();        // (its index -> row table names rows that are gone: nothing is searched until pq_index_set comes again)
    c->docs.release();
    c->ents.release();
    c->n_rows = 0; c->has_ranks = false; c->i8_flags = -1; c->i8_decided_rows = 0;
    return YAMS_OK;
}

yams_status_t vs_corpus_destroy(void*, uint64_t id) {
    NEED_INIT();
    std::shared_ptr<Corpus> c;
    {
        std::lock_guard<std::mutex> lk(g.corpora_mu);
        auto it = g.corpora.find(id);
        if (it == g.corpora.end()) return YAMS_ERR_NOT_FOUND;
        c = it->second;
        g.corpora.erase(it);
    }
    std::unique_lock<std::shared_mutex> lk(c->mu);
    release_corpus(*c);
    return YAMS_OK;
}

yams_status_t vs_corpus_size(void*, uint64_t id, uint64_t* out_rows, uint32_t* out_dim) {
    NEED_INIT();
    auto c = find_corpus(id);
    if (!c) return YAMS_ERR_NOT_FOUND;
    std::shared_lock<std::shared_mutex> lk(c->mu);
    if (out_rows) *out_rows = c->n_rows;
    if (out_dim) *out_dim = c->dim;
    return YAMS_OK;
}

yams_status_t vs_search_batch_ex(void*, uint64_t id, const float* queries, uint32_t nq, uint32_t dim,
                                 uint32_t k, float threshold, uint32_t metric, uint32_t flags,
                                 const uint32_t* row_mask_host, yams_scan_hit_t** out_hits,
                                 uint32_t** out_counts, yams_scan_diag_t* out_diag) {
    NEED_INIT();
    if (!out_hits || !out_counts) return YAMS_ERR_INVALID_ARG;
    *out_hits = nullptr; *out_counts = nullptr;
    auto c = find_corpus(id);
    if (!c) return YAMS_ERR_NOT_FOUND;
    // dimension mismatch -> InvalidArgument (vector_database.cpp:545-550, 626-633)
    if (dim != c->dim) return YAMS_ERR_INVALID_ARG;
    if (nq && !queries) return YAMS_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> lk(c->mu);      // concurrent searches share the corpus
    struct LaneLease {                                  // ... and each runs on its own lane of the sharded handle
        uint32_t lane = 0; bool held = false;
        ~LaneLease() { if (held) yams_scan_sharded_lane_release(g.sharded, lane); }
    } slot;
    if (yams_scan_sharded_lane_acquire(g.sharded, 1, &slot.lane) != YAMS_OK) return YAMS_ERR_INTERNAL;
    slot.held = true;
    const uint32_t n_sh = static_cast<uint32_t>(c->sh.size());
    std::vector<yams_scan_corpus_t> views(n_sh);
    for (uint32_t i = 0; i < n_sh; ++i) {
        views[i] = view_of(*c, i, kViewTies | kViewShadows | kViewStripes);
        if (row_mask_host && views[i].n_rows) {
            (void)hipSetDevice(c->sh[i].device);
            YA_TRY(attach_row_mask(yams_scan_sharded_lane_ctx(g.sharded, i, slot.lane), "plugin_row_mask", row_mask_host, n_sh, i, views[i]));
        }
    }
    // only semantic flags cross the vtable; filter selection stays with the library
    yams_scan_params_t prm{k, threshold, metric, flags & (YAMS_SCAN_FLAG_RECORD_PATH | YAMS_SCAN_FLAG_FORCE_EXACT | YAMS_SCAN_FLAG_DEFER_THRESHOLD |
                                                          YAMS_SCAN_FLAG_L2_ACC_MASK | YAMS_SCAN_FLAG_L2_ACC_FUSED)};
    // vec0's distance arithmetic: the call's own choice (any L2_ACC bit, or L2_ACC_EXPLICIT for a deliberate F64), else
    // the plugin's ("l2_accumulate" in the init config)
    if (metric == YAMS_SCAN_L2 && !(flags & (YAMS_SCAN_FLAG_L2_ACC_MASK | YAMS_SCAN_FLAG_L2_ACC_EXPLICIT))) prm.flags |= g.l2_acc;
    HitResult res(nq, k);
    if (!res.ok()) return YAMS_ERR_INTERNAL;
    std::vector<float> scores(res.slots), dist(res.slots);
    std::vector<int64_t> rows(res.slots);
    yams_status_t s = yams_scan_sharded_submit(g.sharded, slot.lane, views.data(), queries, nq, &prm,
                                               c->has_ranks && n_sh > 1 ? c->rank_of_row.as<uint32_t>() : nullptr, 0,
                                               out_diag ? YAMS_SHARDED_SUBMIT_DIAG : 0u);
    if (s == YAMS_OK) {
        slot.held = false; // wait() frees the lane
        s = yams_scan_sharded_wait(g.sharded, slot.lane, scores.data(), rows.data(), res.counts, dist.data(), out_diag);
    }
    if (s != YAMS_OK) return s;
    pack_hits(nq, k, res.counts, rows.data(), scores.data(), dist.data(), res.hits);
    ++g.searches;
    return res.commit(out_hits, out_counts);
}

yams_status_t vs_search_batch_masked(void* self, uint64_t id, const float* queries, uint32_t nq, uint32_t dim,
                                     uint32_t k, float threshold, uint32_t metric,
                                     const uint32_t* row_mask_host, yams_scan_hit_t** out_hits,
                                     uint32_t** out_counts, yams_scan_diag_t* out_diag) {
    return vs_search_batch_ex(self, id, queries, nq, dim, k, threshold, metric, 0, row_mask_host, out_hits,
                              out_counts, out_diag);
}

yams_status_t vs_search_batch(void* self, uint64_t id, const float* queries, uint32_t nq, uint32_t dim,
                              uint32_t k, float threshold, uint32_t metric,
                              yams_scan_hit_t** out_hits, uint32_t** out_counts,
                              yams_scan_diag_t* out_diag) {
    return vs_search_batch_masked(self, id, queries, nq, dim, k, threshold, metric, nullptr, out_hits,
                                  out_counts, out_diag);
}

// ---- one scaffold for the three single-device engines (PQ, documents, entities) ---------------------------------------------
// It owns the checks of a call (in this order: out-pointers, k, corpus, dimension, null inputs), the corpus's shared lock,
// the refusal of a striped corpus, the result, the lease of a work context, the workspace "plugin_<engine>_*" for queries,
// scores, rows, counts (and the matching-row counts), the query upload, the view with its allow-mask, the downloads and the
// packing.  An engine gives: when there is nothing to find (beyond nq == 0), `reserve` for workspace of its own (taken
// right after the queries'), and `run` for its side tables' uploads and its device call.
struct SearchCall {
    uint64_t id; const float* queries; bool inputs_given; uint32_t nq, dim, k; const uint32_t* row_mask_host;
    yams_scan_hit_t** out_hits; uint32_t** out_counts; uint64_t* out_matching; yams_scan_diag_t* out_diag;
};
struct SearchSlots {
    yams_accel_ctx* x; const yams_scan_corpus_t* view;
    float* d_q; float* d_s; int64_t* d_r; uint32_t* d_n; uint64_t* d_m;
};
template <typename Empty, typename Reserve, typename Run>
yams_status_t search_one_device(const SearchCall& a, const char* engine, unsigned view_what, bool matching, Empty&& nothing_to_find,
                                Reserve&& reserve, Run&& run) {
    NEED_INIT();
    if (!a.out_hits || !a.out_counts) return YAMS_ERR_INVALID_ARG;
    *a.out_hits = nullptr; *a.out_counts = nullptr;
    if (a.k > YAMS_SCAN_MAX_K) return YAMS_ERR_UNSUPPORTED;
    auto c = find_corpus(a.id);
    if (!c) return YAMS_ERR_NOT_FOUND;
    if (a.dim != c->dim) return YAMS_ERR_INVALID_ARG;           // (vector_database.cpp:545-550; entities: a row of another size lives in another corpus, :2858)
    if (a.nq && !a.inputs_given) return YAMS_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> lk(c->mu);
    if (c->sh.size() != 1) return YAMS_ERR_UNSUPPORTED;
    HitResult res(a.nq, a.k);
    if (!res.ok()) return YAMS_ERR_INTERNAL;
    if (a.nq == 0 || nothing_to_find(*c)) { if (a.out_diag) std::memset(a.out_diag, 0, sizeof *a.out_diag); return res.commit(a.out_hits, a.out_counts); }
    (void)hipSetDevice(c->sh[0].device);
    Lease<yams_accel_ctx*> w(g.work_ctx);
    SearchSlots d{};
    d.x = w.v;
    const auto ws = [engine](const char* what) { return std::string("plugin_").append(engine).append("_").append(what); };
    const size_t nq = a.nq;
    YA_TRY(yams_accel::ws_get(d.x, ws("queries").c_str(), nq * a.dim * 4, (void**)&d.d_q));
    YA_TRY(reserve(*c, d.x));
    YA_TRY(yams_accel::ws_get(d.x, ws("scores").c_str(), res.slots * 4, (void**)&d.d_s));
    YA_TRY(yams_accel::ws_get(d.x, ws("rows").c_str(), res.slots * 8, (void**)&d.d_r));
    YA_TRY(yams_accel::ws_get(d.x, ws("counts").c_str(), nq * 4, (void**)&d.d_n));
    if (matching) YA_TRY(yams_accel::ws_get(d.x, ws("matching").c_str(), nq * 8, (void**)&d.d_m));
    if (yams_accel_upload(d.x, d.d_q, a.queries, nq * a.dim * 4) != YAMS_OK) return YAMS_ERR_INTERNAL;
    yams_scan_corpus_t v = view_of(*c, 0, view_what);
    if (a.row_mask_host && v.n_rows) YA_TRY(attach_row_mask(d.x, ws("mask").c_str(), a.row_mask_host, 1, 0, v));
    d.view = &v;
    YA_TRY(run(*c, d));
    std::vector<float> scores(res.slots); std::vector<int64_t> rows(res.slots);
    if (yams_accel_download(d.x, res.counts, d.d_n, nq * 4) != YAMS_OK ||
        (a.k && yams_accel_download(d.x, scores.data(), d.d_s, res.slots * 4) != YAMS_OK) ||
        (a.k && yams_accel_download(d.x, rows.data(), d.d_r, res.slots * 8) != YAMS_OK) ||
        (a.out_matching && yams_accel_download(d.x, a.out_matching, d.d_m, nq * 8) != YAMS_OK)) return YAMS_ERR_INTERNAL;
    pack_hits(a.nq, a.k, res.counts, rows.data(), scores.data(), nullptr, res.hits);
    ++g.searches;
    return res.commit(a.out_hits, a.out_counts);
}
const auto reserve_nothing = [](const Corpus&, yams_accel_ctx*) { return YAMS_OK; };

// ---- version 2: the product-quantised engine over the mirror (yams_scan_pq_topk_device) ------------------------------------
yams_status_t vs_pq_index_set(void*, uint64_t id, const uint8_t* codes, uint64_t n_codes, uint32_t m, const uint64_t* tie_keys,
                              const uint32_t* row_of_index) {
    NEED_INIT();
    auto c = find_corpus(id);
    if (!c) return YAMS_ERR_NOT_FOUND;
    std::unique_lock<std::shared_mutex> lk(c->mu);
    if (c->sh.size() != 1) return YAMS_ERR_UNSUPPORTED;      // (a PQ index over a striped corpus: not built)
    c->pq.release();
    if (n_codes == 0) return YAMS_OK;
    if (!codes || m == 0 || m > 128 || n_codes >= (1ull << 32)) return YAMS_ERR_INVALID_ARG;
    std::vector<uint32_t> rank, key_row;      // once per index build, on the host
    rank_pq_keys(tie_keys, row_of_index, n_codes, rank, key_row);
    PqIndex p; p.n = n_codes; p.m = m;        // (goes with this scope, its arrays with it, unless it becomes the corpus's)
    const int dev = c->sh[0].device;
    (void)hipSetDevice(dev);
    Lease<yams_accel_ctx*> w(g.work_ctx);
    const size_t code_bytes = (static_cast<size_t>(n_codes) * m + 15) & ~static_cast<size_t>(15);
    if (!(p.codes.alloc(dev, code_bytes) && p.tie_rank.alloc(dev, n_codes * 4) && p.key_row.alloc(dev, n_codes * 4))) { (void)hipGetLastError(); return YAMS_ERR_RESOURCE_EXHAUSTED; }
    if (yams_accel_upload(w.v, p.codes, codes, static_cast<size_t>(n_codes) * m) != YAMS_OK ||
        yams_accel_upload(w.v, p.tie_rank, rank.data(), n_codes * 4) != YAMS_OK ||
        yams_accel_upload(w.v, p.key_row, key_row.data(), n_codes * 4) != YAMS_OK) return YAMS_ERR_INTERNAL;
    c->pq = std::move(p);
    return YAMS_OK;
}

yams_status_t vs_search_pq(void*, uint64_t id, const float* queries, const float* luts, uint32_t nq, uint32_t dim, uint32_t k,
                           float threshold, uint32_t rerank_factor, uint32_t flags, const uint32_t* candidates, uint64_t n_candidates,
                           yams_scan_hit_t** out_hits, uint32_t** out_counts, yams_scan_diag_t* out_diag) {
    if (candidates == nullptr) n_candidates = 0;
    float* d_l = nullptr; uint32_t* d_c = nullptr;
    const SearchCall a{id, queries, queries && luts, nq, dim, k, nullptr, out_hits, out_counts, nullptr, out_diag};
    return search_one_device(a, "pq", kViewTies, false,
        // no index (or an empty one), no rows, k == 0, an empty candidate list: nothing (:3873-3880, :3946-3948)
        [&](const Corpus& c) { return k == 0 || c.pq.n == 0 || c.sh[0].n_rows == 0 || (candidates && n_candidates == 0); },
        [&](const Corpus& c, yams_accel_ctx* x) -> yams_status_t {
            YA_TRY(yams_accel::ws_get(x, "plugin_pq_luts", static_cast<size_t>(nq) * c.pq.m * 1024, (void**)&d_l));
            if (candidates) YA_TRY(yams_accel::ws_get(x, "plugin_pq_candidates", n_candidates * 4, (void**)&d_c));
            return YAMS_OK;
        },
        [&](const Corpus& c, const SearchSlots& d) -> yams_status_t {
            const PqIndex& p = c.pq;
            if (yams_accel_upload(d.x, d_l, luts, static_cast<size_t>(nq) * p.m * 1024) != YAMS_OK ||
                (candidates && yams_accel_upload(d.x, d_c, candidates, n_candidates * 4) != YAMS_OK)) return YAMS_ERR_INTERNAL;
            yams_scan_pq_index_t pi{p.codes, p.n, p.m, 0, p.tie_rank, p.key_row};
            yams_scan_pq_params_t prm{k, threshold, rerank_factor, flags & YAMS_PQ_SUM_ORDER_MASK};
            return yams_scan_pq_topk_device(d.x, d.view, &pi, d.d_q, d_l, nq, &prm, d_c, n_candidates, d.d_s, d.d_r, d.d_n, out_diag);
        });
}

void vs_free_hits(void*, yams_scan_hit_t* hits, uint32_t* counts) { std::free(hits); std::free(counts); }

yams_status_t vs_runtime_info(void*, char** out_json) {
    NEED_INIT();
    Lease<yams_accel_ctx*> w(g.work_ctx);
    return yams_accel_device_info_json(w.v, out_json);
}
void vs_free_string(void*, char* s) { std::free(s); }

yams_vector_scan_v1 g_vector_scan = {
    YAMS_IFACE_VECTOR_SCAN_V1_VERSION, nullptr, GUARDED(vs_corpus_create), GUARDED(vs_corpus_append),
    GUARDED(vs_corpus_set_tie_ranks), GUARDED(vs_corpus_clear), GUARDED(vs_corpus_destroy), GUARDED(vs_corpus_size),
    GUARDED(vs_search_batch), GUARDED(vs_free_hits), GUARDED(vs_runtime_info), GUARDED(vs_free_string),
    GUARDED(vs_search_batch_masked), GUARDED(vs_search_batch_ex), GUARDED(vs_pq_index_set), GUARDED(vs_search_pq)};

// ---- vector_doc_scan_v1: document-level selection over a vector_scan_v1 corpus (yams_scan_doc_topk_device) -----------------
yams_status_t ds_corpus_set_documents(void*, uint64_t id, const uint32_t* row_doc, uint64_t n_rows, const uint32_t* doc_rank,
                                      uint32_t n_docs) {
    NEED_INIT();
    auto c = find_corpus(id);
    if (!c) return YAMS_ERR_NOT_FOUND;
    std::unique_lock<std::shared_mutex> lk(c->mu);
    if (c->sh.size() != 1) return YAMS_ERR_UNSUPPORTED;      // (a document map over a striped corpus: not built)
    if (n_rows != c->n_rows || (n_rows && !row_doc) || n_docs == YAMS_SCAN_NO_DOC) return YAMS_ERR_INVALID_ARG;
    for (uint64_t r = 0; r < n_rows; ++r)
        if (row_doc[r] != YAMS_SCAN_NO_DOC && row_doc[r] >= n_docs) return YAMS_ERR_INVALID_ARG;
    if (doc_rank && !is_permutation_of_iota(doc_rank, n_docs)) return YAMS_ERR_INVALID_ARG;
    c->docs.release();
    DocMap m; m.n_rows = n_rows; m.n_docs = n_docs;      // (goes with this scope unless it becomes the corpus's)
    m.row_doc.assign(row_doc, row_doc + n_rows);
    const int dev = c->sh[0].device;
    (void)hipSetDevice(dev);
    if (!((n_rows == 0 || m.d_row_doc.alloc(dev, n_rows * 4)) && (!doc_rank || n_docs == 0 || m.d_doc_rank.alloc(dev, static_cast<size_t>(n_docs) * 4)))) { (void)hipGetLastError(); return YAMS_ERR_RESOURCE_EXHAUSTED; }
    Lease<yams_accel_ctx*> w(g.work_ctx);
    if ((m.d_row_doc && yams_accel_upload(w.v, m.d_row_doc, row_doc, n_rows * 4) != YAMS_OK) ||
        (m.d_doc_rank && yams_accel_upload(w.v, m.d_doc_rank, doc_rank, static_cast<size_t>(n_docs) * 4) != YAMS_OK)) return YAMS_ERR_INTERNAL;
    c->docs = std::move(m);
    return YAMS_OK;
}

yams_status_t ds_search_docs(void*, uint64_t id, const float* queries, uint32_t nq, uint32_t dim, uint32_t k, float threshold,
                             const uint32_t* row_mask_host, yams_scan_hit_t** out_hits, uint32_t** out_counts,
                             uint64_t* out_matching, yams_scan_diag_t* out_diag) {
    const SearchCall a{id, queries, queries != nullptr, nq, dim, k, row_mask_host, out_hits, out_counts, out_matching, out_diag};
    return search_one_device(a, "doc", kViewTies, true, [](const Corpus&) { return false; }, reserve_nothing,
        [&](const Corpus& c, const SearchSlots& d) -> yams_status_t {
            // the document map; rows appended after it was set have no document
            const DocMap& dm = c.docs;
            yams_scan_docs_t docs{dm.d_row_doc, dm.d_doc_rank, dm.n_docs, 0};
            if (d.view->n_rows > dm.n_rows) {
                std::vector<uint32_t> padded(d.view->n_rows, YAMS_SCAN_NO_DOC);
                std::copy(dm.row_doc.begin(), dm.row_doc.end(), padded.begin());
                uint32_t* d_pad;
                YA_TRY(yams_accel::ws_get(d.x, "plugin_doc_row_doc", padded.size() * 4, (void**)&d_pad));
                if (yams_accel_upload(d.x, d_pad, padded.data(), padded.size() * 4) != YAMS_OK) return YAMS_ERR_INTERNAL;
                docs.row_doc = d_pad;
            }
            yams_scan_params_t prm{k, threshold, YAMS_SCAN_COSINE, 0};
            return yams_scan_doc_topk_device(d.x, d.view, &docs, d.d_q, nq, &prm, d.d_s, d.d_r, nullptr, d.d_n, d.d_m, out_diag);
        });
}

void ds_free_doc_hits(void*, yams_scan_hit_t* hits, uint32_t* counts) { std::free(hits); std::free(counts); }

yams_vector_doc_scan_v1 g_vector_doc_scan = {YAMS_IFACE_VECTOR_DOC_SCAN_V1_VERSION, nullptr, GUARDED(ds_corpus_set_documents),
                                             GUARDED(ds_search_docs), GUARDED(ds_free_doc_hits)};

// ---- vector_entity_scan_v1: IEntityStore::searchEntities over a vector_scan_v1 corpus (yams_scan_entity_topk_device) ---------
yams_status_t es_corpus_set_attributes(void*, uint64_t id, uint64_t first_row, uint64_t n_rows, const uint8_t* types,
                                       const uint32_t* node_types, const uint32_t* docs) {
    NEED_INIT();
    auto c = find_corpus(id);
    if (!c) return YAMS_ERR_NOT_FOUND;
    std::unique_lock<std::shared_mutex> lk(c->mu);
    if (c->sh.size() != 1) return YAMS_ERR_UNSUPPORTED;      // (attribute columns over a striped corpus: not built)
    if (first_row > c->n_rows || n_rows > c->n_rows - first_row) return YAMS_ERR_INVALID_ARG;
    EntityCols& e = c->ents;
    // rows never set carry the "unset" values
    e.type.resize(c->n_rows, YAMS_SCAN_ENTITY_TYPE_UNSET);
    e.node.resize(c->n_rows, YAMS_SCAN_ENTITY_UNSET);
    e.doc.resize(c->n_rows, YAMS_SCAN_ENTITY_UNSET);
    if (types) std::copy(types, types + n_rows, e.type.begin() + first_row);
    if (node_types) std::copy(node_types, node_types + n_rows, e.node.begin() + first_row);
    if (docs) std::copy(docs, docs + n_rows, e.doc.begin() + first_row);
    e.d_type = {}; e.d_node = {}; e.d_doc = {};               // (the old columns go first: the new ones may need their memory)
    e.n_rows = 0;
    if (c->n_rows == 0) return YAMS_OK;
    const int dev = c->sh[0].device;
    (void)hipSetDevice(dev);
    const size_t n = c->n_rows;
    DevArray<uint8_t> t; DevArray<uint32_t> nd, dc;            // (go with this scope unless they become the corpus's; the host copies
                                                               //  stay either way: the next search pads from them)
    if (!(t.alloc(dev, n) && nd.alloc(dev, n * 4) && dc.alloc(dev, n * 4))) { (void)hipGetLastError(); return YAMS_ERR_RESOURCE_EXHAUSTED; }
    Lease<yams_accel_ctx*> w(g.work_ctx);
    if (yams_accel_upload(w.v, t, e.type.data(), n) != YAMS_OK || yams_accel_upload(w.v, nd, e.node.data(), n * 4) != YAMS_OK ||
        yams_accel_upload(w.v, dc, e.doc.data(), n * 4) != YAMS_OK) return YAMS_ERR_INTERNAL;
    e.d_type = std::move(t); e.d_node = std::move(nd); e.d_doc = std::move(dc);
    e.n_rows = n;
    return YAMS_OK;
}

yams_status_t es_search_entities(void*, uint64_t id, const float* queries, const yams_scan_entity_filter_t* filters, uint32_t nq,
                                 uint32_t dim, uint32_t k, float threshold, const uint32_t* row_mask_host, yams_scan_hit_t** out_hits,
                                 uint32_t** out_counts, uint64_t* out_matching, yams_scan_diag_t* out_diag) {
    const SearchCall a{id, queries, queries != nullptr, nq, dim, k, row_mask_host, out_hits, out_counts, out_matching, out_diag};
    return search_one_device(a, "ent", 0, true, [](const Corpus&) { return false; }, reserve_nothing,
        [&](const Corpus& c, const SearchSlots& d) -> yams_status_t {
            // the attribute columns; rows appended after they were last set carry the "unset" values
            const EntityCols& e = c.ents;
            yams_scan_entities_t cols{e.d_type, e.d_node, e.d_doc};
            if (d.view->n_rows > e.n_rows) {
                const size_t n = d.view->n_rows;
                std::vector<uint8_t> t(n, YAMS_SCAN_ENTITY_TYPE_UNSET); std::vector<uint32_t> nd(n, YAMS_SCAN_ENTITY_UNSET), dc(n, YAMS_SCAN_ENTITY_UNSET);
                std::copy(e.type.begin(), e.type.end(), t.begin()); std::copy(e.node.begin(), e.node.end(), nd.begin());
                std::copy(e.doc.begin(), e.doc.end(), dc.begin());
                uint8_t* p;
                const size_t off = (n + 15) & ~static_cast<size_t>(15);
                YA_TRY(yams_accel::ws_get(d.x, "plugin_ent_cols", off + n * 8, (void**)&p));
                if (yams_accel_upload(d.x, p, t.data(), n) != YAMS_OK || yams_accel_upload(d.x, p + off, nd.data(), n * 4) != YAMS_OK ||
                    yams_accel_upload(d.x, p + off + n * 4, dc.data(), n * 4) != YAMS_OK) return YAMS_ERR_INTERNAL;
                cols = yams_scan_entities_t{p, reinterpret_cast<uint32_t*>(p + off), reinterpret_cast<uint32_t*>(p + off + n * 4)};
            }
            return yams_scan_entity_topk_device(d.x, d.view, &cols, d.d_q, filters, nq, k, threshold, d.d_s, d.d_r, d.d_n, d.d_m, out_diag);
        });
}

void es_free_entity_hits(void*, yams_scan_hit_t* hits, uint32_t* counts) { std::free(hits); std::free(counts); }

yams_vector_entity_scan_v1 g_vector_entity_scan = {YAMS_IFACE_VECTOR_ENTITY_SCAN_V1_VERSION, nullptr, GUARDED(es_corpus_set_attributes),
                                                   GUARDED(es_search_entities), GUARDED(es_free_entity_hits)};

// ---- topology_cluster_v1: the topology build's k-means over host memory (yams_cluster_kmeans_host / _assign_device) --------
yams_status_t tc_kmeans(void*, const float* rows, uint64_t n, uint32_t dim, uint32_t k, uint32_t max_iterations,
                        uint32_t** out_membership, float** out_centroids, uint32_t* out_k, uint32_t* out_iterations) {
    NEED_INIT();
    if (!out_membership) return YAMS_ERR_INVALID_ARG;
    *out_membership = nullptr;
    if (out_centroids) *out_centroids = nullptr;
    if (out_k) *out_k = 0;
    if (out_iterations) *out_iterations = 0;
    if (n == 0) return YAMS_OK;
    if (dim == 0 || !rows || n < 2) return YAMS_ERR_INVALID_ARG;
    if (n >= (1ull << 31) || dim > YAMS_CLUSTER_MAX_DIM) return YAMS_ERR_UNSUPPORTED;
    // the clamped k bounds the centroid array (:367-371)
    uint64_t kk = k ? k : static_cast<uint64_t>(std::round(std::sqrt(static_cast<double>(n))));
    kk = std::min<uint64_t>(std::max<uint64_t>(kk, 2), n);
    if (kk > YAMS_CLUSTER_MAX_K) return YAMS_ERR_UNSUPPORTED;
    auto* mem = static_cast<uint32_t*>(std::malloc(static_cast<size_t>(n) * 4));
    auto* cent = out_centroids ? static_cast<float*>(std::malloc(static_cast<size_t>(kk) * dim * 4)) : nullptr;
    if (!mem || (out_centroids && !cent)) { std::free(mem); std::free(cent); return YAMS_ERR_RESOURCE_EXHAUSTED; }
    Lease<yams_accel_ctx*> w(g.work_ctx);
    const yams_status_t st = yams_cluster_kmeans_host(w.v, rows, n, dim, k, max_iterations, mem, cent, out_k, out_iterations);
    if (st != YAMS_OK) { std::free(mem); std::free(cent); return st; }
    *out_membership = mem;
    if (out_centroids) *out_centroids = cent;
    return YAMS_OK;
}

yams_status_t tc_assign(void*, const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t n_centroids,
                        const uint8_t* centroid_empty, uint32_t** out_assign, double** out_distance) {
    NEED_INIT();
    if (!out_assign) return YAMS_ERR_INVALID_ARG;
    *out_assign = nullptr;
    if (out_distance) *out_distance = nullptr;
    if (n == 0) return YAMS_OK;
    if (dim == 0 || !rows || (n_centroids && !centroids)) return YAMS_ERR_INVALID_ARG;
    if (n >= (1ull << 31) || dim > YAMS_CLUSTER_MAX_DIM || n_centroids > YAMS_CLUSTER_MAX_K) return YAMS_ERR_UNSUPPORTED;
    auto* asg = static_cast<uint32_t*>(std::malloc(static_cast<size_t>(n) * 4));
    auto* dist = out_distance ? static_cast<double*>(std::malloc(static_cast<size_t>(n) * 8)) : nullptr;
    if (!asg || (out_distance && !dist)) { std::free(asg); std::free(dist); return YAMS_ERR_RESOURCE_EXHAUSTED; }
    auto done = [&](yams_status_t st) { if (st != YAMS_OK) { std::free(asg); std::free(dist); } else { *out_assign = asg; if (out_distance) *out_distance = dist; } return st; };
    Lease<yams_accel_ctx*> w(g.work_ctx);
    yams_accel_ctx* x = w.v;
    const size_t rb = static_cast<size_t>(n) * dim * 4, cb = static_cast<size_t>(n_centroids) * dim * 4;
    float* d_rows; float* d_cent; uint8_t* d_empty = nullptr; uint32_t* d_asg; double* d_dist = nullptr;
    yams_status_t st;
    if ((st = yams_accel::ws_get(x, "plugin_tc_rows", rb, (void**)&d_rows)) != YAMS_OK) return done(st);
    if ((st = yams_accel::ws_get(x, "plugin_tc_centroids", cb + 16, (void**)&d_cent)) != YAMS_OK) return done(st);
    if ((st = yams_accel::ws_get(x, "plugin_tc_assign", static_cast<size_t>(n) * 4, (void**)&d_asg)) != YAMS_OK) return done(st);
    if (out_distance && (st = yams_accel::ws_get(x, "plugin_tc_distance", static_cast<size_t>(n) * 8, (void**)&d_dist)) != YAMS_OK) return done(st);
    if (centroid_empty && n_centroids) {
        if ((st = yams_accel::ws_get(x, "plugin_tc_empty", n_centroids, (void**)&d_empty)) != YAMS_OK) return done(st);
        if (yams_accel_upload(x, d_empty, centroid_empty, n_centroids) != YAMS_OK) return done(YAMS_ERR_INTERNAL);
    }
    if (yams_accel_upload(x, d_rows, rows, rb) != YAMS_OK || (cb && yams_accel_upload(x, d_cent, centroids, cb) != YAMS_OK)) return done(YAMS_ERR_INTERNAL);
    if ((st = yams_cluster_assign_device(x, d_rows, n, dim, d_cent, n_centroids, d_empty, d_asg, d_dist)) != YAMS_OK) return done(st);
    if (yams_accel_download(x, asg, d_asg, static_cast<size_t>(n) * 4) != YAMS_OK ||
        (dist && yams_accel_download(x, dist, d_dist, static_cast<size_t>(n) * 8) != YAMS_OK)) return done(YAMS_ERR_INTERNAL);
    return done(YAMS_OK);
}

void tc_free_clusters(void*, uint32_t* membership, float* centroids) { std::free(membership); std::free(centroids); }
void tc_free_assignment(void*, uint32_t* assign, double* distance) { std::free(assign); std::free(distance); }

yams_topology_cluster_v1 g_topology_cluster = {YAMS_IFACE_TOPOLOGY_CLUSTER_V1_VERSION, nullptr, GUARDED(tc_kmeans), GUARDED(tc_assign),
                                               GUARDED(tc_free_clusters), GUARDED(tc_free_assignment)};

// ---- semantic_graph_v1: the semantic-neighbour graph over host memory (yams_graph_semantic_neighbors_host) ------------------
yams_status_t sg_neighbors(void*, const float* rows, uint64_t n, uint32_t dim, const uint32_t* tie_rank, const uint32_t* source_rows,
                           uint64_t n_sources, uint32_t k, uint32_t flags, float threshold, uint32_t** out_rows, float** out_sims,
                           uint32_t** out_counts, float** out_inv_norm, yams_graph_diag_t* out_diag) {
    NEED_INIT();
    if (!out_rows || !out_sims || !out_counts) return YAMS_ERR_INVALID_ARG;
    *out_rows = nullptr; *out_sims = nullptr; *out_counts = nullptr;
    if (out_inv_norm) *out_inv_norm = nullptr;
    if (out_diag) std::memset(out_diag, 0, sizeof *out_diag);
    const uint64_t S = source_rows ? n_sources : n;
    // the limits bound the arrays allocated here; every other check is the flat entry's
    if (n >= (1ull << 31) || S >= (1ull << 31) || dim > YAMS_GRAPH_MAX_DIM || k > YAMS_GRAPH_MAX_K) return YAMS_ERR_UNSUPPORTED;
    Lease<yams_accel_ctx*> w(g.work_ctx);
    if (k == 0 || n < 2 || S == 0)      // an empty result: null arrays (the flat entry still judges flags and threshold)
        return yams_graph_semantic_neighbors_host(w.v, rows, n, dim, tie_rank, source_rows, n_sources, k, flags, threshold, nullptr, nullptr,
                                                  nullptr, nullptr, out_diag);
    const size_t slots = static_cast<size_t>(S) * k;
    auto* r = static_cast<uint32_t*>(std::malloc(slots * 4));
    auto* s = static_cast<float*>(std::malloc(slots * 4));
    auto* c = static_cast<uint32_t*>(std::malloc(static_cast<size_t>(S) * 4));
    auto* iv = out_inv_norm ? static_cast<float*>(std::malloc(static_cast<size_t>(n) * 4)) : nullptr;
    auto drop = [&] { std::free(r); std::free(s); std::free(c); std::free(iv); };
    if (!r || !s || !c || (out_inv_norm && !iv)) { drop(); return YAMS_ERR_RESOURCE_EXHAUSTED; }
    const yams_status_t st = yams_graph_semantic_neighbors_host(w.v, rows, n, dim, tie_rank, source_rows, n_sources, k, flags, threshold, r, s, c,
                                                                iv, out_diag);
    if (st != YAMS_OK) { drop(); return st; }
    *out_rows = r; *out_sims = s; *out_counts = c;
    if (out_inv_norm) *out_inv_norm = iv;
    return YAMS_OK;
}

void sg_free_neighbors(void*, uint32_t* rows, float* sims, uint32_t* counts, float* inv_norm) {
    std::free(rows); std::free(sims); std::free(counts); std::free(inv_norm);
}

yams_semantic_graph_v1 g_semantic_graph = {YAMS_IFACE_SEMANTIC_GRAPH_V1_VERSION, nullptr, GUARDED(sg_neighbors), GUARDED(sg_free_neighbors)};

// ---- topology_smooth_v1: SGC smoothing over host memory (yams_graph_sgc_smooth_host) -----------------------------------------
yams_status_t ts_smooth(void*, const float* rows, uint64_t n, uint32_t dim, const uint64_t* row_offsets, const uint32_t* cols,
                        const float* weights, uint32_t hops, float* out, yams_sgc_diag_t* out_diag) {
    NEED_INIT();
    if (out_diag) std::memset(out_diag, 0, sizeof *out_diag);
    Lease<yams_accel_ctx*> w(g.work_ctx);      // every check is the flat entry's: the caller owns every array
    return yams_graph_sgc_smooth_host(w.v, rows, n, dim, row_offsets, cols, weights, hops, out, out_diag);
}

yams_topology_smooth_v1 g_topology_smooth = {YAMS_IFACE_TOPOLOGY_SMOOTH_V1_VERSION, nullptr, GUARDED(ts_smooth)};

// ---- topology_artifacts_v1: centroids, representatives, residuals over host memory (yams_cluster_*_host) -------------------
// the limits bound the arrays allocated here; every other check is the flat entries'
yams_status_t ta_centroids(void*, const float* rows, uint64_t n, uint32_t dim, const uint64_t* cluster_offsets, const uint32_t* members,
                           uint32_t n_clusters, float** out_centroids, uint32_t** out_counts) {
    NEED_INIT();
    if (!out_centroids || !out_counts) return YAMS_ERR_INVALID_ARG;
    *out_centroids = nullptr; *out_counts = nullptr;
    if (n >= (1ull << 31) || dim > YAMS_CLUSTER_MAX_DIM || n_clusters > YAMS_CLUSTER_MAX_K) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0) return YAMS_ERR_INVALID_ARG;
    if (n_clusters == 0) return YAMS_OK;
    auto* cent = static_cast<float*>(std::malloc(static_cast<size_t>(n_clusters) * dim * 4));
    auto* cnt = static_cast<uint32_t*>(std::malloc(static_cast<size_t>(n_clusters) * 4));
    if (!cent || !cnt) { std::free(cent); std::free(cnt); return YAMS_ERR_RESOURCE_EXHAUSTED; }
    Lease<yams_accel_ctx*> w(g.work_ctx);
    const yams_status_t st = yams_cluster_centroids_host(w.v, rows, n, dim, cluster_offsets, members, n_clusters, cent, cnt);
    if (st != YAMS_OK) { std::free(cent); std::free(cnt); return st; }
    *out_centroids = cent; *out_counts = cnt;
    return YAMS_OK;
}

yams_status_t ta_representatives(void*, const float* rows, uint64_t n, uint32_t dim, const uint64_t* cluster_offsets,
                                 const uint32_t* candidates, const float* centroids, const uint8_t* centroid_empty, uint32_t n_clusters,
                                 uint32_t n_extra, uint32_t** out_selected, uint32_t** out_counts) {
    NEED_INIT();
    if (!out_selected || !out_counts) return YAMS_ERR_INVALID_ARG;
    *out_selected = nullptr; *out_counts = nullptr;
    if (n >= (1ull << 31) || dim > YAMS_CLUSTER_MAX_DIM || n_clusters > YAMS_CLUSTER_MAX_K || n_extra > YAMS_CLUSTER_MAX_REPRESENTATIVES)
        return YAMS_ERR_UNSUPPORTED;
    if (dim == 0) return YAMS_ERR_INVALID_ARG;
    if (n_clusters == 0) return YAMS_OK;
    auto* sel = n_extra ? static_cast<uint32_t*>(std::malloc(static_cast<size_t>(n_clusters) * n_extra * 4)) : nullptr;
    auto* cnt = static_cast<uint32_t*>(std::malloc(static_cast<size_t>(n_clusters) * 4));
    if ((n_extra && !sel) || !cnt) { std::free(sel); std::free(cnt); return YAMS_ERR_RESOURCE_EXHAUSTED; }
    Lease<yams_accel_ctx*> w(g.work_ctx);
    const yams_status_t st = yams_cluster_representatives_host(w.v, rows, n, dim, cluster_offsets, candidates, centroids, centroid_empty,
                                                               n_clusters, n_extra, sel, cnt);
    if (st != YAMS_OK) { std::free(sel); std::free(cnt); return st; }
    *out_selected = sel; *out_counts = cnt;
    return YAMS_OK;
}

yams_status_t ta_residuals(void*, const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t n_clusters,
                           const uint32_t* primary, const uint64_t* cand_offsets, const uint32_t* cand, uint32_t form,
                           double** out_primary_norm_sq, double** out_cand_norm_sq, double** out_residual_dot) {
    NEED_INIT();
    if (!out_cand_norm_sq || (primary && (!out_primary_norm_sq || !out_residual_dot))) return YAMS_ERR_INVALID_ARG;
    *out_cand_norm_sq = nullptr;
    if (out_primary_norm_sq) *out_primary_norm_sq = nullptr;
    if (out_residual_dot) *out_residual_dot = nullptr;
    if (n >= (1ull << 31) || dim > YAMS_CLUSTER_MAX_DIM || n_clusters > YAMS_CLUSTER_MAX_K) return YAMS_ERR_UNSUPPORTED;
    if (dim == 0 || (cand_offsets == nullptr) != (cand == nullptr)) return YAMS_ERR_INVALID_ARG;
    if (n == 0) return YAMS_OK;
    if (cand_offsets)      // the offsets size the arrays: judged here first
        for (uint64_t i = 0; i < n; ++i)
            if (cand_offsets[0] != 0 || cand_offsets[i + 1] < cand_offsets[i]) return YAMS_ERR_INVALID_ARG;
    const uint64_t pairs = cand_offsets ? cand_offsets[n] : n * n_clusters;
    const size_t p1 = static_cast<size_t>(pairs ? pairs : 1);
    auto* cn = static_cast<double*>(std::malloc(p1 * 8));
    auto* pn = primary ? static_cast<double*>(std::malloc(static_cast<size_t>(n) * 8)) : nullptr;
    auto* rd = primary ? static_cast<double*>(std::malloc(p1 * 8)) : nullptr;
    auto drop = [&] { std::free(cn); std::free(pn); std::free(rd); };
    if (!cn || (primary && (!pn || !rd))) { drop(); return YAMS_ERR_RESOURCE_EXHAUSTED; }
    Lease<yams_accel_ctx*> w(g.work_ctx);
    const yams_status_t st = yams_cluster_residuals_host(w.v, rows, n, dim, centroids, n_clusters, primary, cand_offsets, cand, form, pn, cn, rd);
    if (st != YAMS_OK) { drop(); return st; }
    *out_cand_norm_sq = cn;
    if (primary) { *out_primary_norm_sq = pn; *out_residual_dot = rd; }
    return YAMS_OK;
}

void ta_free_centroids(void*, float* centroids, uint32_t* counts) { std::free(centroids); std::free(counts); }
void ta_free_representatives(void*, uint32_t* selected, uint32_t* counts) { std::free(selected); std::free(counts); }
void ta_free_residuals(void*, double* primary_norm_sq, double* cand_norm_sq, double* residual_dot) {
    std::free(primary_norm_sq); std::free(cand_norm_sq); std::free(residual_dot);
}

yams_topology_artifacts_v1 g_topology_artifacts = {YAMS_IFACE_TOPOLOGY_ARTIFACTS_V1_VERSION, nullptr, GUARDED(ta_centroids),
                                                   GUARDED(ta_representatives), GUARDED(ta_residuals), GUARDED(ta_free_centroids),
                                                   GUARDED(ta_free_representatives), GUARDED(ta_free_residuals)};

// ---- content_hash_v1 --------------------------------------------------------------------------
// Every call leases one of the plugin's work contexts (own stream, own workspace), so hashing, chunking
// and searches of different host threads overlap on the device instead of queueing on one mutex.
// One SHA-256 chain is sequential: ~35 MB/s on a device lane, > 1 GB/s on a host core.  Work the device is worse
// at is refused (YAMS_ERR_UNSUPPORTED: the host hashes it itself), not served slowly — see the header.
yams_status_t ch_hash(void*, const uint8_t* data, size_t n, char out_hex[65]) {
    NEED_INIT();
    if (n > YAMS_HASH_LONE_CHAIN_MAX) { ++g.refused_chains; return YAMS_ERR_UNSUPPORTED; }
    Lease<yams_accel_ctx*> w(g.work_ctx);
    ++g.hashes;
    return yams_sha256_host(w.v, data, n, out_hex);
}
yams_status_t ch_hash_many(void*, const uint8_t* const* msgs, const size_t* lens, size_t n, char* out_hex) {
    NEED_INIT();
    if (n && lens && !chains_suit_the_device(lens, n)) { ++g.refused_chains; return YAMS_ERR_UNSUPPORTED; }
    Lease<yams_accel_ctx*> w(g.work_ctx);
    g.hashes += n;
    return yams_sha256_many_host(w.v, msgs, lens, n, out_hex);
}

// Streaming state (sha256_hasher.cpp:81-109).  update() only BUFFERS on the host: one SHA-256 chain is
// sequential, a launch + sync per update would cost more than the hashing.  Whole 64-byte blocks are
// pushed through the device in pieces of kStreamFlush bytes (one upload + one kernel each), the tail
// and the FIPS 180-4 padding at finalize().  A handle is a single-threaded object, like the reference's
// hasher (sha256_hasher.cpp:34).
struct HashStream {
    uint32_t state[8];
    std::vector<uint8_t> pending; // bytes not yet compressed
    uint64_t total = 0;           // bytes compressed so far + pending
};
constexpr size_t kStreamFlush = 64u << 20;
const uint32_t kShaInit[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                              0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
}  // namespace

namespace yams_accel { // from ingest_kernels.hip
hipError_t launch_sha256(hipStream_t st, const uint8_t* data, const uint64_t* offs,
                         const uint64_t* lens, uint64_t n_long, uint64_t n_msgs, uint8_t* digests,
                         unsigned long long* queue_heads, const uint32_t* init_state,
                         uint32_t* out_state, int raw_blocks_only, uint32_t max_blocks, int slots);
}

namespace {
// Runs the compression function over `n` bytes (a multiple of 64) starting from hs->state.
yams_status_t stream_blocks(yams_accel_ctx* ctx, HashStream* hs, const uint8_t* bytes, size_t n) {
    using namespace yams_accel;
    if (n == 0) return YAMS_OK;
    (void)hipSetDevice(ctx->device);
    uint8_t* d_data; uint64_t* d_tab; uint32_t* d_state; unsigned long long* d_head;
    YA_TRY(ws_get(ctx, "hs_data", n + 64, (void**)&d_data));
    YA_TRY(ws_get(ctx, "hs_tab", 64, (void**)&d_tab));
    YA_TRY(ws_get(ctx, "hs_state", 64, (void**)&d_state));
    YA_TRY(ws_get(ctx, "ing_queue", 64, (void**)&d_head));
    const uint64_t tab[2] = {0, n};
    uint32_t out[8];
    YA_HIP(ctx, hipMemcpyAsync(d_data, bytes, n, hipMemcpyHostToDevice, ctx->stream));
    YA_HIP(ctx, hipMemcpyAsync(d_tab, tab, 16, hipMemcpyHostToDevice, ctx->stream));
    YA_HIP(ctx, hipMemcpyAsync(d_state, hs->state, 32, hipMemcpyHostToDevice, ctx->stream));
    YA_HIP(ctx, launch_sha256(ctx->stream, d_data, d_tab, d_tab + 1, 0, 1, nullptr, d_head, d_state,
                              d_state + 8, 1, 1, 1));
    YA_HIP(ctx, hipMemcpyAsync(out, d_state + 8, 32, hipMemcpyDeviceToHost, ctx->stream));
    YA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(hs->state, out, 32); // the handle changes only after the device call succeeded
    return YAMS_OK;
}
yams_status_t flush_whole_blocks(HashStream* hs) {
    const size_t whole = hs->pending.size() / 64 * 64;
    if (whole == 0) return YAMS_OK;
    Lease<yams_accel_ctx*> w(g.work_ctx);
    YA_TRY(stream_blocks(w.v, hs, hs->pending.data(), whole));
    hs->pending.erase(hs->pending.begin(), hs->pending.begin() + static_cast<std::ptrdiff_t>(whole));
    return YAMS_OK;
}

yams_status_t ch_stream_create(void*, void** out) {
    NEED_INIT();
    if (!out) return YAMS_ERR_INVALID_ARG;
    auto* hs = new HashStream();
    std::memcpy(hs->state, kShaInit, 32);
    *out = hs;
    return YAMS_OK;
}
yams_status_t ch_stream_init(void*, void* s) {
    NEED_INIT();
    if (!s) return YAMS_ERR_INVALID_ARG;
    auto* hs = static_cast<HashStream*>(s);
    std::memcpy(hs->state, kShaInit, 32);
    hs->pending.clear(); hs->total = 0;
    return YAMS_OK;
}
yams_status_t ch_stream_update(void*, void* s, const uint8_t* data, size_t n) {
    NEED_INIT();
    if (!s || (n && !data)) return YAMS_ERR_INVALID_ARG;
    auto* hs = static_cast<HashStream*>(s);
    size_t pos = 0;
    while (pos < n) { // bounded host buffer: flush whole blocks every kStreamFlush bytes
        const size_t take = std::min(n - pos, kStreamFlush - std::min(kStreamFlush, hs->pending.size()) + 64);
        hs->pending.insert(hs->pending.end(), data + pos, data + pos + take);
        hs->total += take;
        pos += take;
        if (hs->pending.size() >= kStreamFlush) {
            const yams_status_t st = flush_whole_blocks(hs);
            if (st != YAMS_OK) return st;
        }
    }
    return YAMS_OK;
}
yams_status_t ch_stream_finalize(void*, void* s, char out_hex[65]) {
    NEED_INIT();
    if (!s || !out_hex) return YAMS_ERR_INVALID_ARG;
    auto* hs = static_cast<HashStream*>(s);
    // padding: 0x80, zeros, the bit length as a big-endian 64-bit word
    const uint64_t bits = hs->total * 8;
    hs->pending.push_back(0x80);
    while (hs->pending.size() % 64 != 56) hs->pending.push_back(0);
    for (int i = 7; i >= 0; --i) hs->pending.push_back(static_cast<uint8_t>(bits >> (8 * i)));
    const yams_status_t st = flush_whole_blocks(hs);
    if (st != YAMS_OK) return st;
    uint8_t digest[32];            // the state's words, big-endian
    for (int i = 0; i < 32; ++i) digest[i] = static_cast<uint8_t>(hs->state[i / 4] >> (24 - 8 * (i % 4)));
    to_hex(digest, out_hex);
    // "Reset for potential reuse" (sha256_hasher.cpp:103-106)
    std::memcpy(hs->state, kShaInit, 32);
    hs->pending.clear(); hs->total = 0;
    ++g.hashes;
    return YAMS_OK;
}
void ch_stream_destroy(void*, void* s) { delete static_cast<HashStream*>(s); }

yams_status_t ch_verify_many(void*, const uint8_t* const* msgs, const size_t* lens, const char* expected_hex,
                             size_t n, uint8_t* out_valid) {
    if (n == 0) return YAMS_OK;
    if (!msgs || !lens || !expected_hex || !out_valid) return YAMS_ERR_INVALID_ARG;
    if (!chains_suit_the_device(lens, n)) { ++g.refused_chains; return YAMS_ERR_UNSUPPORTED; }
    std::vector<char> hex(n * 65);
    {
        NEED_INIT();
        Lease<yams_accel_ctx*> w(g.work_ctx);
        g.hashes += n;
        yams_status_t s = yams_sha256_many_host(w.v, msgs, lens, n, hex.data());
        if (s != YAMS_OK) return s;
    }
    for (size_t i = 0; i < n; ++i) { // the reference compares the lower-case hex strings (:243-249)
        uint8_t a[32], b[32];
        out_valid[i] = (parse_hex32(hex.data() + 65 * i, a) && parse_hex32(expected_hex + 65 * i, b) &&
                        std::memcmp(a, b, 32) == 0) ? 1 : 0;
    }
    return YAMS_OK;
}

// Dedup sets: each owns a context (its table lives in that context's device memory) and a mutex.
struct DedupEntry { yams_accel_ctx* ctx = nullptr; yams_dedup_set* set = nullptr; std::mutex mu; };
std::mutex g_dedup_mu;
std::map<uint64_t, std::shared_ptr<DedupEntry>> g_dedup;
uint64_t g_next_dedup = 1;

std::shared_ptr<DedupEntry> find_dedup(uint64_t id) {
    std::lock_guard<std::mutex> lk(g_dedup_mu);
    auto it = g_dedup.find(id);
    return it == g_dedup.end() ? nullptr : it->second;
}
void destroy_dedup(DedupEntry& e) {
    if (e.set) yams_dedup_set_destroy(e.set);
    if (e.ctx) yams_accel_ctx_destroy(e.ctx);
    e.set = nullptr; e.ctx = nullptr;
}

yams_status_t ch_dedup_create(void*, uint64_t expected, uint64_t* out_id) {
    NEED_INIT();
    if (!out_id) return YAMS_ERR_INVALID_ARG;
    auto e = std::make_shared<DedupEntry>();
    yams_status_t st = yams_accel_ctx_create(g.devices[0], nullptr, &e->ctx);
    if (st != YAMS_OK) return st;
    st = yams_dedup_set_create(e->ctx, expected, &e->set);
    if (st != YAMS_OK) { destroy_dedup(*e); return st; }
    std::lock_guard<std::mutex> lk(g_dedup_mu);
    *out_id = g_next_dedup++;
    g_dedup[*out_id] = e;
    return YAMS_OK;
}
yams_status_t dedup_call(uint64_t id, const char* hashes_hex, size_t n, uint8_t* out, bool insert) {
    NEED_INIT();
    auto e = find_dedup(id);
    if (!e) return YAMS_ERR_NOT_FOUND;
    if (n == 0) return YAMS_OK;
    if (!hashes_hex || !out) return YAMS_ERR_INVALID_ARG;
    std::vector<uint8_t> raw(n * 32);
    for (size_t i = 0; i < n; ++i)
        if (!parse_hex32(hashes_hex + 65 * i, raw.data() + 32 * i)) return YAMS_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->set) return YAMS_ERR_NOT_FOUND;
    return insert ? yams_dedup_insert_host(e->set, raw.data(), n, out, nullptr)
                  : yams_dedup_probe_host(e->set, raw.data(), n, out);
}
yams_status_t ch_dedup_insert(void*, uint64_t id, const char* hex, size_t n, uint8_t* out) { return dedup_call(id, hex, n, out, true); }
yams_status_t ch_dedup_contains(void*, uint64_t id, const char* hex, size_t n, uint8_t* out) { return dedup_call(id, hex, n, out, false); }
yams_status_t ch_dedup_size(void*, uint64_t id, uint64_t* out_entries) {
    NEED_INIT();
    auto e = find_dedup(id);
    if (!e) return YAMS_ERR_NOT_FOUND;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->set) return YAMS_ERR_NOT_FOUND;
    return yams_dedup_set_size(e->set, out_entries);
}
yams_status_t ch_dedup_destroy(void*, uint64_t id) {
    NEED_INIT();
    std::shared_ptr<DedupEntry> e;
    {
        std::lock_guard<std::mutex> lk(g_dedup_mu);
        auto it = g_dedup.find(id);
        if (it == g_dedup.end()) return YAMS_ERR_NOT_FOUND;
        e = it->second;
        g_dedup.erase(it);
    }
    std::lock_guard<std::mutex> lk(e->mu);
    destroy_dedup(*e);
    return YAMS_OK;
}

yams_content_hash_v1 g_content_hash = {YAMS_IFACE_CONTENT_HASH_V1_VERSION, nullptr, GUARDED(ch_hash),
                                       GUARDED(ch_hash_many), GUARDED(ch_stream_create), GUARDED(ch_stream_init),
                                       GUARDED(ch_stream_update), GUARDED(ch_stream_finalize), GUARDED(ch_stream_destroy),
                                       GUARDED(ch_verify_many), GUARDED(ch_dedup_create), GUARDED(ch_dedup_insert),
                                       GUARDED(ch_dedup_contains), GUARDED(ch_dedup_size), GUARDED(ch_dedup_destroy)};

// ---- topology_route_v1: the cluster router's dense signal over a resident index (yams_route_index_* / yams_route_dense_host) ----
// Route indexes: each owns a context (its table lives in that context's device memory, its calls use that context's workspace)
// and a mutex — the shape of the dedup sets above.
struct RouteEntry { yams_accel_ctx* ctx = nullptr; yams_route_index* index = nullptr; std::mutex mu; };
std::mutex g_route_mu;
std::map<uint64_t, std::shared_ptr<RouteEntry>> g_route;
uint64_t g_next_route = 1;

void destroy_route(RouteEntry& e) {
    if (e.index) yams_route_index_destroy(e.index);
    if (e.ctx) yams_accel_ctx_destroy(e.ctx);
    e.index = nullptr; e.ctx = nullptr;
}
std::shared_ptr<RouteEntry> find_route(uint64_t id) {
    std::lock_guard<std::mutex> lk(g_route_mu);
    auto it = g_route.find(id);
    return it == g_route.end() ? nullptr : it->second;
}

yams_status_t tr_index_create(void*, const float* vectors, uint64_t n_vectors, uint32_t dim, const uint32_t* cluster_offsets,
                              const uint8_t* has_centroid, const uint16_t* position, uint32_t n_clusters, uint64_t* out_id, float* out_norms) {
    NEED_INIT();
    if (!out_id) return YAMS_ERR_INVALID_ARG;
    auto e = std::make_shared<RouteEntry>();
    yams_status_t st = yams_accel_ctx_create(g.devices[0], nullptr, &e->ctx);
    if (st != YAMS_OK) return st;
    st = yams_route_index_create_host(e->ctx, vectors, n_vectors, dim, cluster_offsets, has_centroid, position, n_clusters, &e->index, out_norms);
    if (st != YAMS_OK) { destroy_route(*e); return st; }
    std::lock_guard<std::mutex> lk(g_route_mu);
    *out_id = g_next_route++;
    g_route[*out_id] = e;
    return YAMS_OK;
}
yams_status_t tr_index_info(void*, uint64_t id, yams_route_index_info_t* out_info) {
    NEED_INIT();
    auto e = find_route(id);
    if (!e) return YAMS_ERR_NOT_FOUND;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->index) return YAMS_ERR_NOT_FOUND;
    return yams_route_index_info(e->index, out_info);
}
yams_status_t tr_dense(void*, uint64_t id, const float* queries, uint32_t n_queries, uint32_t rep_limit, const uint32_t* candidates,
                       float* out_dense, uint8_t* out_observed, uint32_t* out_evals, yams_route_diag_t* out_diag) {
    NEED_INIT();
    auto e = find_route(id);
    if (!e) return YAMS_ERR_NOT_FOUND;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->index) return YAMS_ERR_NOT_FOUND;
    return yams_route_dense_host(e->index, queries, n_queries, rep_limit, candidates, out_dense, out_observed, out_evals, out_diag);
}
yams_status_t tr_index_destroy(void*, uint64_t id) {
    NEED_INIT();
    std::shared_ptr<RouteEntry> e;
    {
        std::lock_guard<std::mutex> lk(g_route_mu);
        auto it = g_route.find(id);
        if (it == g_route.end()) return YAMS_ERR_NOT_FOUND;
        e = it->second;
        g_route.erase(it);
    }
    std::lock_guard<std::mutex> lk(e->mu);
    destroy_route(*e);
    return YAMS_OK;
}

yams_topology_route_v1 g_topology_route = {YAMS_IFACE_TOPOLOGY_ROUTE_V1_VERSION, nullptr, GUARDED(tr_index_create), GUARDED(tr_index_info),
                                           GUARDED(tr_dense), GUARDED(tr_index_destroy)};

// ---- topology_quality_v1: computePersistenceH0 over host memory (yams_quality_persistence_h0_host) --------------------------
// the limits bound the arrays allocated here; every other check is the flat entry's
yams_status_t tq_persistence_h0(void*, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select,
                                uint32_t form, yams_persistence_h0_t* out, double** out_distances, double** out_merge_weights) {
    NEED_INIT();
    if (!out) return YAMS_ERR_INVALID_ARG;
    const uint64_t m = select ? n_select : n;
    if (m > YAMS_QUALITY_MAX_POINTS || dim > YAMS_CLUSTER_MAX_DIM || n >= (1ull << 31)) return YAMS_ERR_UNSUPPORTED;
    double* dist = nullptr; double* w = nullptr;
    if (out_distances && m) dist = static_cast<double*>(std::malloc(static_cast<size_t>(m) * m * 8));
    if (out_merge_weights && m >= 2) w = static_cast<double*>(std::malloc(static_cast<size_t>(m - 1) * 8));
    if ((out_distances && m && !dist) || (out_merge_weights && m >= 2 && !w)) { std::free(dist); std::free(w); return YAMS_ERR_RESOURCE_EXHAUSTED; }
    yams_persistence_h0_t res{};
    yams_status_t st;
    {
        Lease<yams_accel_ctx*> lease(g.work_ctx);
        st = yams_quality_persistence_h0_host(lease.v, rows, n, dim, select, n_select, form, &res, dist, w, nullptr);
    }
    if (st != YAMS_OK) { std::free(dist); std::free(w); return st; }
    *out = res;
    if (out_distances) *out_distances = dist;
    if (out_merge_weights) *out_merge_weights = w;
    return YAMS_OK;
}
void tq_free_persistence_h0(void*, double* distances, double* merge_weights) { std::free(distances); std::free(merge_weights); }

yams_topology_quality_v1 g_topology_quality = {YAMS_IFACE_TOPOLOGY_QUALITY_V1_VERSION, nullptr, GUARDED(tq_persistence_h0),
                                               GUARDED(tq_free_persistence_h0)};

// ---- topology_features_v1: the topology build's input features over host memory (yams_features_*_host) ----------------------
// every output is the caller's array: every check is the flat entry's
yams_status_t tf_aggregate(void*, const float* rows, uint64_t n_records, uint32_t dim, const uint64_t* doc_offsets, const uint32_t* records,
                           uint64_t n_docs, float* out, uint32_t* out_counts) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    return yams_features_aggregate_host(lease.v, rows, n_records, dim, doc_offsets, records, n_docs, out, out_counts);
}
yams_status_t tf_variance(void*, const float* rows, uint64_t n, uint32_t dim, const uint32_t* select, uint64_t n_select, uint32_t form,
                          double* out_mean, double* out_var) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    return yams_features_variance_host(lease.v, rows, n, dim, select, n_select, form, out_mean, out_var);
}
yams_status_t tf_compose(void*, const float* dense, uint64_t n, uint32_t dim, const float* weights, const float* entity, uint32_t k,
                         const uint8_t* entity_on, const uint32_t* sig, uint32_t sig_len, const uint8_t* sketch_on, uint32_t sketch_dim,
                         float alpha_e, float alpha_m, float* out, uint32_t out_stride, uint32_t* out_dims) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    return yams_features_compose_host(lease.v, dense, n, dim, weights, entity, k, entity_on, sig, sig_len, sketch_on, sketch_dim, alpha_e,
                                      alpha_m, out, out_stride, out_dims);
}

yams_topology_features_v1 g_topology_features = {YAMS_IFACE_TOPOLOGY_FEATURES_V1_VERSION, nullptr, GUARDED(tf_aggregate), GUARDED(tf_variance),
                                                 GUARDED(tf_compose)};

// ---- late_interaction_rerank_v1: ColBERT MaxSim and token pooling over host memory (yams_rerank_*_host) ----------------------
// every output is the caller's array: every check is the flat entry's
yams_status_t lr_maxsim(void*, const float* query, uint32_t tq, uint32_t dim, const float* rows, const uint64_t* doc_offsets, uint64_t n_docs,
                        uint32_t form, float* out_scores, float* out_rowmax, uint32_t* out_rowarg, yams_rerank_diag_t* diag) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    return yams_rerank_maxsim_host(lease.v, query, tq, dim, rows, doc_offsets, n_docs, form, out_scores, out_rowmax, out_rowarg, diag);
}
yams_status_t lr_maxpool(void*, const float* rows, uint32_t dim, const uint64_t* doc_offsets, uint64_t n_docs, float* out) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    return yams_rerank_maxpool_host(lease.v, rows, dim, doc_offsets, n_docs, out);
}

yams_late_interaction_rerank_v1 g_late_rerank = {YAMS_IFACE_LATE_INTERACTION_RERANK_V1_VERSION, nullptr, GUARDED(lr_maxsim), GUARDED(lr_maxpool)};

// ---- embedding_pool_v1: the embedding model's pooling head (yams_embed_*), over host memory or over device addresses -----------
// every output is the caller's array: every check is the flat entry's
yams_status_t ep_pool(void*, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask, uint32_t mask_len,
                      uint32_t mode, uint32_t flags, float* out, yams_embed_diag_t* diag) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    return yams_embed_pool_host(lease.v, hidden, batch, seq, dim, mask, mask_len, mode, flags, out, diag);
}
yams_status_t ep_normalize(void*, const float* rows, uint64_t batch, uint32_t dim, float* out) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    return yams_embed_normalize_host(lease.v, rows, batch, dim, out);
}
// the hidden states (the rows) at a DEVICE address, everything else in host memory: the mask goes up, the B * dim result comes back
yams_status_t ep_pool_device(void*, const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask, uint32_t mask_len,
                             uint32_t mode, uint32_t flags, float* out, yams_embed_diag_t* diag) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    yams_accel_ctx* ctx = lease.v;
    // what the flat entry refuses (or, batch == 0, answers) before it looks at a mask or an output: its verdict, nothing is staged
    if (batch == 0 || !out || dim == 0 || seq == 0 || dim > YAMS_EMBED_MAX_DIM || seq > YAMS_EMBED_MAX_SEQ || batch > YAMS_EMBED_MAX_ROWS / seq)
        return yams_embed_pool_device(ctx, hidden, batch, seq, dim, nullptr, mask_len, mode, flags, out, diag);
    // only the considered columns of the mask go up: at most batch * seq values
    if (mode == YAMS_EMBED_POOL_CLS) mask = nullptr;
    const uint32_t cols = mask_len < seq ? mask_len : seq;
    const size_t mb = mask ? static_cast<size_t>(batch) * cols * 4 : 0, ob = static_cast<size_t>(batch) * dim * 4;
    int32_t* d_mask = nullptr; float* d_out;
    if (mb) YA_TRY(yams_accel::ws_get(ctx, "embed_door_mask", mb, (void**)&d_mask));
    YA_TRY(yams_accel::ws_get(ctx, "embed_door_out", ob, (void**)&d_out));
    if (mb && cols == mask_len) YA_HIP(ctx, yams_accel::staged_h2d(d_mask, mask, mb, ctx->stream));
    else if (mb) YA_HIP(ctx, hipMemcpy2DAsync(d_mask, static_cast<size_t>(cols) * 4, mask, static_cast<size_t>(mask_len) * 4, static_cast<size_t>(cols) * 4, batch, hipMemcpyHostToDevice, ctx->stream));
    if (mask && !mb) mask_len = 0;
    else if (mask) mask_len = cols;
    YA_TRY(yams_embed_pool_device(ctx, hidden, batch, seq, dim, d_mask, mask_len, mode, flags, d_out, diag));
    YA_HIP(ctx, hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    YA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return YAMS_OK;
}
yams_status_t ep_normalize_device(void*, const float* rows, uint64_t batch, uint32_t dim, float* out) {
    NEED_INIT();
    Lease<yams_accel_ctx*> lease(g.work_ctx);
    yams_accel_ctx* ctx = lease.v;
    if (batch == 0 || !out || dim == 0 || dim > YAMS_EMBED_MAX_DIM || batch > YAMS_EMBED_MAX_ROWS)
        return yams_embed_normalize_device(ctx, rows, batch, dim, out);      // its verdict; nothing is staged
    const size_t ob = static_cast<size_t>(batch) * dim * 4;
    float* d_out;
    YA_TRY(yams_accel::ws_get(ctx, "embed_door_out", ob, (void**)&d_out));
    YA_TRY(yams_embed_normalize_device(ctx, rows, batch, dim, d_out));
    YA_HIP(ctx, hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    YA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return YAMS_OK;
}

yams_embedding_pool_v1 g_embedding_pool = {YAMS_IFACE_EMBEDDING_POOL_V1_VERSION, nullptr, GUARDED(ep_pool), GUARDED(ep_normalize),
                                           GUARDED(ep_pool_device), GUARDED(ep_normalize_device)};

// ---- content_checksum_v1: the compressed store's CRC-32 over host memory (yams_crc32_many_host) ------------------------------
yams_status_t cs_crc32_many(void*, const uint8_t* const* msgs, const size_t* lens, size_t n, uint32_t* out) {
    NEED_INIT();
    Lease<yams_accel_ctx*> w(g.work_ctx);
    return yams_crc32_many_host(w.v, msgs, lens, n, out);
}
yams_status_t cs_crc32(void*, const uint8_t* data, size_t n, uint32_t* out) {
    NEED_INIT();
    if (!out || (n && !data)) return YAMS_ERR_INVALID_ARG;
    const uint8_t* msgs[1] = {data};
    const size_t lens[1] = {n};
    Lease<yams_accel_ctx*> w(g.work_ctx);
    return yams_crc32_many_host(w.v, msgs, lens, 1, out);
}
yams_status_t cs_verify_many(void*, const uint8_t* const* msgs, const size_t* lens, const uint32_t* expected, size_t n, uint8_t* out_valid) {
    NEED_INIT();
    if (n == 0) return YAMS_OK;
    if (!msgs || !lens || !expected || !out_valid) return YAMS_ERR_INVALID_ARG;
    std::vector<uint32_t> got(n);
    {
        Lease<yams_accel_ctx*> w(g.work_ctx);
        const yams_status_t s = yams_crc32_many_host(w.v, msgs, lens, n, got.data());
        if (s != YAMS_OK) return s;
    }
    for (size_t i = 0; i < n; ++i) out_valid[i] = got[i] == expected[i] ? 1 : 0;
    return YAMS_OK;
}

yams_content_checksum_v1 g_content_checksum = {YAMS_IFACE_CONTENT_CHECKSUM_V1_VERSION, nullptr, GUARDED(cs_crc32), GUARDED(cs_crc32_many),
                                               GUARDED(cs_verify_many)};

// ---- chunker_v1 -------------------------------------------------------------------------------
yams_status_t ck_default_config(void*, uint32_t mode, yams_cdc_config_t* out_cfg) {
    if (!out_cfg || (mode != YAMS_CDC_RABIN && mode != YAMS_CDC_STREAMING)) return YAMS_ERR_INVALID_ARG;
    yams_cdc_default_config(out_cfg, mode);
    return YAMS_OK;
}
// re-entrant: ContentStore shares one chunker across its workers (content_store_impl.cpp:1412)
// One buffer; the first context_len bytes are history (chunk_window: a window of a stream), 0 for chunk_data.
yams_status_t ck_chunk_window(void*, const uint8_t* data, size_t n, size_t context_len, const yams_cdc_config_t* cfg,
                              yams_chunk_ref_t** out_chunks, size_t* out_count) {
    NEED_INIT();
    if (!out_chunks || !out_count || !cfg) return YAMS_ERR_INVALID_ARG;
    *out_chunks = nullptr; *out_count = 0;
    const uint64_t floor = std::max<uint64_t>(1, cfg->min_size);
    size_t cap = n / floor + 2;
    std::vector<uint64_t> off(cap), sz(cap);
    std::vector<char> hex(cap * 65);
    size_t cnt = 0;
    yams_status_t s;
    {
        Lease<yams_accel_ctx*> w(g.work_ctx);
        s = yams_cdc_chunk_window_host(w.v, data, n, context_len, cfg, off.data(), sz.data(), hex.data(), cap, &cnt);
    }
    if (s != YAMS_OK) return s;
    auto* chunks = static_cast<yams_chunk_ref_t*>(std::calloc(std::max<size_t>(cnt, 1), sizeof(yams_chunk_ref_t)));
    if (!chunks) return YAMS_ERR_INTERNAL;
    for (size_t i = 0; i < cnt; ++i) {
        chunks[i].offset = off[i]; chunks[i].size = sz[i];
        std::memcpy(chunks[i].hash_hex, hex.data() + 65 * i, 65);
    }
    ++g.chunk_calls;
    *out_chunks = chunks; *out_count = cnt;
    return YAMS_OK;
}
yams_status_t ck_chunk_data(void* self, const uint8_t* data, size_t n, const yams_cdc_config_t* cfg,
                            yams_chunk_ref_t** out_chunks, size_t* out_count) {
    return ck_chunk_window(self, data, n, 0, cfg, out_chunks, out_count);
}
void ck_free_chunks(void*, yams_chunk_ref_t* chunks, size_t) { std::free(chunks); }

void ck_free_chunk_batch(void*, yams_chunk_batch_t* b) {
    if (!b) return;
    std::free(b->first_chunk); std::free(b->chunks); std::free(b->buffer_hash_hex); std::free(b);
}
// Many buffers per call: the batched ingest path (yams_ingest_host) behind the plugin door.
yams_status_t ck_chunk_many(void*, const uint8_t* const* buffers, const size_t* lens, size_t n, const yams_cdc_config_t* cfg,
                            uint32_t flags, yams_chunk_batch_t** out_batch) {
    NEED_INIT();
    if (!out_batch) return YAMS_ERR_INVALID_ARG;
    *out_batch = nullptr;
    if (!cfg || (n && (!buffers || !lens))) return YAMS_ERR_INVALID_ARG;
    const bool want_blob = (flags & YAMS_CHUNK_MANY_BUFFER_HASHES) != 0;
    const bool defer = want_blob && (flags & YAMS_CHUNK_MANY_DEFER_LONG_BUFFER_HASHES) != 0;
    // First guess of the chunk count: one chunk per `floor` bytes, where floor is the smallest chunk the configuration
    // can emit in the common case — min(min, max), but never below 256 bytes (min_size == 0 is a legal configuration:
    // a per-byte bound would be ~48 bytes of host vectors per input byte).  Should the guess be too low (min > max, or
    // a degenerate mask) yams_ingest_host reports the required size and the call runs once more with exactly that.
    uint64_t floor = std::min<uint64_t>(cfg->min_size ? cfg->min_size : cfg->max_size, cfg->max_size ? cfg->max_size : cfg->min_size);
    floor = std::max<uint64_t>(floor, 256);
    std::vector<uint64_t> len64(n);
    uint64_t cap = 0, total = 0;
    for (size_t i = 0; i < n; ++i) { len64[i] = lens[i]; cap += lens[i] / floor + 2; total += lens[i]; }
    std::vector<uint64_t> first(n + 1, 0), off, sz;
    std::vector<uint8_t> dig, bdig(want_blob ? n * 32 : 0);
    uint64_t cnt = 0;
    if (n) {
        Lease<yams_accel_ctx*> w(g.work_ctx);
        for (int attempt = 0; ; ++attempt) {
            off.assign(cap, 0); sz.assign(cap, 0); dig.assign(cap * 32, 0);
            const yams_status_t s = yams_ingest_host(w.v, buffers, len64.data(), n, cfg,
                                                     YAMS_INGEST_CHUNK_DIGESTS | (want_blob ? YAMS_INGEST_BLOB_DIGESTS : 0u) |
                                                         (defer ? YAMS_INGEST_DEFER_LONG_BLOB_DIGESTS : 0u), 0,
                                                     first.data(), off.data(), sz.data(), dig.data(), cap,
                                                     want_blob ? bdig.data() : nullptr, &cnt);
            if (s == YAMS_OK) break;
            if (s == YAMS_ERR_INVALID_ARG && attempt == 0 && cnt > cap) { cap = cnt; continue; } // "chunk arrays too small": cnt is the required size
            return s;
        }
    }
    const uint64_t defer_above = defer ? yams_ingest_defer_threshold_host(total) : UINT64_MAX;
    auto* b = static_cast<yams_chunk_batch_t*>(std::calloc(1, sizeof(yams_chunk_batch_t)));
    if (!b) return YAMS_ERR_INTERNAL;
    b->n_buffers = n; b->n_chunks = static_cast<size_t>(cnt);
    b->first_chunk = static_cast<size_t*>(std::calloc(n + 1, sizeof(size_t)));
    b->chunks = static_cast<yams_chunk_ref_t*>(std::calloc(std::max<size_t>(b->n_chunks, 1), sizeof(yams_chunk_ref_t)));
    b->buffer_hash_hex = want_blob ? static_cast<char*>(std::calloc(std::max<size_t>(n, 1), 65)) : nullptr;
    if (!b->first_chunk || !b->chunks || (want_blob && !b->buffer_hash_hex)) { ck_free_chunk_batch(nullptr, b); return YAMS_ERR_INTERNAL; }
    for (size_t i = 0; i <= n; ++i) b->first_chunk[i] = static_cast<size_t>(first[i]);
    for (size_t i = 0; i < b->n_chunks; ++i) {
        b->chunks[i].offset = off[i]; b->chunks[i].size = sz[i];
        to_hex(dig.data() + 32 * i, b->chunks[i].hash_hex);
    }
    if (want_blob)
        for (size_t i = 0; i < n; ++i) {
            if (len64[i] > defer_above) { ++g.deferred_chains; continue; } // (calloc'd: the entry stays empty — the host's hasher fills it)
            to_hex(bdig.data() + 32 * i, b->buffer_hash_hex + 65 * i);
        }
    g.chunk_calls += n;
    *out_batch = b;
    return YAMS_OK;
}

yams_chunker_v1 g_chunker = {YAMS_IFACE_CHUNKER_V1_VERSION, nullptr, GUARDED(ck_default_config),
                             GUARDED(ck_chunk_data), GUARDED(ck_free_chunks), GUARDED(ck_chunk_many),
                             GUARDED(ck_free_chunk_batch), GUARDED(ck_chunk_window)};

void teardown_locked() { // g.mu held exclusively
    {
        std::lock_guard<std::mutex> lk(g.corpora_mu);
        for (auto& kv : g.corpora) { std::unique_lock<std::shared_mutex> cl(kv.second->mu); release_corpus(*kv.second); }
        g.corpora.clear();
    }
    {
        std::lock_guard<std::mutex> lk(g_dedup_mu);
        for (auto& kv : g_dedup) { std::lock_guard<std::mutex> el(kv.second->mu); destroy_dedup(*kv.second); }
        g_dedup.clear();
    }
    {
        std::lock_guard<std::mutex> lk(g_route_mu);
        for (auto& kv : g_route) { std::lock_guard<std::mutex> el(kv.second->mu); destroy_route(*kv.second); }
        g_route.clear();
    }
    if (g.sharded) yams_scan_sharded_destroy(g.sharded);
    g.sharded = nullptr;
    for (auto* c : g.work_ctx.drain()) yams_accel_ctx_destroy(c);
    for (auto* c : g.upload_ctx) yams_accel_ctx_destroy(c);
    g.upload_ctx.clear();
    g.initialised = false;
    // nothing reads the parked mirrors of destroyed corpora any more: their physical memory goes back to the driver
    GrowBuf::evict_all_parked();
}

} // namespace

extern "C" {

int yams_plugin_get_abi_version(void) { return YAMS_PLUGIN_ABI_VERSION; }
const char* yams_plugin_get_name(void) { return "yams_mi355x_accel"; }
const char* yams_plugin_get_version(void) { return YAMS_ACCEL_VERSION_STRING; }
const char* yams_plugin_get_manifest_json(void) { return kManifest; }

// host_context is a yams_plugin_host_context_v1* (host_services_v1.h:19-26); unused here.  The
// legacy one-argument form (abi_plugin_loader.cpp:329-357) is tolerated: the second argument is
// never dereferenced.  config_json: {"device": n} or {"devices": [..]} (a corpus is dealt to all of
// them in stripes and searched behind one call), "search_slots": concurrent searches (default 2),
// "shadows": "both" (default) | "bf16" | "i8" | "none", "collective": "auto" | "rccl" | "peer",
// "rccl_library": "<path>", "fence": "off", "l2_accumulate": "f64" (default) | "f32" | "f32x8" | "f32x16" | "f32_fma" |
// "f32x8_fma" | "f32x16_fma".  Read by a strict tokenizer (struct Config): unknown keys are ignored, a known key with a value
// of the wrong type or an enumerated value that is not listed fails the init (YAMS_PLUGIN_ERR_INIT_FAILED).
static int plugin_init_impl(const char* config_json, const void* host_context) {
    (void)host_context;
    std::unique_lock<std::shared_mutex> lk(g.mu);
    if (g.initialised) return YAMS_PLUGIN_OK;
    auto failed = [&](const char* why) {
        g.init_error = why;
        for (char& ch : g.init_error) if (ch == '"' || ch == '\\') ch = '\'';   // (the health JSON quotes it as is)
        teardown_locked();
        return YAMS_PLUGIN_ERR_INIT_FAILED; // the host keeps its built-in CPU backends
    };
    Config cfg(config_json);
    if (!cfg.error.empty()) return failed(("configuration: " + cfg.error).c_str());
    long v_device = 0, slots = 2, sr = 65536, ex_timeout = 0;
    int shadows = 0, l2 = 0, collective = 0, fence = 0;
    std::string library; bool has_library = false;
    const bool cfg_ok =
        cfg.get_int("device", 0, v_device) && cfg.get_int("search_slots", 2, slots) && cfg.get_int("stripe_rows", 65536, sr) &&
        cfg.get_int("exchange_timeout_ms", 0, ex_timeout) &&
        cfg.get_choice("shadows", {"both", "bf16", "i8", "none"}, 0, shadows) &&
        // layout of the int8 shadow (YAMS_SCAN_I8_ROTATED in the header): measured per corpus at its first append, or fixed
        cfg.get_choice("i8_layout", {"auto", "plain", "rotated"}, 0, g.i8_layout) &&
        // the arithmetic of vec0's L2 distance the host's sqlite-vec-cpp build uses (YAMS_SCAN_FLAG_L2_ACC_* in the header;
        // "..._fma": the same lanes accumulated with ONE fused multiply-add per element, what '-mavx', '-mfma' builds do)
        cfg.get_choice("l2_accumulate", {"f64", "f32", "f32x8", "f32x16", "f32_fma", "f32x8_fma", "f32x16_fma"}, 0, l2) &&
        cfg.get_choice("collective", {"auto", "rccl", "peer"}, 0, collective) &&
        cfg.get_choice("fence", {"auto", "on", "off"}, 0, fence) &&
        cfg.get_string("rccl_library", library, has_library);
    if (!cfg_ok) return failed(("configuration: " + cfg.error).c_str());
    g.devices.clear();
    if (cfg.has("devices")) {
        const auto it = cfg.int_lists.find("devices");
        if (it == cfg.int_lists.end() || it->second.empty()) return failed("configuration: \"devices\" must be a non-empty array of integers");
        for (long d : it->second) g.devices.push_back(static_cast<int>(d));
    } else g.devices.push_back(static_cast<int>(v_device));
    slots = std::max<long>(1, std::min<long>(16, slots));
    kStripeRows = static_cast<uint32_t>(std::max<long>(64, std::min<long>(1 << 24, sr)) / 64 * 64);
    g.want_bf16 = shadows == 0 || shadows == 1;
    g.want_i8 = shadows == 0 || shadows == 2;
    static const uint32_t kL2Acc[7] = {YAMS_SCAN_FLAG_L2_ACC_F64, YAMS_SCAN_FLAG_L2_ACC_F32, YAMS_SCAN_FLAG_L2_ACC_F32X8, YAMS_SCAN_FLAG_L2_ACC_F32X16,
                                       YAMS_SCAN_FLAG_L2_ACC_F32 | YAMS_SCAN_FLAG_L2_ACC_FUSED, YAMS_SCAN_FLAG_L2_ACC_F32X8 | YAMS_SCAN_FLAG_L2_ACC_FUSED,
                                       YAMS_SCAN_FLAG_L2_ACC_F32X16 | YAMS_SCAN_FLAG_L2_ACC_FUSED};
    g.l2_acc = kL2Acc[l2];
    g.append_bytes = 0; g.appends = 0; g.exhausted_appends = 0; g.append_map_ms = 0; g.append_copy_ms = 0; g.append_shadow_ms = 0;
    g.slow_append_ms = 0; g.slow_map_ms = 0; g.slow_copy_ms = 0; g.slow_shadow_ms = 0; g.slow_append_bytes = 0;
    for (size_t i = 0; i < g.devices.size(); ++i) {
        yams_accel_ctx* c = nullptr;
        const yams_status_t s = yams_accel_ctx_create(g.devices[i], nullptr, &c);
        if (s != YAMS_OK) return failed(s == YAMS_ERR_UNSUPPORTED ? "no gfx950 device visible" : "context creation failed");
        g.upload_ctx.push_back(c);
    }
    {
        yams_scan_sharded_options_t so{};
        so.struct_size = sizeof so; so.lanes = static_cast<uint32_t>(slots); so.collective = YAMS_SHARDED_COLLECTIVE_AUTO;
        // "collective": "rccl" (require it) | "peer" | "auto"; "rccl_library": "<path>" — the collective library to bind instead of
        // librccl.so.1 (a site build; the test suite's stand-in, with which several shards may share a device); "fence": "off"
        // lifts the exchange fence; "exchange_timeout_ms": deadline of a sharded batch (default 30000; a batch that misses it
        // fails with YAMS_ERR_TIMEOUT and the sharded handle is stuck until the plugin is shut down and initialised again)
        so.collective = collective == 1 ? YAMS_SHARDED_COLLECTIVE_RCCL : (collective == 2 ? YAMS_SHARDED_COLLECTIVE_PEER : YAMS_SHARDED_COLLECTIVE_AUTO);
        if (has_library && !library.empty()) so.rccl_library = library.c_str();
        so.exchange_timeout_ms = static_cast<uint32_t>(std::max<long>(0, ex_timeout));
        if (fence == 2) so.fence = YAMS_SHARDED_FENCE_OFF;
        if (yams_scan_sharded_create_ex(g.devices.data(), static_cast<uint32_t>(g.devices.size()), &so, &g.sharded) != YAMS_OK)
            return failed("sharded search handle creation failed");
        g.search_slots = static_cast<uint32_t>(slots);
    }
    for (long i = 0; i < std::max<long>(2, slots); ++i) {
        yams_accel_ctx* c = nullptr;
        if (yams_accel_ctx_create(g.devices[0], nullptr, &c) != YAMS_OK) return failed("work context creation failed");
        g.work_ctx.add(c);
    }
    g.initialised = true;
    g.init_error.clear();
    return YAMS_PLUGIN_OK;
}

int yams_plugin_init(const char* config_json, const void* host_context) {
    try { return plugin_init_impl(config_json, host_context); }
    catch (...) { return YAMS_PLUGIN_ERR_INIT_FAILED; } // the host keeps its built-in CPU backends
}

void yams_plugin_shutdown(void) {
    try {
        std::unique_lock<std::shared_mutex> lk(g.mu);
        if (g.initialised) teardown_locked();
    } catch (...) {}
}

// Returns a pointer to a static vtable; unknown id or version -> NOT_FOUND, null args -> INVALID
// (plugins/glint/plugin.cpp:338-359, tools/fuzzing/fuzz_abi_test_plugin.c:48-60).
int yams_plugin_get_interface(const char* iface_id, uint32_t version, void** out_iface) {
    if (!iface_id || !out_iface) return YAMS_PLUGIN_ERR_INVALID;
    *out_iface = nullptr;
    // (only vector_scan_v1, content_hash_v1 and chunker_v1 are in the manifest: see the header)
    const struct { const char* id; uint32_t max_version; void* vtable; } kInterfaces[] = {
        {YAMS_IFACE_VECTOR_SCAN_V1, YAMS_IFACE_VECTOR_SCAN_V1_VERSION, &g_vector_scan},
        {YAMS_IFACE_VECTOR_DOC_SCAN_V1, YAMS_IFACE_VECTOR_DOC_SCAN_V1_VERSION, &g_vector_doc_scan},
        {YAMS_IFACE_VECTOR_ENTITY_SCAN_V1, YAMS_IFACE_VECTOR_ENTITY_SCAN_V1_VERSION, &g_vector_entity_scan},
        {YAMS_IFACE_TOPOLOGY_CLUSTER_V1, YAMS_IFACE_TOPOLOGY_CLUSTER_V1_VERSION, &g_topology_cluster},
        {YAMS_IFACE_SEMANTIC_GRAPH_V1, YAMS_IFACE_SEMANTIC_GRAPH_V1_VERSION, &g_semantic_graph},
        {YAMS_IFACE_TOPOLOGY_SMOOTH_V1, YAMS_IFACE_TOPOLOGY_SMOOTH_V1_VERSION, &g_topology_smooth},
        {YAMS_IFACE_TOPOLOGY_ARTIFACTS_V1, YAMS_IFACE_TOPOLOGY_ARTIFACTS_V1_VERSION, &g_topology_artifacts},
        {YAMS_IFACE_TOPOLOGY_ROUTE_V1, YAMS_IFACE_TOPOLOGY_ROUTE_V1_VERSION, &g_topology_route},
        {YAMS_IFACE_TOPOLOGY_QUALITY_V1, YAMS_IFACE_TOPOLOGY_QUALITY_V1_VERSION, &g_topology_quality},
        {YAMS_IFACE_TOPOLOGY_FEATURES_V1, YAMS_IFACE_TOPOLOGY_FEATURES_V1_VERSION, &g_topology_features},
        {YAMS_IFACE_LATE_INTERACTION_RERANK_V1, YAMS_IFACE_LATE_INTERACTION_RERANK_V1_VERSION, &g_late_rerank},
        {YAMS_IFACE_EMBEDDING_POOL_V1, YAMS_IFACE_EMBEDDING_POOL_V1_VERSION, &g_embedding_pool},
        {YAMS_IFACE_CONTENT_HASH_V1, YAMS_IFACE_CONTENT_HASH_V1_VERSION, &g_content_hash},
        {YAMS_IFACE_CONTENT_CHECKSUM_V1, YAMS_IFACE_CONTENT_CHECKSUM_V1_VERSION, &g_content_checksum},
        {YAMS_IFACE_CHUNKER_V1, YAMS_IFACE_CHUNKER_V1_VERSION, &g_chunker}};
    for (const auto& f : kInterfaces)
        if (std::strcmp(iface_id, f.id) == 0) {
            if (version < 1 || version > f.max_version) return YAMS_PLUGIN_ERR_NOT_FOUND;
            *out_iface = f.vtable;
            return YAMS_PLUGIN_OK;
        }
    return YAMS_PLUGIN_ERR_NOT_FOUND;
}

// malloc'd; the host free()s it (abi_plugin_loader.cpp:481-500).
static int plugin_health_impl(char** out_json) {
    if (!out_json) return YAMS_PLUGIN_ERR_INVALID;
    std::shared_lock<std::shared_mutex> lk(g.mu);
    std::ostringstream os;
    size_t n_corpora;
    // device memory behind the mirrors: mapped into live corpora, and parked (mappings of destroyed corpora waiting for
    // the next one) — what an allocation-failure test watches for leaks
    uint64_t mirror_mapped = 0, mirror_parked = 0;
    size_t rotated_corpora = 0;
    {
        std::lock_guard<std::mutex> cl(g.corpora_mu);
        n_corpora = g.corpora.size();
        for (auto& kv : g.corpora) {
            rotated_corpora += kv.second->i8_flags > 0 && (kv.second->i8_flags & static_cast<int>(YAMS_SCAN_I8_ROTATED));
            for (auto& s : kv.second->sh)
                for (const GrowBuf* b : {&s.rows, &s.bf16, &s.i8, &s.nsq, &s.i8meta, &s.tie, &s.inv}) mirror_mapped += b->mapped;
            mirror_mapped += kv.second->rank_of_row.mapped;
        }
    }
    {
        std::lock_guard<std::mutex> pl(g_park_mu);
        for (auto& kv : g_parked) for (auto& b : kv.second) mirror_parked += b.mapped;
    }
    os << "{\"status\":\"" << (g.initialised ? "ok" : "not_initialised") << "\",\"devices\":[";
    for (size_t i = 0; i < g.devices.size(); ++i) os << (i ? "," : "") << g.devices[i];
    os << "],\"device\":" << (g.devices.empty() ? 0 : g.devices[0]) << ",\"search_slots\":" << g.search_slots
       << ",\"l2_accumulate\":\"" << ((g.l2_acc & YAMS_SCAN_FLAG_L2_ACC_MASK) == YAMS_SCAN_FLAG_L2_ACC_F32X16 ? "f32x16" : (g.l2_acc & YAMS_SCAN_FLAG_L2_ACC_MASK) == YAMS_SCAN_FLAG_L2_ACC_F32X8 ? "f32x8" : (g.l2_acc & YAMS_SCAN_FLAG_L2_ACC_MASK) == YAMS_SCAN_FLAG_L2_ACC_F32 ? "f32" : "f64")
       << ((g.l2_acc & YAMS_SCAN_FLAG_L2_ACC_FUSED) ? "_fma" : "") << "\""
       << ",\"i8_layout\":\"" << (g.i8_layout == 2 ? "rotated" : g.i8_layout == 1 ? "plain" : "auto") << "\",\"corpora_with_rotated_i8_shadow\":" << rotated_corpora
       << ",\"last_append\":{\"bytes\":" << g.append_bytes.load() << ",\"map_ms\":" << g.append_map_ms.load() << ",\"copy_ms\":" << g.append_copy_ms.load()
       << ",\"shadow_ms\":" << g.append_shadow_ms.load() << "}"
       << ",\"appends\":" << g.appends.load() << ",\"exhausted_appends\":" << g.exhausted_appends.load()
       << ",\"slowest_append\":{\"bytes\":" << g.slow_append_bytes.load() << ",\"ms\":" << g.slow_append_ms.load() << ",\"map_ms\":" << g.slow_map_ms.load()
       << ",\"copy_ms\":" << g.slow_copy_ms.load() << ",\"shadow_ms\":" << g.slow_shadow_ms.load() << "}"
       << ",\"mirror_bytes_mapped\":" << mirror_mapped << ",\"mirror_bytes_parked\":" << mirror_parked
       << ",\"alloc_faults_injected\":" << yams_accel_debug_alloc_faults()
       << ",\"corpora\":" << n_corpora << ",\"searches\":" << g.searches.load() << ",\"hashes\":" << g.hashes.load()
       << ",\"chunk_calls\":" << g.chunk_calls.load()
       << ",\"refused_lone_chains\":" << g.refused_chains.load() << ",\"deferred_buffer_hashes\":" << g.deferred_chains.load();
    if (g.sharded) { // how the shards exchange their records: "collective":"rccl" | "peer_copy" | "none" (one device)
        char* info = nullptr;
        if (yams_scan_sharded_info_json(g.sharded, &info) == YAMS_OK && info) { os << ",\"sharded\":" << info; std::free(info); }
    }
    if (!g.init_error.empty()) os << ",\"error\":\"" << g.init_error << "\"";
    os << "}";
    const std::string s = os.str();
    char* buf = static_cast<char*>(std::malloc(s.size() + 1));
    if (!buf) return YAMS_PLUGIN_ERR_INIT_FAILED;
    std::memcpy(buf, s.c_str(), s.size() + 1);
    *out_json = buf;
    return YAMS_PLUGIN_OK;
}

int yams_plugin_get_health_json(char** out_json) {
    try { return plugin_health_impl(out_json); }
    catch (...) { return YAMS_PLUGIN_ERR_INIT_FAILED; }
}

} // extern "C"
