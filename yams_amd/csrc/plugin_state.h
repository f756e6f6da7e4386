// plugin_state.h — what the translation units of the plugin door share (plugin.cpp, plugin_topology.cpp, plugin_content.cpp): the
// guard every vtable entry wears, the pool of work contexts and its lease, the forwarder, the shape of a handle, the plugin's
// state `g`, and what each family file gives to plugin.cpp.  Nothing here is exported (-fvisibility=hidden).
#pragma once
#include <atomic>
#include <condition_variable>
#include <shared_mutex>
#include <type_traits>

#include "accel_ctx.h"
#include "plugin_host.h"

namespace yams_accel {
namespace door {
using namespace yams_accel::plugin_host;

// No exception may cross the C ABI (model_provider_v1.h:44-49; the reference's own plugins wrap every entry point,
// plugins/onnx/model_provider.cpp:51,94,105): every function pointer of every vtable is the guarded form of
// its implementation — std::bad_alloc from an absurd batch size, or anything else thrown below, becomes
// YAMS_ERR_INTERNAL (void functions just return).
template <auto Fn> struct Guard;
template <typename R, typename... A, R (*Fn)(A...)> struct Guard<Fn> {
    static R call(A... a) noexcept {
        try { return Fn(a...); }
        catch (...) { if constexpr (!std::is_void_v<R>) return static_cast<R>(YAMS_ERR_INTERNAL); }
    }
};
#define GUARDED(...) (&Guard<&__VA_ARGS__>::call)

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

struct Corpus;      // (plugin.cpp: the mirror of one corpus)
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
    HandleTable<Corpus> corpora;             // (an entry's own lock is Corpus::mu: searches share it, mutations exclude)
    std::atomic<uint64_t> searches{0}, hashes{0}, chunk_calls{0}, refused_chains{0}, deferred_chains{0};
};

extern PluginState& g;      // (plugin.cpp)

#define NEED_INIT() std::shared_lock<std::shared_mutex> init_lk__(g.mu); do { if (!g.initialised) return YAMS_ERR_UNSUPPORTED; } while (0)

// An object that lives across calls (a dedup set, a route index), kept in a HandleTable: it owns a context — its table lives in
// that context's device memory, its calls use that context's workspace — and a mutex.  destroy() runs under `mu`; a call that
// takes `mu` afterwards finds `obj` null.
template <typename T, void (*Destroy)(T*)> struct Handle {
    yams_accel_ctx* ctx = nullptr; T* obj = nullptr; std::mutex mu;
    void destroy() { if (obj) Destroy(obj); if (ctx) yams_accel_ctx_destroy(ctx); obj = nullptr; ctx = nullptr; }
};

// What a door committed (OwnedArrays, HitResult) comes back through its vtable's free function: free() of every array, null or not.
template <typename... T> void free_arrays(void*, T*... arrays) { (std::free(arrays), ...); }

// An entry whose every check is its flat entry's: lease a work context, forward.  Leased<&yams_xxx_host>::call has the flat
// entry's parameters with the vtable's `self` in place of the context.
template <auto Fn> struct Leased;
template <typename... A, yams_status_t (*Fn)(yams_accel_ctx*, A...)> struct Leased<Fn> {
    static yams_status_t call(void*, A... a) {
        NEED_INIT();
        Lease<yams_accel_ctx*> lease(g.work_ctx);
        return Fn(lease.v, a...);
    }
};

// plugin_topology.cpp
extern yams_topology_cluster_v1 g_topology_cluster;
extern yams_semantic_graph_v1 g_semantic_graph;
extern yams_topology_smooth_v1 g_topology_smooth;
extern yams_topology_artifacts_v1 g_topology_artifacts;
extern yams_topology_route_v1 g_topology_route;
extern yams_topology_quality_v1 g_topology_quality;
extern yams_topology_features_v1 g_topology_features;
extern yams_late_interaction_rerank_v1 g_late_rerank;
extern yams_embedding_pool_v1 g_embedding_pool;
void teardown_topology();      // the route indexes (g.mu held exclusively)
// plugin_content.cpp
extern yams_content_hash_v1 g_content_hash;
extern yams_content_checksum_v1 g_content_checksum;
extern yams_chunker_v1 g_chunker;
void teardown_content();       // the dedup sets (g.mu held exclusively)

} // namespace door
} // namespace yams_accel
