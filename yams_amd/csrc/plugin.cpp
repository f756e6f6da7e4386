// plugin.cpp — the YAMS plugin surface of libyams_mi355x_accel.so.
//
// Exports the eight entry points of the reference's include/yams/plugins/abi.h:26-34 and serves fifteen interface vtables
// written to the conventions of include/yams/plugins/model_provider_v1.h:44-49.  The host side that would load this file is
// AbiPluginLoader::load / getInterface (src/daemon/resource/abi_plugin_loader.cpp:270-442, 657-681): dlopen(RTLD_LAZY|
// RTLD_LOCAL), yams_plugin_init(config_json, host_context), yams_plugin_get_manifest_json, then
// yams_plugin_get_interface(id, version, &vtable).
//
// Where the door's parts live:
//   plugin.cpp            the corpus mirror and the three vtables over it (vector_scan_v1, vector_doc_scan_v1,
//                         vector_entity_scan_v1), configuration and init, shutdown, health, the table of the fifteen interfaces
//   plugin_topology.cpp   topology_cluster_v1, semantic_graph_v1, topology_smooth_v1, topology_artifacts_v1, topology_route_v1,
//                         topology_quality_v1, topology_features_v1, late_interaction_rerank_v1, embedding_pool_v1
//   plugin_content.cpp    content_hash_v1, content_checksum_v1, chunker_v1
//   plugin_state.h        what the three share: the guard of every entry, the work-context pool and its lease, the forwarder
//                         of the entries that only lease and call, the plugin's state
//   grow_buf.h            the device buffer behind a mirror, which grows in place
//   plugin_host.h         what the door computes on the host alone (configuration, row / mask / rank dealing, hit packing,
//                         hex) and its two ownership rules (OwnedArrays / HitResult, HandleTable); tested on the CPU
#include <chrono>
#include <cstdio>
#include <sstream>

#include "grow_buf.h"
#include "plugin_state.h"

// The eight entry points and their return codes are declared in include/yams_mi355x_accel.h exactly as
// the reference's include/yams/plugins/abi.h:18-34 declares them (no local restatement here).

namespace yams_accel {
namespace door {

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

PluginState& g = *new PluginState;   // never destroyed: when a host exits without yams_plugin_shutdown, the corpora's DevArrays must
                                     // not reach hipFree from a static destructor (the runtime may have gone before them)

namespace {

// rows of a stripe when a corpus is dealt to several devices (config "stripe_rows", a multiple of 64;
// fixed at init: it is part of every corpus's row -> shard map)
uint32_t kStripeRows = 65536;

const char kManifest[] =
    "{\"name\":\"yams_mi355x_accel\",\"version\":\"" YAMS_ACCEL_VERSION_STRING "\",\"abi\":1,"
    "\"description\":\"MI355X (gfx950) exact vector scan, SHA-256 and content-defined chunking\","
    "\"interfaces\":[{\"id\":\"vector_scan_v1\",\"version\":1},"
    "{\"id\":\"content_hash_v1\",\"version\":1},{\"id\":\"chunker_v1\",\"version\":3}]}";

std::shared_ptr<Corpus> find_corpus(uint64_t id) { return g.corpora.find(id); }

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
    *out_id = g.corpora.insert(c);
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
    auto c = g.corpora.take(id);
    if (!c) return YAMS_ERR_NOT_FOUND;
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



yams_vector_scan_v1 g_vector_scan = {
    YAMS_IFACE_VECTOR_SCAN_V1_VERSION, nullptr, GUARDED(vs_corpus_create), GUARDED(vs_corpus_append),
    GUARDED(vs_corpus_set_tie_ranks), GUARDED(vs_corpus_clear), GUARDED(vs_corpus_destroy), GUARDED(vs_corpus_size),
    GUARDED(vs_search_batch), GUARDED(free_arrays<yams_scan_hit_t, uint32_t>), GUARDED(Leased<&yams_accel_device_info_json>::call), GUARDED(free_arrays<char>),
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

yams_vector_doc_scan_v1 g_vector_doc_scan = {YAMS_IFACE_VECTOR_DOC_SCAN_V1_VERSION, nullptr, GUARDED(ds_corpus_set_documents),
                                             GUARDED(ds_search_docs), GUARDED(free_arrays<yams_scan_hit_t, uint32_t>)};

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

yams_vector_entity_scan_v1 g_vector_entity_scan = {YAMS_IFACE_VECTOR_ENTITY_SCAN_V1_VERSION, nullptr, GUARDED(es_corpus_set_attributes),
                                                   GUARDED(es_search_entities), GUARDED(free_arrays<yams_scan_hit_t, uint32_t>)};

void teardown_locked() { // g.mu held exclusively
    g.corpora.drain(release_corpus);
    teardown_content();      // the dedup sets
    teardown_topology();     // the route indexes
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
} // namespace door
} // namespace yams_accel

using namespace yams_accel::door;

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
    // device memory behind the mirrors: mapped into live corpora, and parked (mappings of destroyed corpora waiting for
    // the next one) — what an allocation-failure test watches for leaks
    uint64_t mirror_mapped = 0, mirror_parked = 0;
    size_t rotated_corpora = 0;
    const size_t n_corpora = g.corpora.size();
    g.corpora.visit([&](const Corpus& c) {
        rotated_corpora += c.i8_flags > 0 && (c.i8_flags & static_cast<int>(YAMS_SCAN_I8_ROTATED));
        for (auto& s : c.sh)
            for (const GrowBuf* b : {&s.rows, &s.bf16, &s.i8, &s.nsq, &s.i8meta, &s.tie, &s.inv}) mirror_mapped += b->mapped;
        mirror_mapped += c.rank_of_row.mapped;
    });
    mirror_parked = GrowBuf::parked_bytes();
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
