// plugin_content.cpp — the plugin door's content families: content_hash_v1 (one-shot and streaming SHA-256, batch verification,
// the dedup sets), content_checksum_v1 and chunker_v1.
#include "ingest_launch.h"
#include "plugin_state.h"

namespace yams_accel {
namespace door {
namespace {

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

using DedupSet = Handle<yams_dedup_set, yams_dedup_set_destroy>;
HandleTable<DedupSet> dedup_sets;

yams_status_t ch_dedup_create(void*, uint64_t expected, uint64_t* out_id) {
    NEED_INIT();
    if (!out_id) return YAMS_ERR_INVALID_ARG;
    auto e = std::make_shared<DedupSet>();
    yams_status_t st = yams_accel_ctx_create(g.devices[0], nullptr, &e->ctx);
    if (st != YAMS_OK) return st;
    st = yams_dedup_set_create(e->ctx, expected, &e->obj);
    if (st != YAMS_OK) { e->destroy(); return st; }
    *out_id = dedup_sets.insert(e);
    return YAMS_OK;
}
yams_status_t dedup_call(uint64_t id, const char* hashes_hex, size_t n, uint8_t* out, bool insert) {
    NEED_INIT();
    auto e = dedup_sets.find(id);
    if (!e) return YAMS_ERR_NOT_FOUND;
    if (n == 0) return YAMS_OK;
    if (!hashes_hex || !out) return YAMS_ERR_INVALID_ARG;
    std::vector<uint8_t> raw(n * 32);
    for (size_t i = 0; i < n; ++i)
        if (!parse_hex32(hashes_hex + 65 * i, raw.data() + 32 * i)) return YAMS_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->obj) return YAMS_ERR_NOT_FOUND;
    return insert ? yams_dedup_insert_host(e->obj, raw.data(), n, out, nullptr)
                  : yams_dedup_probe_host(e->obj, raw.data(), n, out);
}
yams_status_t ch_dedup_insert(void*, uint64_t id, const char* hex, size_t n, uint8_t* out) { return dedup_call(id, hex, n, out, true); }
yams_status_t ch_dedup_contains(void*, uint64_t id, const char* hex, size_t n, uint8_t* out) { return dedup_call(id, hex, n, out, false); }
yams_status_t ch_dedup_size(void*, uint64_t id, uint64_t* out_entries) {
    NEED_INIT();
    auto e = dedup_sets.find(id);
    if (!e) return YAMS_ERR_NOT_FOUND;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->obj) return YAMS_ERR_NOT_FOUND;
    return yams_dedup_set_size(e->obj, out_entries);
}
yams_status_t ch_dedup_destroy(void*, uint64_t id) {
    NEED_INIT();
    auto e = dedup_sets.take(id);
    if (!e) return YAMS_ERR_NOT_FOUND;
    std::lock_guard<std::mutex> lk(e->mu);
    e->destroy();
    return YAMS_OK;
}

// ---- content_checksum_v1: the compressed store's CRC-32 over host memory (yams_crc32_many_host) ------------------------------
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

} // namespace

yams_content_hash_v1 g_content_hash = {YAMS_IFACE_CONTENT_HASH_V1_VERSION, nullptr, GUARDED(ch_hash),
                                       GUARDED(ch_hash_many), GUARDED(ch_stream_create), GUARDED(ch_stream_init),
                                       GUARDED(ch_stream_update), GUARDED(ch_stream_finalize), GUARDED(ch_stream_destroy),
                                       GUARDED(ch_verify_many), GUARDED(ch_dedup_create), GUARDED(ch_dedup_insert),
                                       GUARDED(ch_dedup_contains), GUARDED(ch_dedup_size), GUARDED(ch_dedup_destroy)};
yams_content_checksum_v1 g_content_checksum = {YAMS_IFACE_CONTENT_CHECKSUM_V1_VERSION, nullptr, GUARDED(cs_crc32), GUARDED(Leased<&yams_crc32_many_host>::call),
                                               GUARDED(cs_verify_many)};
yams_chunker_v1 g_chunker = {YAMS_IFACE_CHUNKER_V1_VERSION, nullptr, GUARDED(ck_default_config),
                             GUARDED(ck_chunk_data), GUARDED(ck_free_chunks), GUARDED(ck_chunk_many),
                             GUARDED(ck_free_chunk_batch), GUARDED(ck_chunk_window)};

void teardown_content() { dedup_sets.drain([](DedupSet& e) { e.destroy(); }); }

} // namespace door
} // namespace yams_accel
