// plugin_host.h — the plugin door's pure host logic (plugin.cpp is the door).
//
// What the door computes on the host before and after a device call: the strict reader of its configuration, the dealing
// of rows, allow-masks and tie ranks to the shards of a striped corpus, the ranking of the PQ engine's keys, the packing of
// hits, hex — and the door's two ownership rules: the malloc'd arrays a call hands out (OwnedArrays, HitResult) and the registry
// of a handle family (HandleTable).  No HIP call and no global: the stripe width is a parameter, and the local -> global direction of the dealing
// is contract_rules.h's global_row_id, the function the kernels undo the dealing with.  Compiles with g++ -std=c++17 and no
// ROCm include path; tests/cpp/plugin_host_test.cpp holds every function here on the CPU, under ASan and UBSan.
#pragma once
#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <set>
#include <string>
#include <vector>

#include "contract_rules.h"

namespace yams_accel {
namespace plugin_host {

// ---- the plugin's configuration: a strict reader of ONE flat JSON object ----------------------------------------------------
// {"key": "string" | integer | [integers] | true | false | null | {...} | [...]}: keys the plugin does not know are skipped
// (whatever their value, nested or not); a key it knows with a value of the wrong TYPE, an enumerated value it does not
// list, or text that is not a JSON object fails yams_plugin_init — a host's typo must not silently serve another arithmetic
// (round 5 read its keys with strstr: {"shadows":"none","note":"both"} enabled both shadows).
struct Config {
    std::map<std::string, std::string> strings;
    std::map<std::string, long> ints;
    std::map<std::string, std::vector<long>> int_lists;
    std::set<std::string> other;       // keys present with a value of another type (booleans, null, objects, nested arrays, floats)
    std::string error;                 // non-empty: the text did not parse

    static void ws(const char*& p) { while (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r') ++p; }
    static bool str(const char*& p, std::string& out) {
        if (*p != '"') return false;
        out.clear();
        for (++p; *p && *p != '"'; ++p) {
            if (*p == '\\') { ++p; if (!*p) return false; out.push_back(*p == 'n' ? '\n' : (*p == 't' ? '\t' : *p)); }
            else out.push_back(*p);
        }
        if (*p != '"') return false;
        ++p;
        return true;
    }
    static bool integer(const char*& p, long& v) {
        char* e = nullptr;
        v = std::strtol(p, &e, 10);
        if (e == p || *e == '.' || *e == 'e' || *e == 'E') return false;
        p = e;
        return true;
    }
    static bool skip(const char*& p, int depth = 0) {   // any JSON value
        ws(p);
        if (depth > 32) return false;
        std::string t;
        if (*p == '"') return str(p, t);
        if (*p == '{' || *p == '[') {
            const char close = *p == '{' ? '}' : ']';
            const bool object = *p == '{';
            ++p; ws(p);
            if (*p == close) { ++p; return true; }
            for (;;) {
                ws(p);
                if (object) { if (!str(p, t)) return false; ws(p); if (*p++ != ':') return false; }
                if (!skip(p, depth + 1)) return false;
                ws(p);
                if (*p == ',') { ++p; continue; }
                if (*p == close) { ++p; return true; }
                return false;
            }
        }
        const char* b = p;
        while (*p && (std::isalnum(static_cast<unsigned char>(*p)) || *p == '-' || *p == '+' || *p == '.')) ++p;
        return p != b;
    }
    explicit Config(const char* json) {
        if (!json) return;
        const char* p = json;
        ws(p);
        if (!*p) return;                                // "" = no configuration
        if (*p != '{') { error = "the configuration is not a JSON object"; return; }
        ++p; ws(p);
        if (*p == '}') { ++p; ws(p); if (*p) error = "text after the configuration object"; return; }
        for (;;) {
            std::string key;
            ws(p);
            if (!str(p, key)) { error = "expected a key"; return; }
            ws(p);
            if (*p++ != ':') { error = "expected ':' after \"" + key + "\""; return; }
            ws(p);
            if (*p == '"') { std::string v; if (!str(p, v)) { error = "unterminated string for \"" + key + "\""; return; } strings[key] = v; }
            else if (*p == '-' || std::isdigit(static_cast<unsigned char>(*p))) {
                const char* q = p; long v;
                if (integer(q, v)) { ints[key] = v; p = q; }
                else { if (!skip(p)) { error = "bad number for \"" + key + "\""; return; } other.insert(key); }
            } else if (*p == '[') {
                const char* q = p + 1; std::vector<long> lst; bool ok = true;
                ws(q);
                if (*q == ']') ++q;
                else for (;;) {
                    long v; ws(q);
                    if (!integer(q, v)) { ok = false; break; }
                    lst.push_back(v); ws(q);
                    if (*q == ',') { ++q; continue; }
                    if (*q == ']') { ++q; break; }
                    ok = false; break;
                }
                if (ok) { int_lists[key] = lst; p = q; }
                else { if (!skip(p)) { error = "bad array for \"" + key + "\""; return; } other.insert(key); }
            } else { if (!skip(p)) { error = "bad value for \"" + key + "\""; return; } other.insert(key); }
            ws(p);
            if (*p == ',') { ++p; continue; }
            if (*p == '}') { ++p; break; }
            error = "expected ',' or '}' after \"" + key + "\""; return;
        }
        ws(p);
        if (*p) error = "text after the configuration object";
    }
    bool has(const std::string& k) const { return strings.count(k) || ints.count(k) || int_lists.count(k) || other.count(k); }
    // typed reads: false (with `error` set) when the key is there with another type
    bool get_int(const std::string& k, long dflt, long& out) {
        out = dflt;
        if (!has(k)) return true;
        const auto it = ints.find(k);
        if (it == ints.end()) { error = "\"" + k + "\" must be an integer"; return false; }
        out = it->second;
        return true;
    }
    bool get_string(const std::string& k, std::string& out, bool& present) {
        present = false;
        if (!has(k)) return true;
        const auto it = strings.find(k);
        if (it == strings.end()) { error = "\"" + k + "\" must be a string"; return false; }
        out = it->second; present = true;
        return true;
    }
    // an enumerated string: index into `allowed`, dflt when absent; false on any other value
    bool get_choice(const std::string& k, std::initializer_list<const char*> allowed, int dflt, int& out) {
        out = dflt;
        std::string v; bool present;
        if (!get_string(k, v, present)) return false;
        if (!present) return true;
        int i = 0;
        for (const char* a : allowed) { if (v == a) { out = i; return true; } ++i; }
        error = "\"" + k + "\": \"" + v + "\" is not one of";
        for (const char* a : allowed) error += std::string(" \"") + a + "\"";
        return false;
    }
};

// ---- the stripe dealing: global row -> (shard, local row); one shard holds everything, in order ---------------------------
inline uint32_t shard_of(uint64_t row, uint32_t stripe_rows, uint32_t n_sh) {
    return n_sh == 1 ? 0u : static_cast<uint32_t>((row / stripe_rows) % n_sh);
}
inline uint64_t local_of(uint64_t row, uint32_t stripe_rows, uint32_t n_sh) {
    return n_sh == 1 ? row : (row / stripe_rows / n_sh) * stripe_rows + row % stripe_rows;
}
// rows of a corpus of n rows that live on shard i
inline uint64_t shard_rows(uint64_t n, uint32_t stripe_rows, uint32_t n_sh, uint32_t i) {
    if (n_sh == 1) return n;
    const uint64_t full = n / stripe_rows, rem = n % stripe_rows;
    uint64_t r = (full / n_sh) * stripe_rows + ((full % n_sh) > i ? stripe_rows : 0);
    if (full % n_sh == i) r += rem;
    return r;
}
// ... and back: the rule the kernels turn a shard's row ordinal into the caller's row id with (a shard holds < 2^32 rows)
inline uint64_t global_of(uint64_t local, uint32_t stripe_rows, uint32_t n_sh, uint32_t i) {
    return static_cast<uint64_t>(global_row_id(0, n_sh == 1 ? 0u : stripe_rows, n_sh, i, static_cast<uint32_t>(local)));
}

// The host's allow-mask over GLOBAL rows (document_hash / candidate_hashes restriction, :4137-4175), dealt like the rows:
// shard i's words over its `local_rows` LOCAL rows, and how many bits they hold.  stripe_rows % 32 == 0, so a local word is
// a global word; bits at or beyond local_rows are cleared.  One shard: the copy of the words, its tail trimmed.
struct DealtMask { std::vector<uint32_t> words; uint64_t bits = 0; };
inline DealtMask deal_row_mask(const uint32_t* global_words, uint64_t local_rows, uint32_t stripe_rows, uint32_t n_sh, uint32_t i) {
    DealtMask m;
    m.words.resize((local_rows + 31) / 32);
    for (size_t w = 0; w < m.words.size(); ++w) {
        const uint64_t l0 = static_cast<uint64_t>(w) * 32;
        uint32_t v = global_words[global_of(l0, stripe_rows, n_sh, i) >> 5];
        if (local_rows - l0 < 32) v &= (1u << (local_rows - l0)) - 1u;
        m.words[w] = v;
        m.bits += static_cast<uint64_t>(__builtin_popcount(v));
    }
    return m;
}

// Shard i's tie ranks from the corpus-wide ones: a permutation of 0..nl-1 that preserves the global order (the scan sorts
// ties by it inside the shard; the merge compares the global ranks through rank_of_row), and its inverse.
inline void local_tie_ranks(const uint32_t* ranks, uint64_t nl, uint32_t stripe_rows, uint32_t n_sh, uint32_t i,
                            std::vector<uint32_t>& lrank, std::vector<uint32_t>& linv) {
    std::vector<uint32_t> glob(nl), order(nl);
    lrank.resize(nl); linv.resize(nl);
    for (uint64_t l = 0; l < nl; ++l) glob[l] = ranks[global_of(l, stripe_rows, n_sh, i)];
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return glob[x] < glob[y]; });
    for (uint32_t p = 0; p < nl; ++p) { lrank[order[p]] = p; linv[p] = order[p]; }
}

// The PQ engine's tie-break keys: the rank of every key (ascending key, equal keys by index: the comparator of :3985-3990;
// no keys: the index order) and the mirror row behind every rank (no table: the key's own index).
inline void rank_pq_keys(const uint64_t* tie_keys, const uint32_t* row_of_index, uint64_t n, std::vector<uint32_t>& rank,
                         std::vector<uint32_t>& key_row) {
    std::vector<uint32_t> order(n);
    rank.resize(n); key_row.resize(n);
    std::iota(order.begin(), order.end(), 0u);
    if (tie_keys)
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return tie_keys[a] != tie_keys[b] ? tie_keys[a] < tie_keys[b] : a < b; });
    for (uint64_t r = 0; r < n; ++r) { rank[order[r]] = static_cast<uint32_t>(r); key_row[r] = row_of_index ? row_of_index[order[r]] : order[r]; }
}

// v[0..n) holds every value of 0..n-1 once
inline bool is_permutation_of_iota(const uint32_t* v, uint64_t n) {
    std::vector<uint8_t> seen(n, 0);
    for (uint64_t r = 0; r < n; ++r) {
        if (v[r] >= n || seen[v[r]]) return false;
        seen[v[r]] = 1;
    }
    return true;
}

// (counts[nq], rows / scores / dist[nq][k]) -> hits[nq][k].  `dist` null: distance = 1 - score (the cosine engines,
// utils::similarityToDistance); a slot beyond its query's count reads {-1, 0, 0}.
inline void pack_hits(uint32_t nq, uint32_t k, const uint32_t* counts, const int64_t* rows, const float* scores, const float* dist,
                      yams_scan_hit_t* hits) {
    for (uint32_t q = 0; q < nq; ++q)
        for (uint32_t i = 0; i < k; ++i) {
            const size_t o = static_cast<size_t>(q) * k + i;
            if (i < counts[q]) { hits[o].row = rows[o]; hits[o].similarity = scores[o]; hits[o].distance = dist ? dist[o] : 1.0f - scores[o]; }
            else { hits[o].row = -1; hits[o].similarity = 0.f; hits[o].distance = 0.f; }
        }
}

// ---- what a door hands to its caller: malloc'd arrays that go with the object unless they are committed -------------------
// add() allocates count elements behind the out parameter `out` (not wanted: no array, the out parameter still gets its null;
// a wanted array of no elements is one byte, never a null that reads as a failure); ok() is false once a wanted allocation
// failed or its size overflows size_t.  commit() writes every array to its out parameter (a null out parameter is skipped)
// and lets go of them: the caller frees them through the vtable's free function.  What was not committed is freed here, so a
// door returns from any failure as it stands and its out parameters stay as it left them.
class OwnedArrays {
public:
    OwnedArrays() = default;
    OwnedArrays(const OwnedArrays&) = delete;
    OwnedArrays& operator=(const OwnedArrays&) = delete;
    ~OwnedArrays() { for (const Slot& s : slots_) std::free(s.p); }
    template <typename T> T* add(T** out, size_t count, bool wanted = true) {
        slots_.push_back(Slot{nullptr, out});      // (first: an array is never without its slot)
        if (!wanted) return nullptr;
        if (count > SIZE_MAX / sizeof(T)) { ok_ = false; return nullptr; }
        slots_.back().p = std::malloc(std::max<size_t>(count * sizeof(T), 1));
        if (!slots_.back().p) ok_ = false;
        return static_cast<T*>(slots_.back().p);
    }
    bool ok() const { return ok_; }
    yams_status_t commit() {
        for (const Slot& s : slots_) if (s.out) std::memcpy(s.out, &s.p, sizeof s.p);      // (*out = p, whatever the element type)
        slots_.clear();
        return YAMS_OK;
    }
private:
    struct Slot { void* p; void* out; };
    std::vector<Slot> slots_;
    bool ok_ = true;
};

// The malloc'd result of a search: hits[nq * max(k, 1)], every row preset to -1, and counts[max(nq, 1)], zeroed.  commit()
// hands both to the caller (who frees them through the vtable's free function); what was not committed goes with the object.
// (The same rule as OwnedArrays; written out, because its two arrays are calloc'd and preset.)
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

// ---- the registry of a handle family: id -> entry ---------------------------------------------------------------------------
// Ids start at 1 and are never reused within the table's life (not after take(), not after drain(): an id a host kept
// across a shutdown names nothing afterwards).  An Entry carries its own mutex `mu` and its payload.  find() and take() hand
// out a shared_ptr, so an entry outlives its removal for as long as a call holds it: whoever took it locks `mu` and destroys
// the payload; a call that found it earlier locks `mu`, sees the payload gone and answers NOT_FOUND.
template <typename Entry> class HandleTable {
public:
    uint64_t insert(std::shared_ptr<Entry> e) { std::lock_guard<std::mutex> lk(mu_); map_[next_] = std::move(e); return next_++; }
    std::shared_ptr<Entry> find(uint64_t id) { return get(id, false); }
    std::shared_ptr<Entry> take(uint64_t id) { return get(id, true); }      // removed; its contents are the caller's to destroy, under the entry's mu
    template <typename F> void drain(F&& destroy) {   // teardown: every entry, locked; the table is empty afterwards
        std::lock_guard<std::mutex> lk(mu_);
        for (auto& kv : map_) { std::unique_lock<decltype(kv.second->mu)> el(kv.second->mu); destroy(*kv.second); }
        map_.clear();
    }
    template <typename F> void visit(F&& look) {      // every entry, NOT locked: for figures that may be a moment old
        std::lock_guard<std::mutex> lk(mu_);
        for (auto& kv : map_) look(*kv.second);
    }
    size_t size() { std::lock_guard<std::mutex> lk(mu_); return map_.size(); }
private:
    std::shared_ptr<Entry> get(uint64_t id, bool remove) {
        std::lock_guard<std::mutex> lk(mu_);
        const auto it = map_.find(id);
        if (it == map_.end()) return nullptr;
        std::shared_ptr<Entry> e = it->second;
        if (remove) map_.erase(it);
        return e;
    }
    std::mutex mu_;
    std::map<uint64_t, std::shared_ptr<Entry>> map_;
    uint64_t next_ = 1;
};

// One SHA-256 chain is sequential: ~35 MB/s on a device lane, > 1 GB/s on a host core.  Work the device is worse
// at is refused (YAMS_ERR_UNSUPPORTED: the host hashes it itself), not served slowly — see the public header.
inline bool chains_suit_the_device(const size_t* lens, size_t n) {
    size_t longest = 0, total = 0;
    for (size_t i = 0; i < n; ++i) { longest = std::max(longest, lens[i]); total += lens[i]; }
    return longest <= std::max<size_t>(YAMS_HASH_LONE_CHAIN_MAX, total / YAMS_HASH_CHAIN_RATIO);
}

// hex (either case) -> 32 raw bytes; false on anything that is not 64 hex digits
inline bool parse_hex32(const char* hex, uint8_t out[32]) {
    for (int i = 0; i < 32; ++i) {
        int v = 0;
        for (int j = 0; j < 2; ++j) {
            const char c = hex[2 * i + j];
            int d;
            if (c >= '0' && c <= '9') d = c - '0';
            else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
            else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
            else return false;
            v = v * 16 + d;
        }
        out[i] = static_cast<uint8_t>(v);
    }
    return hex[64] == 0;
}
inline void to_hex(const uint8_t* d, char out[65]) {
    static const char kHexDigits[] = "0123456789abcdef";
    for (int i = 0; i < 32; ++i) { out[2 * i] = kHexDigits[d[i] >> 4]; out[2 * i + 1] = kHexDigits[d[i] & 15]; }
    out[64] = 0;
}

} // namespace plugin_host
} // namespace yams_accel
