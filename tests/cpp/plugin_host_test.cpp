// plugin_host_test.cpp — the plugin door's host logic (yams_amd/csrc/plugin_host.h) on the CPU.
//
// Plain g++, no GPU, no ROCm include path; built with -fsanitize=address,undefined.  Every array handed to the header is
// a heap array of exactly the length its contract states, so a read or write past the contract fails the run.
//
//   plugin_host_test           runs every case, prints one line per failure and "OK (0 failures)"
//   plugin_host_test --threads eight threads on one HandleTable, nothing else (the -fsanitize=thread build runs only this)
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../yams_amd/csrc/plugin_host.h"

using namespace yams_accel;
using namespace yams_accel::plugin_host;

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

constexpr uint32_t kStripe = 64;   // the smallest stripe the configuration admits
std::mt19937_64 g_rng(20240611);

std::vector<uint64_t> lattice(uint32_t n_sh) {
    const uint64_t s = kStripe * n_sh;
    return {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, s - 1, s, s + 1, 2 * s + 17, 1000};
}
bool bit(const std::vector<uint32_t>& words, uint64_t r) { return (words[r >> 5] >> (r & 31)) & 1u; }
std::vector<uint32_t> random_permutation(uint64_t n) {
    std::vector<uint32_t> p(n);
    std::iota(p.begin(), p.end(), 0u);
    std::shuffle(p.begin(), p.end(), g_rng);
    return p;
}

void test_dealing() {
    for (uint32_t n_sh = 1; n_sh <= 4; ++n_sh)
        for (uint64_t n : lattice(n_sh)) {
            uint64_t sum = 0;
            for (uint32_t i = 0; i < n_sh; ++i) sum += shard_rows(n, kStripe, n_sh, i);
            CHECK(sum == n, "n_sh %u n %llu: shard rows sum to %llu", n_sh, (unsigned long long)n, (unsigned long long)sum);
            std::vector<std::vector<uint8_t>> taken(n_sh);
            for (uint32_t i = 0; i < n_sh; ++i) taken[i].assign(shard_rows(n, kStripe, n_sh, i), 0);
            for (uint64_t r = 0; r < n; ++r) {
                const uint32_t i = shard_of(r, kStripe, n_sh);
                const uint64_t l = local_of(r, kStripe, n_sh);
                CHECK(i < n_sh, "n_sh %u n %llu row %llu: shard %u", n_sh, (unsigned long long)n, (unsigned long long)r, i);
                if (i >= n_sh) continue;
                CHECK(l < taken[i].size(), "n_sh %u n %llu row %llu: local %llu of %zu", n_sh, (unsigned long long)n, (unsigned long long)r,
                      (unsigned long long)l, taken[i].size());
                if (l >= taken[i].size()) continue;
                CHECK(!taken[i][l], "n_sh %u n %llu row %llu: (%u, %llu) dealt twice", n_sh, (unsigned long long)n, (unsigned long long)r, i,
                      (unsigned long long)l);
                taken[i][l] = 1;
                const int64_t back = n_sh == 1 ? global_row_id(0, 0, 1, 0, static_cast<uint32_t>(l))
                                               : global_row_id(0, kStripe, n_sh, i, static_cast<uint32_t>(l));
                CHECK(back == static_cast<int64_t>(r), "n_sh %u n %llu row %llu: global_row_id gives %lld", n_sh, (unsigned long long)n,
                      (unsigned long long)r, (long long)back);
                CHECK(global_of(l, kStripe, n_sh, i) == r, "n_sh %u n %llu row %llu: global_of", n_sh, (unsigned long long)n, (unsigned long long)r);
            }
        }
}

void check_mask(uint32_t n_sh, uint64_t n, const std::vector<uint32_t>& global, const char* what) {
    for (uint32_t i = 0; i < n_sh; ++i) {
        const uint64_t nl = shard_rows(n, kStripe, n_sh, i);
        const DealtMask m = deal_row_mask(global.data(), nl, kStripe, n_sh, i);
        CHECK(m.words.size() == (nl + 31) / 32, "%s n_sh %u n %llu shard %u: %zu words", what, n_sh, (unsigned long long)n, i, m.words.size());
        if (m.words.size() != (nl + 31) / 32) continue;
        uint64_t pop = 0;
        for (uint64_t l = 0; l < m.words.size() * 32; ++l) {
            const bool want = l < nl && bit(global, global_of(l, kStripe, n_sh, i));
            CHECK(bit(m.words, l) == want, "%s n_sh %u n %llu shard %u: local bit %llu", what, n_sh, (unsigned long long)n, i, (unsigned long long)l);
            pop += bit(m.words, l);
        }
        CHECK(m.bits == pop, "%s n_sh %u n %llu shard %u: count %llu, popcount %llu", what, n_sh, (unsigned long long)n, i,
              (unsigned long long)m.bits, (unsigned long long)pop);
    }
}
void test_mask() {
    for (uint32_t n_sh = 1; n_sh <= 4; ++n_sh)
        for (uint64_t n : lattice(n_sh)) {
            const size_t words = (n + 31) / 32;
            std::vector<uint32_t> random(words), zeros(words, 0u), ones(words, 0xffffffffu);   // (all-one: the tail bits set too)
            for (auto& w : random) w = static_cast<uint32_t>(g_rng());
            if (n % 32) random.back() |= ~((1u << (n % 32)) - 1u);                             // every bit at or beyond n
            check_mask(n_sh, n, random, "random");
            check_mask(n_sh, n, zeros, "zeros");
            check_mask(n_sh, n, ones, "ones");
        }
}

void test_tie_ranks() {
    for (uint32_t n_sh = 1; n_sh <= 4; ++n_sh)
        for (uint64_t n : lattice(n_sh)) {
            if (n == 0) continue;
            const std::vector<uint32_t> ranks = random_permutation(n);
            for (uint32_t i = 0; i < n_sh; ++i) {
                const uint64_t nl = shard_rows(n, kStripe, n_sh, i);
                std::vector<uint32_t> lrank, linv;
                local_tie_ranks(ranks.data(), nl, kStripe, n_sh, i, lrank, linv);
                CHECK(lrank.size() == nl && linv.size() == nl, "n_sh %u n %llu shard %u: sizes", n_sh, (unsigned long long)n, i);
                if (lrank.size() != nl || linv.size() != nl) continue;
                CHECK(is_permutation_of_iota(lrank.data(), nl), "n_sh %u n %llu shard %u: lrank is no permutation", n_sh, (unsigned long long)n, i);
                if (!is_permutation_of_iota(lrank.data(), nl)) continue;
                int bad_order = 0, bad_inverse = 0;
                for (uint64_t a = 0; a < nl; ++a) {
                    bad_inverse += linv[lrank[a]] != a;
                    const uint32_t ga = ranks[global_of(a, kStripe, n_sh, i)];
                    for (uint64_t b = 0; b < nl; ++b) bad_order += (ga < ranks[global_of(b, kStripe, n_sh, i)]) != (lrank[a] < lrank[b]);
                }
                CHECK(bad_order == 0, "n_sh %u n %llu shard %u: %d pairs out of order", n_sh, (unsigned long long)n, i, bad_order);
                CHECK(bad_inverse == 0, "n_sh %u n %llu shard %u: %d inverse entries wrong", n_sh, (unsigned long long)n, i, bad_inverse);
            }
        }
}

void test_pq_keys() {
    const uint64_t n = 61;
    std::vector<uint64_t> keys(n);
    for (auto& k : keys) k = g_rng() % 7 ? (g_rng() % 5) << 40 : ~0ull;   // many duplicates, some at the top of the range
    const std::vector<uint32_t> row_of_index = random_permutation(n);
    auto order_of = [&](const std::vector<uint32_t>& rank) {
        std::vector<uint32_t> order(n, 0xffffffffu);
        for (uint32_t x = 0; x < n; ++x) if (rank[x] < n) order[rank[x]] = x;
        return order;
    };
    std::vector<uint32_t> rank, key_row;
    rank_pq_keys(keys.data(), row_of_index.data(), n, rank, key_row);
    CHECK(rank.size() == n && key_row.size() == n && is_permutation_of_iota(rank.data(), n), "ranks are no permutation");
    std::vector<uint32_t> order = order_of(rank);
    for (uint64_t r = 0; r < n; ++r) {
        if (r) {
            const uint32_t a = order[r - 1], b = order[r];
            CHECK(keys[a] < keys[b] || (keys[a] == keys[b] && a < b), "rank %llu does not ascend by (key, index)", (unsigned long long)r);
        }
        CHECK(key_row[r] == row_of_index[order[r]], "key_row[%llu]", (unsigned long long)r);
    }
    rank_pq_keys(nullptr, row_of_index.data(), n, rank, key_row);            // no keys: the index order
    for (uint32_t r = 0; r < n; ++r) CHECK(rank[r] == r && key_row[r] == row_of_index[r], "null keys, index %u", r);
    rank_pq_keys(keys.data(), nullptr, n, rank, key_row);                    // no table: the key's own index
    order = order_of(rank);
    for (uint32_t r = 0; r < n; ++r) CHECK(key_row[r] == order[r], "null row_of_index, rank %u", r);
    rank_pq_keys(nullptr, nullptr, 0, rank, key_row);
    CHECK(rank.empty() && key_row.empty(), "an empty index");
}

void test_permutation_check() {
    const std::vector<uint32_t> good = random_permutation(97), repeat = {0, 2, 2, 1}, beyond = {0, 1, 4, 2};
    CHECK(is_permutation_of_iota(good.data(), good.size()), "a permutation is refused");
    CHECK(!is_permutation_of_iota(repeat.data(), repeat.size()), "a repeat is accepted");
    CHECK(!is_permutation_of_iota(beyond.data(), beyond.size()), "a value out of range is accepted");
    CHECK(is_permutation_of_iota(nullptr, 0), "the empty permutation is refused");
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
void test_pack_hits() {
    const uint32_t nq = 3, k = 3;
    const std::vector<uint32_t> counts = {0, 1, 3};
    const std::vector<int64_t> rows = {70, 71, 72, 5, 73, 74, 1ll << 40, 0, 9};
    const std::vector<float> scores = {9.f, 9.f, 9.f, 0.75f, 9.f, 9.f, 1.0f, 0.333333343f, -0.0f};
    const std::vector<float> dist = {8.f, 8.f, 8.f, 0.5f, 8.f, 8.f, 0.0f, 1.25f, 3.0f};
    for (int with_dist = 0; with_dist < 2; ++with_dist) {
        std::vector<yams_scan_hit_t> hits(nq * k);
        std::memset(hits.data(), 0x55, hits.size() * sizeof(yams_scan_hit_t));
        pack_hits(nq, k, counts.data(), rows.data(), scores.data(), with_dist ? dist.data() : nullptr, hits.data());
        for (uint32_t q = 0; q < nq; ++q)
            for (uint32_t i = 0; i < k; ++i) {
                const size_t o = q * k + i;
                if (i >= counts[q]) {
                    CHECK(hits[o].row == -1 && bits(hits[o].similarity) == 0 && bits(hits[o].distance) == 0, "form %d: unused slot %zu", with_dist, o);
                    continue;
                }
                const float want = with_dist ? dist[o] : 1.0f - scores[o];
                CHECK(hits[o].row == rows[o] && bits(hits[o].similarity) == bits(scores[o]) && bits(hits[o].distance) == bits(want),
                      "form %d: slot %zu", with_dist, o);
            }
    }
    pack_hits(0, k, nullptr, nullptr, nullptr, nullptr, nullptr);   // no queries: nothing is touched
}

void test_hex_and_chains() {
    std::vector<uint8_t> raw(32), back(32);
    for (auto& b : raw) b = static_cast<uint8_t>(g_rng());
    raw[0] = 0x00; raw[1] = 0xff; raw[2] = 0x0a; raw[3] = 0xa0;
    std::vector<char> hex(65);
    to_hex(raw.data(), hex.data());
    CHECK(std::strlen(hex.data()) == 64 && std::strspn(hex.data(), "0123456789abcdef") == 64, "to_hex: %s", hex.data());
    CHECK(parse_hex32(hex.data(), back.data()) && raw == back, "lower-case round trip");
    for (auto& c : hex) if (c >= 'a' && c <= 'f') c = static_cast<char>(c - 'a' + 'A');
    std::fill(back.begin(), back.end(), 0);
    CHECK(parse_hex32(hex.data(), back.data()) && raw == back, "upper-case round trip");
    for (auto& c : hex) if (c >= 'A' && c <= 'F') c = static_cast<char>(c - 'A' + 'a');
    const std::vector<char> short_hex(hex.begin() + 1, hex.end());          // 63 digits and the terminator: 64 bytes
    CHECK(!parse_hex32(short_hex.data(), back.data()), "63 digits are accepted");
    std::vector<char> long_hex(hex.begin(), hex.end() - 1);                  // 65 digits and the terminator
    long_hex.push_back('0'); long_hex.push_back(0);
    long_hex.shrink_to_fit();
    CHECK(!parse_hex32(long_hex.data(), back.data()), "65 digits are accepted");
    for (const char c : {'g', 'G', ' ', '-', 'x', '/', ':', '@', '`'}) {
        std::vector<char> bad = hex;
        bad[37] = c;
        CHECK(!parse_hex32(bad.data(), back.data()), "'%c' is taken for a hex digit", c);
    }
    // a lone chain up to YAMS_HASH_LONE_CHAIN_MAX bytes; beyond it, the longest chain at most 1 / YAMS_HASH_CHAIN_RATIO of the bytes
    const size_t lone = YAMS_HASH_LONE_CHAIN_MAX, big = 2 * lone;
    const std::vector<size_t> at_lone = {lone}, above_lone = {lone + 1};
    CHECK(chains_suit_the_device(at_lone.data(), 1), "a lone chain at the limit is refused");
    CHECK(!chains_suit_the_device(above_lone.data(), 1), "a lone chain above the limit is taken");
    std::vector<size_t> many(YAMS_HASH_CHAIN_RATIO, big);                    // the longest is exactly total / ratio
    CHECK(chains_suit_the_device(many.data(), many.size()), "the longest chain at total / ratio is refused");
    many.back() -= 1;                                                        // ... and one byte above it
    CHECK(!chains_suit_the_device(many.data(), many.size()), "the longest chain above total / ratio is taken");
    CHECK(chains_suit_the_device(nullptr, 0), "no chains");
}

void test_config() {
    {   // round 5: a value that merely CONTAINS another choice
        Config c("{\"shadows\":\"none\",\"note\":\"both\"}");
        int shadows = -1;
        CHECK(c.error.empty() && c.strings["shadows"] == "none", "error '%s'", c.error.c_str());
        CHECK(c.get_choice("shadows", {"both", "bf16", "i8", "none"}, 0, shadows) && shadows == 3, "shadows %d", shadows);
    }
    {   // unknown keys are skipped whatever their value
        Config c(" {\"x\":{\"a\":[1,{\"b\":null}],\"c\":\"}\"}, \"device\" : 3 ,\"y\":[1,\"two\",[ ]],\"z\":true,\"devices\":[2, 0 ,1],\"e\":[]}\n");
        long device = -1;
        CHECK(c.error.empty(), "error '%s'", c.error.c_str());
        CHECK(c.get_int("device", 0, device) && device == 3, "device %ld", device);
        CHECK(c.has("x") && c.has("y") && c.has("z") && !c.has("a") && !c.has("b") && !c.has("c"), "which keys are there");
        CHECK((c.int_lists["devices"] == std::vector<long>{2, 0, 1}) && c.int_lists.count("e") && c.int_lists["e"].empty(), "integer lists");
        long absent = 0;
        CHECK(c.get_int("search_slots", 2, absent) && absent == 2, "an absent key does not give its default");
    }
    {   // a known key of the wrong type
        Config c("{\"device\":\"0\",\"shadows\":3,\"rccl_library\":[1],\"search_slots\":2.5,\"stripe_rows\":1e3}");
        long v = 7; int ch = 7; std::string s; bool present = true;
        CHECK(c.error.empty(), "error '%s'", c.error.c_str());
        CHECK(!c.get_int("device", 0, v) && c.error == "\"device\" must be an integer", "'%s'", c.error.c_str());
        CHECK(!c.get_choice("shadows", {"both", "none"}, 0, ch) && c.error == "\"shadows\" must be a string", "'%s'", c.error.c_str());
        CHECK(!c.get_string("rccl_library", s, present) && !present && c.error == "\"rccl_library\" must be a string", "'%s'", c.error.c_str());
        CHECK(!c.get_int("search_slots", 2, v) && c.error == "\"search_slots\" must be an integer", "a float: '%s'", c.error.c_str());
        CHECK(!c.get_int("stripe_rows", 65536, v) && c.error == "\"stripe_rows\" must be an integer", "an exponent: '%s'", c.error.c_str());
    }
    for (const char* text : {"{} x", "{\"a\":1} x", "{\"a\":1}{", "{\"a\":1},"})
        CHECK(Config(text).error == "text after the configuration object", "'%s': '%s'", text, Config(text).error.c_str());
    for (const char* text : {"[1]", "7", "\"device\""})
        CHECK(Config(text).error == "the configuration is not a JSON object", "'%s': '%s'", text, Config(text).error.c_str());
    for (const char* text : {"{", "{\"a\"", "{\"a\":", "{\"a\":1", "{\"a\":1,", "{\"a\":\"b", "{\"a\":[1,", "{\"a\":{\"b\":1}", "{a:1}", "{\"a\" 1}", "{\"a\":}", "{\"a\":\"b\\"})
        CHECK(!Config(text).error.empty(), "'%s' parses", text);
    {   // nesting: a value 32 levels down is skipped, one at 33 is refused
        for (int depth : {32, 33}) {
            const std::string text = "{\"deep\":" + std::string(depth, '[') + "1" + std::string(depth, ']') + ",\"device\":1}";
            Config c(text.c_str());
            if (depth == 32) CHECK(c.error.empty() && c.has("deep") && c.ints["device"] == 1, "depth 32: '%s'", c.error.c_str());
            else CHECK(c.error == "bad array for \"deep\"", "depth 33: '%s'", c.error.c_str());
        }
    }
    for (const char* text : {static_cast<const char*>(nullptr), "", "  \n\t", "{}", " { } "}) {
        Config c(text);
        CHECK(c.error.empty() && !c.has("device"), "'%s': '%s'", text ? text : "(null)", c.error.c_str());
    }
    {   // escapes: \n and \t are translated, any other escaped character stands for itself
        Config c("{\"k\\\"ey\":\"a\\\"b\\\\c\\nd\\te\\/f\"}");
        CHECK(c.error.empty() && c.strings["k\"ey"] == "a\"b\\c\nd\te/f", "'%s' / '%s'", c.error.c_str(), c.strings["k\"ey"].c_str());
    }
    {   // an enumerated value that is not listed: refused, and the error names the list
        Config c("{\"shadows\":\"bth\"}");
        int shadows = -1;
        CHECK(!c.get_choice("shadows", {"both", "bf16", "i8", "none"}, 0, shadows), "\"bth\" is taken");
        CHECK(c.error == "\"shadows\": \"bth\" is not one of \"both\" \"bf16\" \"i8\" \"none\"", "'%s'", c.error.c_str());
        CHECK(shadows == 0, "the default is not left in place: %d", shadows);
    }
}

// ---- HandleTable: the registry of a handle family -------------------------------------------------------------------------------
struct Thing {                   // an entry as the door keeps them: its own mutex, a payload that its taker destroys under it
    std::mutex mu;
    int* payload;
    std::atomic<int>* destroyed; // how often this entry's payload was destroyed
    Thing(int v, std::atomic<int>* d) : payload(new int(v)), destroyed(d) {}
    ~Thing() { delete payload; } // (an entry that was never destroyed still gives its payload back: the test leaks nothing)
    void destroy() { if (payload) { delete payload; payload = nullptr; ++*destroyed; } }
};

void test_handle_table() {
    std::atomic<int> destroyed{0};
    HandleTable<Thing> t;
    CHECK(t.size() == 0 && !t.find(0) && !t.find(1) && !t.take(1), "an empty table knows an id");
    const uint64_t a = t.insert(std::make_shared<Thing>(10, &destroyed)), b = t.insert(std::make_shared<Thing>(20, &destroyed)),
                   c = t.insert(std::make_shared<Thing>(30, &destroyed));
    CHECK(a == 1 && b == 2 && c == 3 && t.size() == 3, "ids %llu %llu %llu", (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
    CHECK(t.find(b) && *t.find(b)->payload == 20 && !t.find(4) && !t.find(0) && !t.take(4) && !t.take(~0ull), "find / take of unknown ids");
    {   // a call that found the entry before the destroy: the entry outlives take(), its payload reads as destroyed
        const std::shared_ptr<Thing> held = t.find(b);
        const std::shared_ptr<Thing> taken = t.take(b);
        CHECK(taken && taken == held, "take() does not hand out the entry find() found");
        CHECK(!t.find(b) && !t.take(b) && t.size() == 2, "a taken id is still known");
        { std::lock_guard<std::mutex> lk(taken->mu); taken->destroy(); }
        std::lock_guard<std::mutex> lk(held->mu);
        CHECK(held->payload == nullptr && destroyed == 1, "the holder does not see the destroy");
    }
    const uint64_t d = t.insert(std::make_shared<Thing>(40, &destroyed));
    CHECK(d == 4, "the id of a taken entry is reused: %llu", (unsigned long long)d);
    std::vector<int> seen;
    t.visit([&](const Thing& e) { seen.push_back(*e.payload); });
    CHECK((seen == std::vector<int>{10, 30, 40}), "visit() walks %zu entries", seen.size());
    seen.clear();
    t.drain([&](Thing& e) { seen.push_back(*e.payload); e.destroy(); });
    CHECK((seen == std::vector<int>{10, 30, 40}) && destroyed == 4, "drain() visits every entry once: %zu visits, %d destroyed", seen.size(), destroyed.load());
    CHECK(t.size() == 0 && !t.find(a) && !t.find(c) && !t.find(d), "the table is not empty after drain()");
    t.drain([&](Thing&) { CHECK(false, "a drained table still holds an entry"); });
    const uint64_t e = t.insert(std::make_shared<Thing>(50, &destroyed));      // ids go on across a shutdown and a fresh init
    CHECK(e == 5 && *t.find(e)->payload == 50, "after drain() the ids start again: %llu", (unsigned long long)e);
}

// Eight threads on one table: insert, find-and-use, take-and-destroy, mixed; then the teardown walk.  Every entry that was ever
// inserted has been destroyed exactly once at the end — by the thread that took it or by drain() — and no use of a found entry
// touched a payload outside its mutex.
int run_threads() {
    constexpr int kThreads = 8, kOps = 4000;
    std::vector<std::atomic<int>> destroyed(kThreads * kOps);
    for (auto& d : destroyed) d = 0;
    std::atomic<uint64_t> inserted{0}, high{0};
    HandleTable<Thing> t;
    std::vector<std::thread> threads;
    for (int w = 0; w < kThreads; ++w)
        threads.emplace_back([&, w] {
            std::mt19937_64 rng(1000 + w);
            for (int op = 0; op < kOps; ++op) {
                const uint64_t known = high.load();
                const uint64_t id = known ? 1 + rng() % known : 1;
                switch (rng() % 4) {
                    case 0: {
                        const uint64_t slot = inserted++;
                        const uint64_t got = t.insert(std::make_shared<Thing>(static_cast<int>(slot), &destroyed[slot]));
                        uint64_t h = high.load();
                        while (h < got && !high.compare_exchange_weak(h, got)) {}
                        break;
                    }
                    case 1: case 2:
                        if (const std::shared_ptr<Thing> e = t.find(id)) {
                            std::lock_guard<std::mutex> lk(e->mu);
                            if (e->payload) CHECK(*e->payload >= 0, "a live payload reads %d", *e->payload);
                        }
                        break;
                    default:
                        if (const std::shared_ptr<Thing> e = t.take(id)) {
                            std::lock_guard<std::mutex> lk(e->mu);
                            e->destroy();
                        }
                }
            }
        });
    for (auto& th : threads) th.join();
    CHECK(high.load() == inserted.load(), "%llu ids for %llu entries", (unsigned long long)high.load(), (unsigned long long)inserted.load());
    t.drain([](Thing& e) { e.destroy(); });
    CHECK(t.size() == 0, "entries after drain()");
    int wrong = 0;
    for (uint64_t i = 0; i < inserted; ++i) wrong += destroyed[i] != 1;
    CHECK(wrong == 0 && inserted > 0, "%d of %llu entries were not destroyed exactly once", wrong, (unsigned long long)inserted.load());
    if (g_failures == 0) std::printf("threads OK (0 failures, %llu entries)\n", (unsigned long long)inserted.load());
    else std::printf("%d FAILURES\n", g_failures);
    return g_failures == 0 ? 0 : 1;
}

// ---- OwnedArrays and HitResult: what a door hands to its caller ------------------------------------------------------------------
// Under AddressSanitizer an array that is neither committed nor freed is a leak that fails the run at exit, a freed one that
// is handed out fails at the write below.
void test_owned_arrays() {
    for (int commit = 0; commit < 2; ++commit)
        for (int wanted = 0; wanted < 8; ++wanted) {      // one mandatory array and three optional ones, wanted or not
            const bool w1 = wanted & 1, w2 = wanted & 2, w3 = wanted & 4;
            uint32_t* const before32 = reinterpret_cast<uint32_t*>(0x10); double* const before64 = reinterpret_cast<double*>(0x20);
            uint32_t* o0 = before32; double* o1 = before64; double* o2 = before64; uint32_t* o3 = before32;
            {
                OwnedArrays res;
                uint32_t* a0 = res.add(&o0, 5);
                double* a1 = res.add(&o1, 3, w1);
                double* a2 = res.add(w2 ? &o2 : nullptr, 7, w2);      // an optional out parameter that is not there
                uint32_t* a3 = res.add(&o3, 0, w3);                   // no elements: an array all the same
                CHECK(res.ok() && a0 && (a1 != nullptr) == w1 && (a2 != nullptr) == w2 && (a3 != nullptr) == w3, "wanted %d: what add() returns", wanted);
                CHECK(o0 == before32 && o1 == before64 && o2 == before64 && o3 == before32, "wanted %d: add() writes an out parameter", wanted);
                for (int i = 0; i < 5; ++i) a0[i] = 7;
                if (a1) a1[2] = 1.5;
                if (a2) a2[6] = 2.5;
                if (commit) {
                    CHECK(res.commit() == YAMS_OK, "commit()");
                    CHECK(o0 == a0 && o1 == a1 && o3 == a3 && o2 == (w2 ? a2 : before64), "wanted %d: what commit() hands out", wanted);
                }
            }
            if (commit) {      // the caller's now, intact behind the helper's back: freed as the vtable's free function does
                CHECK(o0[4] == 7 && (!w1 || o1[2] == 1.5) && (!w2 || o2[6] == 2.5), "wanted %d: a committed array changed", wanted);
                CHECK((o1 != nullptr) == w1 && (o3 != nullptr) == w3, "wanted %d: an unwanted array is handed out", wanted);
                std::free(o0); std::free(o1); std::free(o3);
                if (w2) std::free(o2);
            } else CHECK(o0 == before32 && o1 == before64 && o2 == before64 && o3 == before32, "wanted %d: an uncommitted helper wrote an out parameter", wanted);
        }
    {   // an allocation that cannot be had (SIZE_MAX / 2 elements of 8 bytes: beyond size_t): not ok, nothing handed out, and
        // the arrays that were had go with the helper
        uint32_t* o0 = nullptr; uint64_t* o1 = reinterpret_cast<uint64_t*>(0x30); float* o2 = nullptr;
        OwnedArrays res;
        uint32_t* a0 = res.add(&o0, 16);
        uint64_t* a1 = res.add(&o1, SIZE_MAX / 2);
        float* a2 = res.add(&o2, 4);
        CHECK(!res.ok() && a0 && !a1 && a2, "the impossible allocation");
        CHECK(o0 == nullptr && o1 == reinterpret_cast<uint64_t*>(0x30) && o2 == nullptr, "a failed helper wrote an out parameter");
    }
}

void test_hit_result() {
    for (uint32_t nq : {0u, 1u, 3u})
        for (uint32_t k : {0u, 1u, 4u}) {
            yams_scan_hit_t* hits = nullptr; uint32_t* counts = nullptr;
            size_t slots;
            {
                HitResult res(nq, k);
                slots = res.slots;
                CHECK(res.ok() && res.slots == static_cast<size_t>(nq) * (k ? k : 1), "nq %u k %u: %zu slots", nq, k, res.slots);
                if ((nq + k) % 2) continue;      // not committed: both arrays go with the object
                CHECK(res.commit(&hits, &counts) == YAMS_OK && hits && counts && !res.hits && !res.counts, "nq %u k %u: commit", nq, k);
            }
            for (size_t o = 0; o < slots; ++o)
                CHECK(hits[o].row == -1 && bits(hits[o].similarity) == 0 && bits(hits[o].distance) == 0, "nq %u k %u: slot %zu is not preset", nq, k, o);
            for (uint32_t q = 0; q < (nq ? nq : 1); ++q) CHECK(counts[q] == 0, "nq %u k %u: count %u is not zero", nq, k, q);
            std::free(hits); std::free(counts);
        }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--threads") == 0) return run_threads();
    test_dealing();
    test_mask();
    test_tie_ranks();
    test_pq_keys();
    test_permutation_check();
    test_pack_hits();
    test_hex_and_chains();
    test_config();
    test_handle_table();
    test_owned_arrays();
    test_hit_result();
    if (g_failures == 0) std::printf("OK (0 failures)\n");
    else std::printf("%d FAILURES\n", g_failures);
    return g_failures == 0 ? 0 : 1;
}
