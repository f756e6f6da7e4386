// entity_index_test.cpp — AccelEntityIndex (include/yams_accel/entity_index.hpp, standalone types) against a host loop that
// restates searchEntities (sqlite_vec_backend.cpp:2801-2887) with computeCosineSimilarity's arithmetic
// (vector_database.cpp:1786-1810) and the served order rule (similarity desc, table order): inserts over two dimensions,
// INSERT OR REPLACE, deletes by node and by document, a compaction, every filter, a filter string never interned (no device
// call), k above YAMS_SCAN_MAX_K (rounds), zero queries and zero rows.  Driven by tests/test_entity_gpu.py;
// `--expect-no-gpu`: the plugin refuses to initialise and the adapter is never built (the CPU suite).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "yams_accel/entity_index.hpp"

using namespace yams;
using vector::EntityEmbeddingType;
using vector::EntitySearchParams;
using vector::EntityVectorRecord;

static int failures = 0, comparisons = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static float cosine(const std::vector<float>& a, const std::vector<float>& b) {
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (size_t i = 0; i < a.size(); ++i) {
        dot += static_cast<double>(a[i]) * static_cast<double>(b[i]);
        na += static_cast<double>(a[i]) * static_cast<double>(a[i]);
        nb += static_cast<double>(b[i]) * static_cast<double>(b[i]);
    }
    na = std::sqrt(na); nb = std::sqrt(nb);
    if (na == 0.0 || nb == 0.0) return 0.0f;
    return static_cast<float>(dot / (na * nb));
}

// the table as the reference keeps it: rows in rowid order, INSERT OR REPLACE moves a row to the end
struct HostTable {
    std::vector<EntityVectorRecord> rows;
    void insert(const EntityVectorRecord& r) {
        for (size_t i = 0; i < rows.size(); ++i)
            if (rows[i].node_key == r.node_key && rows[i].embedding_type == r.embedding_type) { rows.erase(rows.begin() + i); break; }
        rows.push_back(r);
    }
    template <typename P> void erase(P p) { rows.erase(std::remove_if(rows.begin(), rows.end(), p), rows.end()); }
    std::vector<EntityVectorRecord> search(const std::vector<float>& q, const EntitySearchParams& p) const {
        std::vector<EntityVectorRecord> kept;
        if (q.empty()) return kept;
        for (const auto& r : rows) {
            if (p.embedding_type && r.embedding_type != *p.embedding_type) continue;
            if (p.node_type && r.node_type != *p.node_type) continue;
            if (p.document_hash && r.document_hash != *p.document_hash) continue;
            if (r.embedding.size() != q.size()) continue;
            const float s = cosine(q, r.embedding);
            if (s >= p.similarity_threshold) { kept.push_back(r); kept.back().relevance_score = s; }
        }
        std::stable_sort(kept.begin(), kept.end(), [](const EntityVectorRecord& a, const EntityVectorRecord& b) { return a.relevance_score > b.relevance_score; });
        if (kept.size() > p.k) kept.resize(p.k);
        return kept;
    }
};

static void compare(vector::AccelEntityIndex& idx, const HostTable& t, const std::vector<float>& q, const EntitySearchParams& p) {
    ++comparisons;
    auto got = idx.searchEntities(q, p);
    CHECK(got.has_value());
    if (!got.has_value()) { std::printf("  error: %s\n", got.error().message.c_str()); return; }
    const auto want = t.search(q, p);
    CHECK(got.value().size() == want.size());
    for (size_t i = 0; i < std::min(got.value().size(), want.size()); ++i) {
        const auto& a = got.value()[i]; const auto& b = want[i];
        uint32_t ba, bb; std::memcpy(&ba, &a.relevance_score, 4); std::memcpy(&bb, &b.relevance_score, 4);
        if (a.node_key != b.node_key || a.embedding_type != b.embedding_type || ba != bb || a.content != b.content ||
            a.embedding.size() != (p.include_embeddings ? b.embedding.size() : 0u)) {
            std::printf("  rank %zu: %s %08x vs %s %08x\n", i, a.node_key.c_str(), ba, b.node_key.c_str(), bb);
            ++failures;
            break;
        }
    }
}

int main(int argc, char** argv) {
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    if (argc < 2) { std::printf("usage: %s <plugin.so> [--expect-no-gpu]\n", argv[0]); return 2; }
    const bool expectNoGpu = argc > 2 && std::strcmp(argv[2], "--expect-no-gpu") == 0;
    auto loaded = accel::Plugin::load(argv[1], "{\"device\":0}");
    if (expectNoGpu) {   // no device: the plugin refuses to initialise, nothing falls back
        CHECK(!loaded.has_value());
        if (!loaded.has_value()) CHECK(loaded.error().code == ErrorCode::NotInitialized);
        std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
        return failures ? 1 : 0;
    }
    if (!loaded.has_value()) { std::printf("plugin load failed: %s\n", loaded.error().message.c_str()); return 1; }
    auto made = vector::createAccelEntityIndex(loaded.value());
    if (!made.has_value()) { std::printf("no entity interface: %s\n", made.error().message.c_str()); return 1; }
    vector::AccelEntityIndex& idx = *made.value();
    HostTable t;
    std::mt19937 rng(7);
    std::normal_distribution<float> nd(0.f, 1.f);
    auto gauss = [&](size_t dim) { std::vector<float> v(dim); for (auto& x : v) x = nd(rng); return v; };
    const char* nodeTypes[] = {"function", "class", "method", ""};
    auto record = [&](int i, size_t dim) {
        EntityVectorRecord r;
        r.node_key = "node" + std::to_string(i / 2);               // two embedding types per node
        r.embedding_type = static_cast<EntityEmbeddingType>((i % 2) * 2 + (i / 2) % 2);
        r.embedding = gauss(dim);
        r.content = "content " + std::to_string(i);
        r.node_type = nodeTypes[(i / 2) % 4];
        r.document_hash = "doc" + std::to_string(i / 40);
        return r;
    };
    auto put = [&](const EntityVectorRecord& r) { CHECK(idx.insertEntityVector(r).has_value()); t.insert(r); };

    // an empty index: empty results, filters or not
    EntitySearchParams p; p.similarity_threshold = -1.0f;
    compare(idx, t, gauss(64), p);
    p.embedding_type = EntityEmbeddingType::ALIAS; compare(idx, t, gauss(64), p); p.embedding_type.reset();

    for (int i = 0; i < 6000; ++i) put(record(i, i % 7 == 3 ? 32 : 64));
    {   // duplicates (ties), a zero row, a row that scores -0.0f against e0
        auto r = record(100000, 64); r.embedding = t.rows[10].embedding; put(r);
        r = record(100002, 64); r.embedding = t.rows[10].embedding; put(r);
        r = record(100004, 64); r.embedding.assign(64, 0.f); put(r);
        r = record(100006, 64); r.embedding.assign(64, 0.f); r.embedding[0] = -1e-40f; r.embedding[1] = 1e6f; put(r);
    }
    CHECK(idx.getEntityVectorCount().value() == t.rows.size());
    std::vector<float> e0(64, 0.f); e0[0] = 1.f;
    const std::vector<std::vector<float>> queries = {gauss(64), gauss(32), t.rows[10].embedding, std::vector<float>(64, 0.f), e0, gauss(48)};
    auto sweep = [&]() {
        for (const auto& q : queries) {
            for (float thr : {-1.0f, 0.0f, 0.1f}) {
                EntitySearchParams s; s.similarity_threshold = thr; s.k = 25;
                compare(idx, t, q, s);
                s.embedding_type = EntityEmbeddingType::ALIAS; compare(idx, t, q, s);
                s.node_type = "class"; compare(idx, t, q, s);
                s.embedding_type.reset(); s.document_hash = "doc3"; compare(idx, t, q, s);
                s.node_type.reset(); s.include_embeddings = true; compare(idx, t, q, s);
                s.document_hash = "doc17"; s.node_type = ""; compare(idx, t, q, s);        // the empty string is a value
            }
        }
    };
    sweep();
    {   // a filter string never interned: empty, and no device call
        const uint64_t before = idx.deviceCalls();
        EntitySearchParams s; s.similarity_threshold = -1.0f; s.node_type = "no such type";
        compare(idx, t, queries[0], s);
        s.node_type.reset(); s.document_hash = "no such document"; compare(idx, t, queries[0], s);
        CHECK(idx.deviceCalls() == before);
    }
    {   // k above YAMS_SCAN_MAX_K: rounds behind the mask
        EntitySearchParams s; s.similarity_threshold = -1.0f; s.k = 2500;
        const uint64_t before = idx.deviceCalls();
        compare(idx, t, queries[0], s);
        CHECK(idx.deviceCalls() == before + 3);
        s.k = 100000; compare(idx, t, queries[2], s);                                      // k > rows
        s.embedding_type = EntityEmbeddingType::CONTEXT; s.k = 1025; compare(idx, t, queries[0], s);
    }
    // INSERT OR REPLACE: the new value takes a fresh rowid at the end (ties move with it); another dimension moves corpora
    for (int i = 0; i < 300; i += 3) put(record(i, 64));
    { auto r = record(20, 64); r.embedding = t.rows[10].embedding; put(r); }
    for (int i = 1; i < 100; i += 10) put(record(i, 32));
    sweep();
    // deletes: by node (both embedding types), by document
    for (int i = 200; i < 260; ++i) {
        CHECK(idx.deleteEntityVectorsByNode("node" + std::to_string(i)).has_value());
        t.erase([&](const EntityVectorRecord& r) { return r.node_key == "node" + std::to_string(i); });
    }
    CHECK(idx.deleteEntityVectorsByDocument("doc3").has_value());
    t.erase([](const EntityVectorRecord& r) { return r.document_hash == "doc3"; });
    CHECK(!idx.hasEntityEmbedding("node210").value() && idx.hasEntityEmbedding("node1").value());
    CHECK(idx.getEntityVectorCount().value() == t.rows.size());
    sweep();
    // enough tombstones for a compaction (corpus_clear + re-append), then inserts after it
    for (int d = 20; d < 90; ++d) {
        CHECK(idx.deleteEntityVectorsByDocument("doc" + std::to_string(d)).has_value());
        t.erase([&](const EntityVectorRecord& r) { return r.document_hash == "doc" + std::to_string(d); });
    }
    sweep();
    for (int i = 7000; i < 7200; ++i) put(record(i, 64));
    sweep();
    CHECK(idx.getEntityVectorCount().value() == t.rows.size());
    CHECK(idx.getEntityVectorsByNode("node1").value().size() == 2);
    std::printf("%s (%d failures, %d comparisons)\n", failures ? "FAILED" : "OK", failures, comparisons);
    return failures ? 1 : 0;
}
