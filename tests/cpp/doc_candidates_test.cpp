// doc_candidates_test.cpp — AccelExactScanBackend::searchDocumentCandidatesWithDiagnostics (the device route:
// vector_doc_scan_v1) equals the all-rows route it replaces, bestRecordPerDocument(searchAllExactCandidateRows...):
// chunk ids, score bits, order and the four diagnostics fields, over inserts, upserts, deletes that compact the mirror,
// a rolled-back transaction, chunk ids that do not ascend with the rows and rows without a document hash.
// Built against the reference's own headers (-DYAMS_ACCEL_USE_HOST_TYPES), driven by tests/test_doc_candidates_cpp_gpu.py.
#include <yams/vector/vector_store.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "yams_accel/exact_scan_backend.hpp"

using namespace yams;
static int failures = 0, comparisons = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static std::vector<float> gauss(std::mt19937& rng, size_t dim) {
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> v(dim);
    for (auto& x : v) x = nd(rng);
    return v;
}

static void compare(vector::IVectorStore* backend, const std::vector<float>& q, size_t k, float thr,
                    const std::unordered_set<std::string>& cand, bool collect) {
    auto* docs = dynamic_cast<vector::IDocumentCandidateVectorStore*>(backend);
    auto* all = dynamic_cast<vector::IAllExactCandidateVectorStore*>(backend);
    vector::VectorSearchDiagnostics dNew, dOld;
    dNew.collectVisitedDocumentHashes = dOld.collectVisitedDocumentHashes = collect;
    auto got = docs->searchDocumentCandidatesWithDiagnostics(q, k, thr, cand, dNew);
    auto rows = all->searchAllExactCandidateRowsWithDiagnostics(q, thr, cand, dOld);
    ++comparisons;
    CHECK(got.has_value() == rows.has_value());
    if (!got.has_value() || !rows.has_value()) return;
    auto want = vector::AccelExactScanBackend::bestRecordPerDocument(std::move(rows.value()), k);
    CHECK(got.value().size() == want.size());
    for (size_t i = 0; i < std::min(got.value().size(), want.size()); ++i) {
        const auto& a = got.value()[i]; const auto& b = want[i];
        uint32_t ba, bb; std::memcpy(&ba, &a.relevance_score, 4); std::memcpy(&bb, &b.relevance_score, 4);
        if (a.chunk_id != b.chunk_id || ba != bb) {
            std::printf("  rank %zu: %s %08x vs %s %08x\n", i, a.chunk_id.c_str(), ba, b.chunk_id.c_str(), bb);
            ++failures;
            break;
        }
    }
    CHECK(dNew.rowsVisited == dOld.rowsVisited);
    CHECK(dNew.exactDistanceEvaluations == dOld.exactDistanceEvaluations);
    CHECK(dNew.returnedRows == dOld.returnedRows);
    CHECK(dNew.usedExactScan == dOld.usedExactScan);
    CHECK(dNew.visitedDocumentHashes == dOld.visitedDocumentHashes);
}

int main(int argc, char** argv) {
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    if (argc < 2) { std::printf("usage: %s <plugin.so>\n", argv[0]); return 2; }
    auto loaded = accel::Plugin::load(argv[1], "{\"device\":0}");
    if (!loaded.has_value()) { std::printf("plugin load failed\n"); return 1; }
    auto plugin = loaded.value();
    std::unique_ptr<vector::IVectorStore> backend = vector::createAccelExactScanBackend(plugin);
    CHECK(backend->initialize(":memory:").has_value() && backend->createTables(384).has_value());
    const size_t dim = 384, nDocs = 700;
    std::mt19937 rng(7);
    std::uniform_int_distribution<size_t> pickDoc(0, nDocs - 1);
    auto docName = [](size_t d) { char b[32]; std::snprintf(b, sizeof b, "%08zx", (d * 2654435761u) & 0xffffffffu); return std::string(b); };
    auto chunkName = [](size_t i) { char b[32]; std::snprintf(b, sizeof b, "c%07zu", (i * 7919u) % 1000003u); return std::string(b); };
    std::vector<vector::VectorRecord> recs;
    for (size_t i = 0; i < 6000; ++i) {   // documents' chunks appended together, chunk ids out of row order
        const size_t d = i / 9;
        vector::VectorRecord r(chunkName(i), i % 97 == 5 ? std::string() : docName(d), gauss(rng, dim), "x");
        if (i % 50 == 0 && i) r.embedding = recs[i - 3].embedding;          // equal scores within / across documents
        recs.push_back(std::move(r));
    }
    for (size_t i = 0; i < 40; ++i) recs[100 + i].embedding.assign(dim, 0.f);   // zero rows
    CHECK(backend->insertVectorsBatch(recs).has_value());
    std::vector<std::vector<float>> queries;
    for (int i = 0; i < 3; ++i) queries.push_back(gauss(rng, dim));
    queries.push_back(recs[50].embedding);
    auto candidates = [&](size_t n) {
        std::unordered_set<std::string> c;
        while (c.size() < n) c.insert(docName(pickDoc(rng)));
        c.insert(std::string());                  // rows without a document: scored, counted, never returned
        c.insert("not-a-document");
        return c;
    };
    auto round = [&](const char* what) {
        std::printf("[round] %s\n", what);
        for (const auto& q : queries)
            for (size_t nc : {3u, 60u, 400u}) {
                const auto c = candidates(nc);
                compare(backend.get(), q, 10, -1.0f, c, nc == 3);
                compare(backend.get(), q, 1, 0.02f, c, true);
                compare(backend.get(), q, 0, -1.0f, c, false);
                compare(backend.get(), q, 2000, -1.0f, c, false);
            }
    };
    round("insert");
    // upserts (a chunk id written again: the old row becomes a tombstone) and new documents
    std::vector<vector::VectorRecord> up;
    for (size_t i = 0; i < 300; ++i) { vector::VectorRecord r = recs[i * 13]; r.embedding = gauss(rng, dim); up.push_back(r); }
    for (size_t i = 0; i < 200; ++i) up.emplace_back(chunkName(6000 + i), docName(pickDoc(rng)), gauss(rng, dim), "y");
    CHECK(backend->insertVectorsBatch(up).has_value());
    round("upsert");
    // deletes that trigger the compaction of the mirror (> 1024 tombstones and > a quarter of the rows)
    for (size_t i = 0; i < 2100; ++i) (void)backend->deleteVector(recs[(i * 17) % 6000].chunk_id);
    round("delete + compaction");
    // a rolled-back transaction leaves the committed state
    CHECK(backend->beginTransaction().has_value());
    for (size_t i = 0; i < 50; ++i) (void)backend->insertVector(vector::VectorRecord(chunkName(9000 + i), docName(1), gauss(rng, dim), "z"));
    (void)backend->deleteVector(recs[1].chunk_id);
    CHECK(backend->rollbackTransaction().has_value());
    round("rollback");
    // an invalid query fails both routes the same way
    compare(backend.get(), std::vector<float>(dim, 0.f), 10, -1.0f, candidates(5), false);
    std::printf("%s (%d failures, %d comparisons)\n", failures ? "FAILED" : "OK", failures, comparisons);
    return failures ? 1 : 0;
}
