// mirror_model_test.cpp — model-based CRUD stress of the stateful mirror: AccelVectorIndex / AccelVectorTable
// (include/yams_accel/vector_index.hpp) over the plugin's vector_scan_v1 / vector_doc_scan_v1 corpus.  One seeded stream of
// inserts / replacements / deletes / updates with searches of every kind in between (tests/cpp/mirror_model.hpp) is replayed
// into the host model and into a backend, and EVERY search is compared, all of it: size, chunk ids in order, relevance_score
// bits and the diagnostics counters the reference defines for that kind of search.  No tolerance, no skipped search.
//
//   mirror_model_test <plugin.so> --config '<json>' --seed S [--ops N]     the adapter on the device
//   mirror_model_test --dry-run --seed S [--ops N]                          generator + model alone: the coverage counters
//   mirror_model_test --model-only <libyams_scan_ref.so> --seed S           the model against the reference-compiled table
//                                                                           (phases A and D; cosine and vec0 searches)
//   mirror_model_test <plugin.so> --expect-no-gpu                           the plugin refuses to initialise
//   --only-scripted: the three scripted cases alone.
// Phases: A AccelVectorTable over dims 8 / 32 / 48; B AccelVectorIndex dim 256, cosine, grown past 20 000 rows in ragged
// batches, shrunk through compactions, grown again past 4096 and 16 384; C the same index with a PQ index set ONCE; D
// AccelVectorIndex(Vec0L2) dim 64 with fp64 accumulation.  --ops N scales the number of searches per phase (default 100 =
// the committed size), never what is compared.
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "mirror_model.hpp"
#include "yams_accel/vector_index.hpp"

using namespace yams;
namespace mm = mirror_model;
static_assert(mm::kScanMaxK == YAMS_SCAN_MAX_K, "the model restates YAMS_SCAN_MAX_K");

struct Outcome {                      // what one search returned: per query, plus the counters of the call
    std::vector<mm::Answer> per;
    bool counters = false;
    uint64_t visited = 0, evaluated = 0, returned = 0;
    bool notImplemented = false;      // ErrorCode::NotImplemented (a striped corpus: PQ and document searches)
    bool unsupported = false;         // this backend cannot run the search at all (the reference leg: PQ, documents)
    std::string error;                // any other error
};

struct Counters {
    uint64_t compared = 0, failures = 0, skipped = 0, mutations = 0, replacements = 0, repeatedBatches = 0, crossDimRepeats = 0, tieSearches = 0,
             docRestriction = 0, metaPath = 0, allMatching = 0, bigK = 0, searchDocuments = 0, pq = 0, pqWithCandidates = 0, emptyIndex = 0,
             compactionsB = 0, compactionsC = 0, bigBatchB = 0, notImplemented = 0, unpinned = 0, invalidQueries = 0, batches = 0, maxLive = 0,
             notFound = 0, l2 = 0, layoutRemeasures = 0, compactionsOther = 0;
};

// ---- backends -------------------------------------------------------------------------------------------------------------
struct Backend {
    virtual ~Backend() = default;
    virtual bool striped() const { return false; }
    virtual std::string mutate(const mm::Op& op, const std::vector<mm::Change>& log, bool found) = 0;   // "" or what went wrong
    virtual Outcome search(const mm::Op& op, const mm::HostModel& model) = 0;
    virtual long mirrorRows() const { return -1; }
};

struct NullBackend : Backend {          // --dry-run: nothing to compare with
    std::string mutate(const mm::Op&, const std::vector<mm::Change>&, bool) override { return {}; }
    Outcome search(const mm::Op&, const mm::HostModel&) override { Outcome o; o.unsupported = true; return o; }
};

static vector::VectorRecord toRecord(const mm::Rec& r) {
    vector::VectorRecord v;
    v.chunk_id = r.chunk_id; v.document_hash = r.document_hash; v.embedding = r.embedding; v.metadata = r.metadata;
    v.content = "content of " + r.chunk_id;
    return v;
}

struct AdapterBackend : Backend {
    std::shared_ptr<accel::Plugin> plugin;
    bool isStriped = false;
    std::unique_ptr<vector::AccelVectorTable> table;
    std::unique_ptr<vector::AccelVectorIndex> index;
    AdapterBackend(std::shared_ptr<accel::Plugin> p, bool stripedCorpus) : plugin(std::move(p)), isStriped(stripedCorpus) {}
    bool striped() const override { return isStriped; }
    long mirrorRows() const override { return index ? static_cast<long>(index->mirrorRows()) : -1; }

    std::string mutate(const mm::Op& op, const std::vector<mm::Change>&, bool found) override {
        auto status = [&](const Result<void>& r, bool wantOk) -> std::string {
            if (r.has_value() == wantOk) {
                if (!wantOk && r.error().code != ErrorCode::NotFound) return "expected NotFound, got: " + r.error().message;
                return {};
            }
            return wantOk ? "failed: " + r.error().message : "succeeded where the table holds no such row";
        };
        std::vector<vector::VectorRecord> recs;
        for (const auto& r : op.recs) recs.push_back(toRecord(r));
        switch (op.kind) {
            case mm::Op::Insert: return status(table ? table->insertVectorsBatch(recs) : index->insertVectorsBatch(recs), true);
            case mm::Op::Erase: return status(table ? table->deleteVector(op.id) : index->deleteVector(op.id), found);
            case mm::Op::EraseDocument: return status(table ? table->deleteVectorsByDocument(op.id) : index->deleteVectorsByDocument(op.id), true);
            case mm::Op::Update:
                if (table) {   // (the table has no updateVector: its host replaces through getVector + insert)
                    const bool there = table->getVector(op.id).value().has_value();
                    if (there != found) return "getVector disagrees with the table";
                    return there ? status(table->insertVectorsBatch(recs), true) : std::string();
                }
                return status(index->updateVector(op.id, recs[0]), found);
            case mm::Op::SetPq: {
                auto r = table ? table->setPqIndex(op.dim, op.codes, op.m, op.pqIds) : index->setPqIndex(op.codes, op.m, op.pqIds);
                if (isStriped) return !r.has_value() && r.error().code == ErrorCode::NotImplemented ? std::string() : "a striped corpus must answer NotImplemented";
                return status(r, true);
            }
            default: return "not a mutation";
        }
    }
    static mm::Answer toAnswer(const std::vector<vector::VectorRecord>& recs, const mm::HostModel& model, std::string& err) {
        mm::Answer a;
        for (const auto& r : recs) {
            a.hits.push_back({r.chunk_id, mm::bitsOf(r.relevance_score)});
            const mm::Row* row = model.find(r.chunk_id);   // the record that comes back is the row's own (content of a replaced row, ...)
            if (row && (r.document_hash != row->document_hash || r.embedding != row->embedding || r.metadata != row->metadata) && err.empty())
                err = "record of " + r.chunk_id + " does not carry the table's current content";
        }
        return a;
    }
    Outcome search(const mm::Op& op, const mm::HostModel& model) override {
        Outcome o;
        vector::VectorSearchDiagnostics dg;
        const std::unordered_set<std::string> cands(op.cands.begin(), op.cands.end());
        auto fail = [&](const Error& e) {
            if (e.code == ErrorCode::NotImplemented) o.notImplemented = true;
            else if (e.code == ErrorCode::InvalidArgument) { o.per.assign(op.queries.size(), mm::Answer{}); for (auto& a : o.per) a.invalid = true; }
            else o.error = e.message;
        };
        auto counters = [&] { o.counters = true; o.visited = dg.rowsVisited; o.evaluated = dg.exactDistanceEvaluations; o.returned = dg.returnedRows; };
        switch (op.kind) {
            case mm::Op::Search: {
                Result<std::vector<vector::VectorRecord>> r = std::vector<vector::VectorRecord>{};
                const bool plain = !op.doc && op.cands.empty() && op.meta.empty() && !op.all;
                if (table) r = op.all ? table->searchSimilarRows(op.queries[0], op.k, op.thr, cands, &dg, vector::ExactRowSelection::AllMatching)
                                      : table->searchSimilar(op.queries[0], op.k, op.thr, op.doc, cands, op.meta, &dg);
                else r = plain ? index->searchSimilar(op.queries[0], op.k, op.thr, &dg)
                               : index->searchSimilar(op.queries[0], op.k, op.thr, op.doc, cands, op.meta, &dg,
                                                      op.all ? vector::ExactRowSelection::AllMatching : vector::ExactRowSelection::TopK);
                if (!r) { fail(r.error()); return o; }
                o.per.push_back(toAnswer(r.value(), model, o.error));
                counters();
                return o;
            }
            case mm::Op::SearchBatch: {
                auto r = table ? table->searchSimilarBatch(op.queries, op.k, op.thr) : index->searchSimilarBatch(op.queries, op.k, op.thr);
                if (!r) { fail(r.error()); return o; }
                for (const auto& one : r.value()) o.per.push_back(toAnswer(one, model, o.error));
                return o;
            }
            case mm::Op::SearchDocuments: {
                auto r = table ? table->searchDocuments(op.queries[0], op.k, op.thr, cands, &dg) : index->searchDocuments(op.queries[0], op.k, op.thr, cands, &dg);
                if (!r) { fail(r.error()); return o; }
                o.per.push_back(toAnswer(r.value(), model, o.error));
                counters();
                return o;
            }
            case mm::Op::SearchPq: {
                const std::vector<uint32_t>* cd = op.useCandidates ? &op.candidates : nullptr;
                auto r = table ? table->searchPqBatch(op.queries, op.luts, op.k, op.thr, op.rerank, cd, YAMS_PQ_SUM_SEQUENTIAL, &dg)
                               : index->searchPqBatch(op.queries, op.luts, op.k, op.thr, op.rerank, cd, YAMS_PQ_SUM_SEQUENTIAL, &dg);
                if (!r) { fail(r.error()); return o; }
                for (const auto& one : r.value()) o.per.push_back(toAnswer(one, model, o.error));
                counters();
                return o;
            }
            default: o.error = "not a search"; return o;
        }
    }
};

// The reference's own compiled loop (oracle/_ref/libyams_scan_ref.so, oracle/scan_ref_wrap.cpp): one scanref table, rows
// inserted with the model's rowid as their ordinal, a replacement = delete + insert as :1155-1167 does.
struct RefBackend : Backend {
    void* lib = nullptr; void* h = nullptr;
    bool l2 = false;
    uint64_t rebuiltAt = ~0ull; size_t rebuiltDim = 0;
    void* (*open_)(void) = nullptr; void (*close_)(void*) = nullptr;
    int (*insert_)(void*, const char*, const char*, const void*, int, long long, long long, const char*) = nullptr;
    int (*deleteOrdinal_)(void*, long long) = nullptr;
    long (*searchEx_)(void*, const float*, size_t, size_t, float, const char*, const char* const*, size_t, const char* const*, size_t, int, long long*, float*,
                      size_t, size_t*, unsigned long long*) = nullptr;
    long (*vec0Rebuild_)(void*, size_t) = nullptr;
    long (*vec0Search_)(void*, const float*, size_t, size_t, float, const long long*, size_t, long long*, float*, size_t, size_t*, unsigned long long*) = nullptr;
    int (*invalidArgument_)(void) = nullptr;
    explicit RefBackend(const char* path) {
        lib = dlopen(path, RTLD_NOW);
        if (!lib) { std::printf("dlopen %s: %s\n", path, dlerror()); return; }
        auto sym = [&](const char* n) { void* s = dlsym(lib, n); if (!s) std::printf("missing %s\n", n); return s; };
        open_ = reinterpret_cast<decltype(open_)>(sym("scanref_open")); close_ = reinterpret_cast<decltype(close_)>(sym("scanref_close"));
        insert_ = reinterpret_cast<decltype(insert_)>(sym("scanref_insert")); deleteOrdinal_ = reinterpret_cast<decltype(deleteOrdinal_)>(sym("scanref_delete_ordinal"));
        searchEx_ = reinterpret_cast<decltype(searchEx_)>(sym("scanref_search_ex")); vec0Rebuild_ = reinterpret_cast<decltype(vec0Rebuild_)>(sym("scanref_vec0_rebuild"));
        vec0Search_ = reinterpret_cast<decltype(vec0Search_)>(sym("scanref_vec0_search"));
        invalidArgument_ = reinterpret_cast<decltype(invalidArgument_)>(sym("scanref_error_code_invalid_argument"));
    }
    bool ok() const { return open_ && close_ && insert_ && deleteOrdinal_ && searchEx_ && vec0Rebuild_ && vec0Search_ && invalidArgument_; }
    void reset(bool vec0) { if (h) close_(h); h = open_(); l2 = vec0; rebuiltAt = ~0ull; }
    ~RefBackend() override { if (h) close_(h); }
    std::string mutate(const mm::Op&, const std::vector<mm::Change>& log, bool) override {
        for (const auto& c : log) {
            if (!c.inserted) { if (deleteOrdinal_(h, c.row.rowid) != 0) return "scanref_delete_ordinal failed"; continue; }
            std::string meta = "{";
            for (const auto& [k, v] : c.row.metadata) meta += (meta.size() > 1 ? ",\"" : "\"") + k + "\":\"" + v + "\"";
            meta += "}";
            if (insert_(h, c.row.chunk_id.c_str(), c.row.document_hash.c_str(), c.row.embedding.data(), static_cast<int>(c.row.embedding.size() * 4),
                        static_cast<long long>(c.row.embedding.size()), c.row.rowid, meta.c_str()) != 0)
                return "scanref_insert failed";
        }
        return {};
    }
    Outcome search(const mm::Op& op, const mm::HostModel& model) override {
        Outcome o;
        if (op.kind != mm::Op::Search && op.kind != mm::Op::SearchBatch) { o.unsupported = true; return o; }
        const size_t cap = model.count() + 1;
        std::vector<long long> ords(cap); std::vector<float> scores(cap);
        for (const auto& q : op.queries) {
            size_t n = 0; long rc; unsigned long long diag[4] = {0, 0, 0, 0};
            if (l2) {
                if (rebuiltAt != model.version || rebuiltDim != q.size()) {
                    if (vec0Rebuild_(h, q.size()) != 0) { o.error = "scanref_vec0_rebuild failed"; return o; }
                    rebuiltAt = model.version; rebuiltDim = q.size();
                }
                rc = vec0Search_(h, q.data(), q.size(), op.k, op.thr, nullptr, 0, ords.data(), scores.data(), cap, &n, nullptr);
            } else {
                std::vector<const char*> cd, kv;
                for (const auto& c : op.cands) cd.push_back(c.c_str());
                for (const auto& [k, v] : op.meta) { kv.push_back(k.c_str()); kv.push_back(v.c_str()); }
                rc = searchEx_(h, q.data(), q.size(), op.k, op.thr, op.doc ? op.doc->c_str() : nullptr, cd.data(), cd.size(), kv.data(), op.meta.size(),
                               op.all ? 1 : 0, ords.data(), scores.data(), cap, &n, diag);
            }
            mm::Answer a;
            if (rc == -static_cast<long>(invalidArgument_())) a.invalid = true;
            else if (rc != 0) { o.error = "the reference returned error " + std::to_string(-rc); return o; }
            for (size_t i = 0; i < n && i < cap; ++i) {
                auto it = model.rows.find(ords[i]);
                a.hits.push_back({it == model.rows.end() ? "<rowid " + std::to_string(ords[i]) + " not in the model>" : it->second.chunk_id, mm::bitsOf(scores[i])});
            }
            o.per.push_back(std::move(a));
            if (op.kind == mm::Op::Search && !l2) { o.counters = true; o.visited = diag[0]; o.evaluated = diag[1]; o.returned = diag[2]; }
        }
        return o;
    }
};

// ---- one run ---------------------------------------------------------------------------------------------------------------
struct Run {
    uint64_t seed; Backend& be; Counters& c; bool dry; char phase = '?';
    mm::HostModel model; mm::OpGenerator gen;
    bool l2 = false;
    size_t records = 0, dead = 0;     // the shape the mirror must have: rows incl. tombstones, tombstones (one index only)
    bool trackShape = false, pqSet = false, everHeld = false;
    uint64_t opNumber = 0;
    Run(uint64_t s, Backend& b, Counters& cn, bool dryRun) : seed(s), be(b), c(cn), dry(dryRun), gen(s) {}

    void report(const mm::Op& op, const std::string& what) {
        ++c.failures;
        if (c.failures <= 40) std::printf("MISMATCH seed=%llu phase=%c op#%llu [%s] live=%zu: %s\n", static_cast<unsigned long long>(seed), phase,
                                          static_cast<unsigned long long>(opNumber), op.describe().c_str(), model.count(), what.c_str());
    }
    // the mirror compacts on the first synchronisation after its tombstones exceed 1024 and a quarter of its rows
    void synchronised() {
        if (!trackShape) return;
        if (dead > 1024 && dead * 4 > records) {
            records -= dead; dead = 0;
            if (phase == 'B') ++c.compactionsB;
            else if (phase == 'C' && pqSet) ++c.compactionsC;
            else ++c.compactionsOther;
        }
    }
    void mutate(const mm::Op& op) {
        ++opNumber; ++c.mutations;
        std::vector<mm::Change> log; bool found = true;
        const size_t before = model.count();
        switch (op.kind) {
            case mm::Op::Insert: {
                log = model.insertBatch(op.recs);
                if (op.repeatedId) {
                    ++c.repeatedBatches;
                    std::map<std::string, size_t> dimOf;
                    for (const auto& r : op.recs) { auto [it, fresh] = dimOf.emplace(r.chunk_id, r.embedding.size()); if (!fresh && it->second != r.embedding.size()) { ++c.crossDimRepeats; break; } }
                }
                break;
            }
            case mm::Op::Erase: { auto r = model.erase(op.id); found = r.has_value(); if (r) log = std::move(*r); break; }
            case mm::Op::EraseDocument: log = model.eraseDocument(op.id); break;
            case mm::Op::Update: { auto r = model.update(op.id, op.recs[0]); found = r.has_value(); if (r) log = std::move(*r); break; }
            case mm::Op::SetPq: model.setPq(op.dim, op.codes, op.m, op.pqIds); synchronised(); pqSet = true; break;
            default: break;
        }
        if (!found) ++c.notFound;
        for (size_t i = 0; i < log.size(); ++i) {
            if (log[i].inserted) { ++records; everHeld = true; } else ++dead;
            if (!log[i].inserted && i + 1 < log.size() && log[i + 1].inserted && log[i + 1].row.chunk_id == log[i].row.chunk_id) ++c.replacements;
        }
        if (phase == 'B' && before < 4096 && model.count() >= 4096) ++c.layoutRemeasures;
        c.maxLive = std::max<uint64_t>(c.maxLive, model.count());
        if (const std::string err = be.mutate(op, log, found); !err.empty()) report(op, err);
    }
    Outcome expected(const mm::Op& op) const {
        Outcome o;
        switch (op.kind) {
            case mm::Op::Search:
                o.per.push_back(l2 ? model.l2(op.queries[0], op.k, op.thr) : model.cosine(op.queries[0], op.k, op.thr, op.doc, op.cands, op.meta, op.all));
                break;
            case mm::Op::SearchBatch: {   // (the queries of a batch are independent: the model answers them on a few threads)
                o.per.resize(op.queries.size());
                model.prepare(op.queries[0].size());
                std::vector<std::thread> pool;
                const size_t nt = std::min<size_t>(8, op.queries.size());
                for (size_t t = 0; t < nt; ++t)
                    pool.emplace_back([&, t] {
                        for (size_t i = t; i < op.queries.size(); i += nt) {
                            o.per[i] = l2 ? model.l2(op.queries[i], op.k, op.thr) : model.cosine(op.queries[i], op.k, op.thr, std::nullopt, {}, {}, false);
                            o.per[i].counters = false;
                        }
                    });
                for (auto& th : pool) th.join();
                break;
            }
            case mm::Op::SearchDocuments: o.per.push_back(model.documents(op.queries[0], op.k, op.thr, op.cands)); break;
            case mm::Op::SearchPq:
                for (size_t i = 0; i < op.queries.size(); ++i) o.per.push_back(model.pq(op.queries[i], op.luts[i], op.k, op.thr, op.rerank, op.useCandidates ? &op.candidates : nullptr));
                break;
            default: break;
        }
        bool invalid = false;
        for (const auto& a : o.per) invalid |= a.invalid;
        if (invalid) for (auto& a : o.per) { a = mm::Answer{}; a.invalid = true; }   // one invalid query fails the call (:1619-1626)
        o.counters = !o.per.empty() && o.per[0].counters && !invalid;
        for (const auto& a : o.per) { o.visited += a.visited; o.evaluated += a.evaluated; o.returned += a.returned; }
        if (op.kind == mm::Op::Search) o.returned = o.per[0].returned;
        return o;
    }
    void search(const mm::Op& op) {
        ++opNumber;
        synchronised();
        const Outcome want = expected(op);
        // coverage, from the model alone
        bool tie = false, invalid = false;
        for (const auto& a : want.per) { tie |= a.tie(); invalid |= a.invalid; }
        c.tieSearches += tie; c.invalidQueries += invalid;
        const size_t dim = op.queries[0].size();
        if (model.countDim(dim) == 0 && records == 0 && trackShape && everHeld) ++c.emptyIndex;
        if (op.kind == mm::Op::Search) {
            if (l2) ++c.l2;
            if (op.doc || !op.cands.empty()) ++c.docRestriction;
            if (!op.meta.empty()) ++c.metaPath;
            if (op.all) ++c.allMatching;
            if (op.k > mm::kScanMaxK) ++c.bigK;
        } else if (op.kind == mm::Op::SearchBatch) {
            ++c.batches;
            if (phase == 'B' && model.countDim(dim) > 16384 && op.queries.size() > 128) ++c.bigBatchB;
        } else if (op.kind == mm::Op::SearchDocuments) ++c.searchDocuments;
        else if (op.kind == mm::Op::SearchPq) { ++c.pq; c.pqWithCandidates += op.useCandidates; }
        if (dry) { ++c.compared; return; }
        const Outcome got = be.search(op, model);
        if (got.unsupported) { ++c.unpinned; return; }
        ++c.compared;
        if (!got.error.empty()) { report(op, "error: " + got.error); return; }
        const bool refused = be.striped() && (op.kind == mm::Op::SearchPq || op.kind == mm::Op::SearchDocuments);
        if (refused || got.notImplemented) {
            if (refused && got.notImplemented) ++c.notImplemented;
            else report(op, refused ? "a striped corpus must answer NotImplemented" : "NotImplemented from a corpus on one device");
            return;
        }
        if (got.per.size() != want.per.size()) { report(op, "answers for " + std::to_string(got.per.size()) + " queries, expected " + std::to_string(want.per.size())); return; }
        for (size_t q = 0; q < want.per.size(); ++q) {
            const auto& g = got.per[q]; const auto& w = want.per[q];
            if (g.invalid != w.invalid) { report(op, "query " + std::to_string(q) + (w.invalid ? ": expected InvalidArgument" : ": unexpected InvalidArgument")); return; }
            for (size_t i = 0; i < std::min(g.hits.size(), w.hits.size()); ++i)
                if (g.hits[i].chunk_id != w.hits[i].chunk_id || g.hits[i].bits != w.hits[i].bits) {
                    char b[256];
                    std::snprintf(b, sizeof b, "query %zu rank %zu: got %s %08x, expected %s %08x (sizes %zu / %zu)", q, i, g.hits[i].chunk_id.c_str(), g.hits[i].bits,
                                  w.hits[i].chunk_id.c_str(), w.hits[i].bits, g.hits.size(), w.hits.size());
                    report(op, b);
                    return;
                }
            if (g.hits.size() != w.hits.size()) { report(op, "query " + std::to_string(q) + ": " + std::to_string(g.hits.size()) + " results, expected " + std::to_string(w.hits.size())); return; }
        }
        if (want.counters && got.counters && (got.visited != want.visited || got.evaluated != want.evaluated || got.returned != want.returned)) {
            char b[200];
            std::snprintf(b, sizeof b, "counters visited/evaluated/returned: got %llu/%llu/%llu, expected %llu/%llu/%llu", static_cast<unsigned long long>(got.visited),
                          static_cast<unsigned long long>(got.evaluated), static_cast<unsigned long long>(got.returned), static_cast<unsigned long long>(want.visited),
                          static_cast<unsigned long long>(want.evaluated), static_cast<unsigned long long>(want.returned));
            report(op, b);
            return;
        }
        if (trackShape && be.mirrorRows() >= 0 && static_cast<size_t>(be.mirrorRows()) != records)
            report(op, "mirrorRows() = " + std::to_string(be.mirrorRows()) + ", the mirror's rules give " + std::to_string(records));
    }
    void apply(const mm::Op& op) { if (op.kind >= mm::Op::Search && op.kind != mm::Op::SetPq) search(op); else mutate(op); }

    // ---- building blocks of the phases ------------------------------------------------------------------------------------
    size_t ragged(size_t maxBatch) { const uint32_t r = gen.below(100); return r < 25 ? 1 + gen.below(3) : (r < 85 ? 1 + gen.below(static_cast<uint32_t>(std::max<size_t>(maxBatch / 8, 1))) : 1 + gen.below(static_cast<uint32_t>(maxBatch))); }
    void growTo(size_t live, size_t maxBatch, size_t every, const std::function<void()>& searches) {
        for (size_t step = 0; model.count() < live; ++step) {
            const uint32_t what = gen.below(100);
            if (what < 6 && model.count() > 10) apply(gen.erase(model));
            else if (what < 12 && model.count() > 10) apply(gen.update(model));
            else apply(gen.insert(model, std::min(ragged(maxBatch), live + 50 - model.count())));
            if (every && step % every == every - 1) searches();
        }
    }
    void shrinkTo(size_t live, size_t every, const std::function<void()>& searches) {
        for (size_t step = 0; model.count() > live; ++step) {
            const uint32_t what = gen.below(100);
            if (what < 55) apply(gen.eraseDocument(model));
            else if (what < 90) { for (int i = 0; i < 60 && model.count() > live; ++i) apply(gen.erase(model)); }
            else apply(gen.insert(model, 1 + gen.below(40)));
            if (every && step % every == every - 1) searches();
            if (step > 200000) break;
        }
    }
};

static int runScripted(uint64_t seed, Backend& be, Counters& c, bool dry, AdapterBackend* ad, RefBackend* ref) {
    mm::OpGenerator g(seed ^ 0x5c);
    auto vec = [&](size_t dim) { return g.randomVector(dim); };
    auto rec = [&](const std::string& id, const std::string& doc, std::vector<float> e) { mm::Rec r; r.chunk_id = id; r.document_hash = doc; r.embedding = std::move(e); return r; };
    auto idOf = [](const char* p, int i) { char b[24]; std::snprintf(b, sizeof b, "%s%05d", p, i); return std::string(b); };
    // 1. a compaction that restores the row count: 4000 rows, setPqIndex, delete 1500, insert 1500 new rows, searchPqBatch
    if (!ref) {
        Run r(seed, be, c, dry); r.phase = '1'; r.trackShape = true;
        if (ad) { ad->table.reset(); ad->index = std::move(vector::createAccelVectorIndex(ad->plugin, 16).value()); if (!ad->index->initialize()) return 1; }
        mm::Op ins; ins.kind = mm::Op::Insert;
        for (int i = 0; i < 4000; ++i) ins.recs.push_back(rec(idOf("p", i), "doc" + std::to_string(i % 40), vec(16)));
        r.apply(ins);
        r.gen.profile.dims = {16};
        r.apply(r.gen.setPq(r.model, 16, 8));
        r.apply(r.gen.searchPq(r.model, 3, false));
        for (int i = 0; i < 1500; ++i) { mm::Op e; e.kind = mm::Op::Erase; e.id = idOf("p", i * 2); r.apply(e); }
        mm::Op more; more.kind = mm::Op::Insert;
        for (int i = 0; i < 1500; ++i) more.recs.push_back(rec(idOf("q", i), "doc" + std::to_string(i % 40), vec(16)));
        r.apply(more);
        if (ad && !be.striped() && ad->index->mirrorRows() != 5500) r.report(more, "mirrorRows() before the search is not 5500");
        r.apply(r.gen.searchPq(r.model, 3, false));
        if (r.records != 4000 || (ad && ad->index->mirrorRows() != 4000)) r.report(more, "the compaction did not restore 4000 rows");
        r.apply(r.gen.searchPq(r.model, 2, true));
    }
    // 2. [a, b, a'] with a' and b equidistant under the vec0 engine: first-occurrence position, last content
    {
        Run r(seed, be, c, dry); r.phase = '2'; r.l2 = true;
        if (ad) {
            ad->table.reset(); ad->index = std::move(vector::createAccelVectorIndex(ad->plugin, 8, vector::VectorSearchEngine::Vec0L2).value());
            if (!ad->index->initialize()) return 1;
            ad->index->setL2(vector::L2Setting{true, true, YAMS_SCAN_FLAG_L2_ACC_F64 | YAMS_SCAN_FLAG_L2_ACC_EXPLICIT, "fp64, set by the test"});
        }
        if (ref) ref->reset(true);
        const auto e1 = vec(8), e2 = vec(8);
        mm::Op ins; ins.kind = mm::Op::Insert; ins.repeatedId = true;
        ins.recs = {rec("a", "d1", e1), rec("b", "d1", e2), rec("a", "d2", e2), rec("c", "d2", vec(8))};
        r.apply(ins);
        mm::Op s; s.kind = mm::Op::Search; s.queries = {e2}; s.k = 3; s.thr = -1.0f;
        r.apply(s);
    }
    // 3. the same chunk_id at two dimensions in one batch of the table: the last write wins
    {
        Run r(seed, be, c, dry); r.phase = '3';
        if (ad) { ad->index.reset(); ad->table = std::make_unique<vector::AccelVectorTable>(ad->plugin); }
        if (ref) ref->reset(false);
        const auto e8 = vec(8), e4 = vec(4);
        mm::Op ins; ins.kind = mm::Op::Insert; ins.repeatedId = true;
        ins.recs = {rec("b", "d1", vec(8)), rec("a", "d1", e8), rec("c", "d1", vec(4)), rec("a", "d2", e4)};
        r.apply(ins);
        for (const auto& q : {e8, e4}) { mm::Op s; s.kind = mm::Op::Search; s.queries = {q}; s.k = 5; s.thr = -1.0f; r.apply(s); }
    }
    return 0;
}

static int runPhases(uint64_t seed, Backend& be, Counters& c, bool dry, AdapterBackend* ad, RefBackend* ref, size_t ops) {
    auto scaled = [&](size_t n) { return std::max<size_t>(1, n * ops / 100); };
    // ---- A: AccelVectorTable, dims 8 / 32 / 48 -----------------------------------------------------------------------------
    {
        Run r(seed, be, c, dry); r.phase = 'A';
        r.gen.profile = {{8, 32, 48}, 7000, 50, 300, true, false};
        if (ad) { ad->index.reset(); ad->table = std::make_unique<vector::AccelVectorTable>(ad->plugin); }
        if (ref) ref->reset(false);
        int turn = 0;
        auto searches = [&] {
            for (size_t i = 0; i < scaled(3); ++i) {
                switch (turn++ % 8) {
                    case 0: r.apply(r.gen.search(r.model, 5)); break;
                    case 1: r.apply(r.gen.search(r.model, 1)); break;
                    case 2: r.apply(r.gen.search(r.model, 2)); break;
                    case 3: r.apply(r.gen.search(r.model, 3)); break;
                    case 4: r.apply(r.gen.search(r.model, 4)); break;
                    case 5: r.apply(r.gen.searchDocuments(r.model)); break;
                    case 6: r.apply(r.gen.searchBatch(r.model, 1 + r.gen.below(12))); break;
                    default: r.apply(r.gen.search(r.model, 0)); break;
                }
            }
        };
        r.growTo(1500, 200, 5, searches);
        r.growTo(5200, 600, 8, searches);
        r.shrinkTo(3200, 10, searches);
        r.growTo(5600, 500, 8, searches);
    }
    // ---- D: AccelVectorIndex(Vec0L2), dim 64, fp64 accumulation ------------------------------------------------------------
    {
        Run r(seed + 1000, be, c, dry); r.phase = 'D'; r.l2 = true; r.trackShape = true;
        r.gen.profile = {{64}, 9000, 40, 200, false, true};
        if (ad) {
            ad->table.reset(); ad->index = std::move(vector::createAccelVectorIndex(ad->plugin, 64, vector::VectorSearchEngine::Vec0L2).value());
            if (!ad->index->initialize()) return 1;
            ad->index->setL2(vector::L2Setting{true, true, YAMS_SCAN_FLAG_L2_ACC_F64 | YAMS_SCAN_FLAG_L2_ACC_EXPLICIT, "fp64, set by the test"});
        }
        if (ref) ref->reset(true);
        int turn = 0;
        auto searches = [&] {
            for (size_t i = 0; i < scaled(2); ++i) {
                if (turn % 9 == 4) r.apply(r.gen.search(r.model, 4));
                else if (turn % 9 == 7) r.apply(r.gen.searchBatch(r.model, 1 + r.gen.below(9)));
                else r.apply(r.gen.search(r.model, 0));
                ++turn;
            }
        };
        r.growTo(2500, 300, 5, searches);
        r.growTo(7000, 900, 6, searches);
        r.shrinkTo(3000, 8, searches);
        r.growTo(4500, 400, 6, searches);
        // every row deleted: by document, then the rows that carry no document
        for (uint32_t d = 0; d < r.gen.profile.docPool; ++d) { mm::Op e; e.kind = mm::Op::EraseDocument; e.id = r.gen.docName(d); r.apply(e); }
        while (r.model.count()) { mm::Op e; e.kind = mm::Op::Erase; e.id = r.model.rows.begin()->second.chunk_id; r.apply(e); }
        r.apply(r.gen.search(r.model, 0));
        r.apply(r.gen.search(r.model, 4));
        r.growTo(300, 100, 2, searches);
    }
    if (ref) return 0;   // (the reference loop pins phases A and D)
    // ---- B: AccelVectorIndex, dim 256, cosine: shadows appended, cleared and rebuilt ---------------------------------------
    Run r(seed + 2000, be, c, dry); r.phase = 'B'; r.trackShape = true;
    r.gen.profile = {{256}, 30000, 220, 500, false, false};
    if (ad) { ad->table.reset(); ad->index = std::move(vector::createAccelVectorIndex(ad->plugin, 256).value()); if (!ad->index->initialize()) return 1; }
    int turn = 0;
    static const size_t widths[] = {1, 7, 129, 7, 1, 300};
    auto small = [&] {   // single-query searches of the kinds that stay cheap at any size
        for (size_t i = 0; i < scaled(2); ++i) {
            switch (turn++ % 5) {
                case 0: r.apply(r.gen.search(r.model, 5)); break;
                case 1: r.apply(r.gen.search(r.model, 1)); break;
                case 2: r.apply(r.gen.searchDocuments(r.model)); break;
                case 3: r.apply(r.gen.search(r.model, 2)); break;
                default: r.apply(r.gen.searchBatch(r.model, widths[r.gen.below(2)])); break;
            }
        }
    };
    auto wide = [&](size_t nq) { r.apply(r.gen.searchBatch(r.model, nq)); };
    r.apply(r.gen.search(r.model, 5));                     // an index that never held a row
    r.growTo(3000, 700, 6, small);
    wide(129);
    r.growTo(9000, 2500, 5, small);                        // the int8 layout is measured again at 4096 rows
    wide(7);
    r.growTo(20500, 5000, 4, small);
    wide(300); wide(129);
    r.shrinkTo(9000, 10, small);                           // through two compactions
    wide(129);
    r.shrinkTo(2500, 25, small);
    wide(7);
    r.growTo(17000, 5000, 4, small);                       // past 4096 and 16 384 again, on a mirror that was cleared and rebuilt
    wide(300); wide(129);
    // ---- C: the same index, PQ: setPqIndex ONCE, then CRUD without calling it again ----------------------------------------
    r.phase = 'C';
    r.apply(r.gen.setPq(r.model, 256, 16));
    auto pq = [&] {
        for (size_t i = 0; i < scaled(2); ++i) {
            switch (turn++ % 4) {
                case 0: r.apply(r.gen.searchPq(r.model, 1 + r.gen.below(4), false)); break;
                case 1: r.apply(r.gen.searchPq(r.model, 1 + r.gen.below(9), true)); break;
                case 2: r.apply(r.gen.search(r.model, 1)); break;
                default: r.apply(r.gen.searchPq(r.model, 1, r.gen.chance(50))); break;
            }
        }
    };
    pq(); pq();
    r.growTo(17600, 300, 4, pq);                           // appends and replacements under the index
    r.shrinkTo(11000, 10, pq);                             // a compaction after setPqIndex
    r.growTo(12500, 800, 4, pq);
    pq();
    return 0;
}

int main(int argc, char** argv) {
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    std::string pluginPath, config = "{\"device\":0}", refPath;
    uint64_t seed = 1; size_t ops = 100;
    bool dry = false, expectNoGpu = false, onlyScripted = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--config" && i + 1 < argc) config = argv[++i];
        else if (a == "--seed" && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--ops" && i + 1 < argc) ops = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--dry-run") dry = true;
        else if (a == "--model-only" && i + 1 < argc) refPath = argv[++i];
        else if (a == "--expect-no-gpu") expectNoGpu = true;
        else if (a == "--only-scripted") onlyScripted = true;
        else if (a[0] != '-') pluginPath = a;
        else { std::printf("unknown argument %s\n", a.c_str()); return 2; }
    }
    if (!dry && refPath.empty() && pluginPath.empty()) {
        std::printf("usage: %s <plugin.so> [--config <json>] --seed S [--ops N] | --dry-run --seed S | --model-only <libyams_scan_ref.so> --seed S | <plugin.so> --expect-no-gpu\n", argv[0]);
        return 2;
    }
    Counters c;
    std::unique_ptr<Backend> be;
    AdapterBackend* ad = nullptr; RefBackend* ref = nullptr;
    const char* mode = dry ? "dry-run" : (!refPath.empty() ? "model-only" : "device");
    if (dry) be = std::make_unique<NullBackend>();
    else if (!refPath.empty()) {
        auto rb = std::make_unique<RefBackend>(refPath.c_str());
        if (!rb->ok()) { std::printf("FAILED: %s lacks an entry this leg needs\n", refPath.c_str()); return 1; }
        ref = rb.get(); be = std::move(rb);
    } else {
        auto loaded = accel::Plugin::load(pluginPath, config);
        if (expectNoGpu) {   // no device: the plugin refuses to initialise, nothing falls back
            const bool refused = !loaded.has_value() && loaded.error().code == ErrorCode::NotInitialized;
            std::printf("%s\n", refused ? "OK (0 failures, refused without a GPU)" : "FAILED: the plugin initialised or failed otherwise");
            return refused ? 0 : 1;
        }
        if (!loaded.has_value()) { std::printf("plugin load failed: %s\n", loaded.error().message.c_str()); return 1; }
        auto ab = std::make_unique<AdapterBackend>(loaded.value(), config.find("\"devices\"") != std::string::npos);
        ad = ab.get(); be = std::move(ab);
    }
    if (runScripted(seed, *be, c, dry, ad, ref) != 0) { std::printf("FAILED: could not set up a scripted case\n"); return 1; }
    if (!onlyScripted && runPhases(seed, *be, c, dry, ad, ref, ops) != 0) { std::printf("FAILED: could not set up a phase\n"); return 1; }
    if (ad) { ad->index.reset(); ad->table.reset(); }

    // the coverage conditions: the run must have reached what it is for
    std::vector<std::string> missing;
    auto need = [&](bool ok, const char* what) { if (!ok) missing.push_back(what); };
    if (!onlyScripted && ref) {
        need(c.compared >= 100, "100 searches compared with the reference-compiled table");
        need(c.l2 >= 10 && c.docRestriction >= 10 && c.metaPath >= 10 && c.allMatching >= 10 && c.bigK >= 10, "10 searches of every pinned kind");
    } else if (!onlyScripted) {
        need(c.compared >= 300, ">= 300 compared searches");
        need(c.compactionsB >= 2, ">= 2 compactions in phase B");
        need(c.compactionsC >= 1, ">= 1 compaction in phase C after setPqIndex");
        need(c.bigBatchB >= 1, ">= 1 search in phase B at > 16384 live rows with > 128 queries");
        need(c.layoutRemeasures >= 2, "phase B crosses 4096 rows twice");
        need(c.replacements >= 20, ">= 20 replacements of a live chunk_id");
        need(c.repeatedBatches >= 5, ">= 5 batches with a repeated chunk_id");
        need(c.crossDimRepeats >= 1, ">= 1 batch that repeats a chunk_id across dimensions");
        need(c.tieSearches >= 10, ">= 10 searches whose expected top-k contains an exact tie");
        need(c.docRestriction >= 10 && c.metaPath >= 10 && c.allMatching >= 10 && c.bigK >= 10 && c.searchDocuments >= 10 && c.pq >= 10,
             ">= 10 searches each of: document restriction, metadata path, AllMatching, k > YAMS_SCAN_MAX_K, searchDocuments, PQ");
        need(c.emptyIndex >= 1, ">= 1 search over an index whose every row was deleted");
        need(c.skipped == 0 && c.unpinned == 0, "zero searches skipped");
        if (ad) need(c.notImplemented == (be->striped() ? c.pq + c.searchDocuments : 0), "NotImplemented for exactly the PQ and document searches of a striped corpus");
    }
    std::printf("{\"mode\":\"%s\",\"seed\":%llu,\"ops\":%zu,\"compared\":%llu,\"failures\":%llu,\"mutations\":%llu,\"max_live\":%llu,\"replacements\":%llu,"
                "\"repeated_batches\":%llu,\"cross_dim_repeats\":%llu,\"tie_searches\":%llu,\"doc_restriction\":%llu,\"meta_path\":%llu,\"all_matching\":%llu,"
                "\"big_k\":%llu,\"search_documents\":%llu,\"pq\":%llu,\"pq_with_candidates\":%llu,\"l2\":%llu,\"batches\":%llu,\"empty_index\":%llu,"
                "\"compactions_b\":%llu,\"compactions_c\":%llu,\"big_batch_b\":%llu,\"layout_remeasures\":%llu,\"invalid_queries\":%llu,\"not_found\":%llu,"
                "\"not_implemented\":%llu,\"unpinned\":%llu,\"skipped\":%llu,\"coverage_missing\":%zu}\n",
                mode, (unsigned long long)seed, ops, (unsigned long long)c.compared, (unsigned long long)c.failures, (unsigned long long)c.mutations,
                (unsigned long long)c.maxLive, (unsigned long long)c.replacements, (unsigned long long)c.repeatedBatches, (unsigned long long)c.crossDimRepeats,
                (unsigned long long)c.tieSearches, (unsigned long long)c.docRestriction, (unsigned long long)c.metaPath, (unsigned long long)c.allMatching,
                (unsigned long long)c.bigK, (unsigned long long)c.searchDocuments, (unsigned long long)c.pq, (unsigned long long)c.pqWithCandidates,
                (unsigned long long)c.l2, (unsigned long long)c.batches, (unsigned long long)c.emptyIndex, (unsigned long long)c.compactionsB,
                (unsigned long long)c.compactionsC, (unsigned long long)c.bigBatchB, (unsigned long long)c.layoutRemeasures, (unsigned long long)c.invalidQueries,
                (unsigned long long)c.notFound, (unsigned long long)c.notImplemented, (unsigned long long)c.unpinned, (unsigned long long)c.skipped, missing.size());
    for (const auto& m : missing) std::printf("COVERAGE NOT MET: %s\n", m.c_str());
    const bool ok = c.failures == 0 && missing.empty();
    std::printf("%s (%llu failures, %llu comparisons)\n", ok ? "OK" : "FAILED", (unsigned long long)c.failures, (unsigned long long)c.compared);
    return ok ? 0 : 1;
}
