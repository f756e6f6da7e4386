// mirror_model.hpp — TEST: an independent host model of the `vectors` table and a seeded operation generator, for
// tests/cpp/mirror_model_test.cpp.  Plain C++20: no GPU, no plugin, none of the adapter's code (include/yams_accel is
// not included here).  The model owns WHICH ROWS EXIST AND IN WHAT ORDER — the CRUD rules of the reference's
// sqlite_vec_backend.cpp, each restated next to the lines it comes from —; the ARITHMETIC and the selection of every
// search come from the oracle's C restatement (oracle/yams_oracle.c, linked as l2_calibration_test links it), which is
// pinned on the reference-compiled loop by tests/test_oracle.py and, for the model as a whole, by this driver's
// --model-only leg.  Not pinned by compiled reference code: the batch de-duplication rule, the best-row-per-document
// reduction and the product-quantised engine (restated).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <optional>
#include <set>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

extern "C" {
long oracle_exact_scan_cosine(const float* corpus, size_t n_rows, size_t dim, const float* query, size_t k, float similarity_threshold,
                              const uint64_t* tie_rank, int64_t* out_rows, float* out_sims, uint64_t* rows_visited, uint64_t* evaluations);
long oracle_exact_scan_cosine_records(const float* corpus, size_t n_rows, size_t dim, const float* query, size_t k, int all_matching,
                                      float similarity_threshold, const uint64_t* tie_rank, const uint8_t* allow, int64_t* out_rows,
                                      float* out_sims, uint64_t* evaluations);
long oracle_exact_scan_l2(const float* corpus, size_t n_rows, size_t dim, const float* query, size_t k, float similarity_threshold,
                          const uint64_t* tie_rank, int64_t* out_rows, float* out_dist, float* out_sims);
long oracle_pq_search(const float* corpus, size_t n_rows, size_t dim, const uint8_t* codes, size_t n_codes, size_t m, const float* lut,
                      const uint64_t* tie_keys, const uint32_t* row_of_index, const uint64_t* chunk_rank, const float* query, size_t k,
                      float threshold, size_t rerank_factor, const uint32_t* candidates, size_t n_candidates, int sum_lanes,
                      int64_t* out_rows, float* out_sims, uint64_t* out_stats);
}

namespace mirror_model {

constexpr size_t kScanMaxK = 1024;   // YAMS_SCAN_MAX_K restated (the driver static_asserts that the two agree)

struct Rec {
    std::string chunk_id, document_hash;
    std::map<std::string, std::string> metadata;
    std::vector<float> embedding;
};
struct Row : Rec { int64_t rowid = 0; };
struct Change { bool inserted; Row row; };          // what a mutation did to the table, in the order it did it
struct Hit { std::string chunk_id; uint32_t bits; };
struct Answer {
    bool invalid = false;                           // the reference answers InvalidArgument (:4127-4130)
    std::vector<Hit> hits;
    bool counters = false;                          // the reference reports the three counters for this kind of search
    uint64_t visited = 0, evaluated = 0, returned = 0;
    bool tie() const {
        for (size_t i = 1; i < hits.size(); ++i) if (hits[i].bits == hits[i - 1].bits) return true;
        return false;
    }
};

inline uint32_t bitsOf(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
inline uint64_t stableStringKey(const std::string& s) {   // FNV-1a 64 (:141-148)
    uint64_t h = 1469598103934665603ULL;
    for (const unsigned char b : s) { h ^= b; h *= 1099511628211ULL; }
    return h;
}

// The host's SimeonPqIndexState as the engine reads it (:48-62): codes, and per indexed row the ROWID it had when the
// index was built.  A row deleted or replaced since then (a replacement takes a new rowid, :1155-1167) is a row the
// table lost: getVectorByRowidUnlocked finds nothing and the hit is skipped (:4010-4012).
struct PqIndex {
    size_t dim = 0, m = 0;
    std::vector<uint8_t> codes;
    std::vector<std::string> chunk_ids;
    std::vector<int64_t> rowids;                    // -1: the chunk id named no row when the index was set
    std::vector<uint64_t> keys;                     // stableStringKey(chunk id) (:3337)
};

class HostModel {
public:
    std::map<int64_t, Row> rows;                    // rowid order (:4175 ORDER BY rowid)
    std::unordered_map<std::string, int64_t> byId;
    int64_t nextRowid = 1;
    uint64_t version = 0;                           // bumped by every mutation (snapshots are cached per version)
    PqIndex pqIndex;

    size_t count() const { return rows.size(); }
    size_t countDim(size_t dim) const { size_t n = 0; for (const auto& [id, r] : rows) n += r.embedding.size() == dim; return n; }
    const Row* find(const std::string& id) const {
        auto it = byId.find(id);
        return it == byId.end() ? nullptr : &rows.at(it->second);
    }

    // insertVectorsBatch (:1086-1226).  One table for every dimension: a chunk_id lives in one row (chunk_id is
    // UNIQUE, :342-371), so re-inserting it with another embedding size moves it.
    std::vector<Change> insertBatch(const std::vector<Rec>& recs) {
        std::vector<Change> log;
        // :1114-1130 — unique_indices keeps the POSITION of a chunk_id's first occurrence and the INDEX of its last
        std::vector<size_t> unique;
        std::unordered_map<std::string, size_t> pos;
        for (size_t i = 0; i < recs.size(); ++i) {
            auto it = pos.find(recs[i].chunk_id);
            if (it == pos.end()) { pos.emplace(recs[i].chunk_id, unique.size()); unique.push_back(i); }
            else unique[it->second] = i;
        }
        for (size_t i : unique) {
            // :1136-1176 — an existing row is deleted and the record inserted again: a new rowid, at the end
            if (auto it = byId.find(recs[i].chunk_id); it != byId.end()) removeRow(it->second, log);
            addRow(recs[i], log);                   // :1178-1190
        }
        ++version;
        return log;
    }
    // deleteVector (:1318-1375): NotFound when the chunk_id names no row
    std::optional<std::vector<Change>> erase(const std::string& id) {
        auto it = byId.find(id);
        if (it == byId.end()) return std::nullopt;
        std::vector<Change> log;
        removeRow(it->second, log);
        ++version;
        return log;
    }
    // deleteVectorsByDocument: every row of the document, whatever its dimension
    std::vector<Change> eraseDocument(const std::string& hash) {
        std::vector<Change> log;
        std::vector<int64_t> ids;
        for (const auto& [rowid, r] : rows) if (r.document_hash == hash) ids.push_back(rowid);
        for (int64_t rowid : ids) removeRow(rowid, log);
        ++version;
        return log;
    }
    // updateVector (:1228-1316): NotFound, else delete + insert inside one savepoint (:1271-1283) — the row moves to the end
    std::optional<std::vector<Change>> update(const std::string& id, const Rec& rec) {
        auto it = byId.find(id);
        if (it == byId.end()) return std::nullopt;
        std::vector<Change> log;
        removeRow(it->second, log);
        Rec r = rec; r.chunk_id = id;
        addRow(r, log);
        ++version;
        return log;
    }

    void setPq(size_t dim, const std::vector<uint8_t>& codes, size_t m, const std::vector<std::string>& ids) {
        pqIndex = PqIndex{dim, m, codes, ids, {}, {}};
        for (const auto& id : ids) {
            const Row* r = find(id);
            pqIndex.rowids.push_back(r && r->embedding.size() == dim ? r->rowid : -1);
            pqIndex.keys.push_back(stableStringKey(id));
        }
    }

    // ---- searches -----------------------------------------------------------------------------------------------------
    // bruteForceSearchUnlocked (:4115-4409).  The statement visits the rows of the query's dimension (:4147) whose
    // document_hash equals `doc` (if given) and is in `cands` (if not empty) (:4151-4175); no metadata filter: the fast
    // path (:4228-4326); a metadata filter: the record path with its norm^2 < 1e-10 rule (:4333-4409); `all`:
    // ExactRowSelection::AllMatching (:4398-4400; on the fast path the heap is as large as the table).
    Answer cosine(const std::vector<float>& q, size_t k, float thr, const std::optional<std::string>& doc,
                  const std::vector<std::string>& cands, const std::map<std::string, std::string>& meta, bool all) const {
        Snap local;
        const bool whole = !doc && cands.empty();
        if (!whole) local = restricted(q.size(), doc, cands);
        const Snap& s = whole ? snapshot(q.size()) : local;
        const size_t n = s.r.size();
        Answer a; a.counters = true;
        std::vector<int64_t> outRows(std::max<size_t>(n, 1));
        std::vector<float> outSims(std::max<size_t>(n, 1));
        long got;
        if (meta.empty()) {
            const size_t kk = std::min<size_t>(all ? std::max<size_t>(n, 1) : k, std::max<size_t>(n, 1));
            got = oracle_exact_scan_cosine(s.flat.data(), n, q.size(), q.data(), kk, thr, s.rank.data(), outRows.data(), outSims.data(),
                                           &a.visited, &a.evaluated);
        } else {
            std::vector<uint8_t> allow(std::max<size_t>(n, 1), 0);
            for (size_t i = 0; i < n; ++i) {          // :4350-4360: every (key, value) pair must be present
                bool ok = true;
                for (const auto& [key, value] : meta) {
                    auto it = s.r[i]->metadata.find(key);
                    if (it == s.r[i]->metadata.end() || it->second != value) { ok = false; break; }
                }
                allow[i] = ok;
            }
            got = oracle_exact_scan_cosine_records(s.flat.data(), n, q.size(), q.data(), k, all ? 1 : 0, thr, s.rank.data(), allow.data(),
                                                   outRows.data(), outSims.data(), &a.evaluated);
            a.visited = n;                            // :4336-4338
        }
        if (got < 0) { a.invalid = true; a.visited = a.evaluated = 0; return a; }
        for (long i = 0; i < got; ++i) a.hits.push_back({s.r[static_cast<size_t>(outRows[i])]->chunk_id, bitsOf(outSims[i])});
        a.returned = a.hits.size();
        return a;
    }
    // CandidateFilterMode::DocumentTopK, exact arm (:1508-1518): every matching row of the candidate documents, then
    // retainBestRecordPerDocument (:86-125).  `returned` = the matching rows before the reduction.
    Answer documents(const std::vector<float>& q, size_t k, float thr, const std::vector<std::string>& cands) const {
        Answer rowsAns = cosine(q, 0, thr, std::nullopt, cands, {}, true);
        if (rowsAns.invalid) return rowsAns;
        struct Best { uint32_t bits; float score; std::string chunk, doc; };
        std::unordered_map<std::string, Best> best;
        for (const auto& h : rowsAns.hits) {
            const Row* r = find(h.chunk_id);
            if (r->document_hash.empty()) continue;                                       // :90-92
            float sc; std::memcpy(&sc, &h.bits, 4);
            auto it = best.find(r->document_hash);
            if (it == best.end()) { best.emplace(r->document_hash, Best{h.bits, sc, h.chunk_id, r->document_hash}); continue; }   // :94-98
            if (sc > it->second.score || (sc == it->second.score && h.chunk_id < it->second.chunk))             // :99-103
                it->second = Best{h.bits, sc, h.chunk_id, r->document_hash};
        }
        std::vector<Best> out;
        for (auto& [d, b] : best) out.push_back(b);
        std::sort(out.begin(), out.end(), [](const Best& x, const Best& y) {                 // :111-121
            if (x.score != y.score) return x.score > y.score;
            if (x.doc != y.doc) return x.doc < y.doc;
            return x.chunk < y.chunk;
        });
        if (out.size() > k) out.resize(k);                                                  // :122-124
        Answer a; a.counters = true; a.visited = rowsAns.visited; a.evaluated = rowsAns.evaluated; a.returned = rowsAns.hits.size();
        for (const auto& b : out) a.hits.push_back({b.chunk, b.bits});
        return a;
    }
    // vec0SearchUnlocked (:4450-4530) with the fp64 definition of the distance: the k nearest, equal distances in rowid
    // order, THEN the similarity threshold (:4506-4510).  The function takes no diagnostics: no counters.
    Answer l2(const std::vector<float>& q, size_t k, float thr) const {
        const Snap& s = snapshot(q.size());
        const size_t n = s.r.size();
        Answer a;
        const size_t kk = std::min(k, std::max<size_t>(n, 1));
        std::vector<int64_t> outRows(kk);
        std::vector<float> outDist(kk), outSims(kk);
        const long got = oracle_exact_scan_l2(s.flat.data(), n, q.size(), q.data(), kk, thr, nullptr, outRows.data(), outDist.data(), outSims.data());
        for (long i = 0; i < got; ++i) a.hits.push_back({s.r[static_cast<size_t>(outRows[i])]->chunk_id, bitsOf(outSims[i])});
        return a;
    }
    // simeonPqSearchUnlocked (:3868-4056) over the index of setPq: the oracle's restatement with THIS table's live rows,
    // its own index -> row table (0xffffffff: a row the table lost) and the chunk_id ranking of the final order.
    Answer pq(const std::vector<float>& q, const std::vector<float>& lut, size_t k, float thr, size_t rerank,
              const std::vector<uint32_t>* candidates) const {
        Answer a; a.counters = true;
        const PqIndex& p = pqIndex;
        if (p.dim != q.size() || p.chunk_ids.empty()) return a;                            // :3877-3880
        const Snap& s = snapshot(q.size());
        std::unordered_map<int64_t, uint32_t> where;
        for (size_t i = 0; i < s.r.size(); ++i) where.emplace(s.r[i]->rowid, static_cast<uint32_t>(i));
        std::vector<uint32_t> rowOf(p.rowids.size(), 0xffffffffu);
        for (size_t i = 0; i < p.rowids.size(); ++i)
            if (auto it = where.find(p.rowids[i]); it != where.end()) rowOf[i] = it->second;
        std::vector<int64_t> outRows(std::max<size_t>(k, 1));
        std::vector<float> outSims(std::max<size_t>(k, 1));
        uint64_t stats[2] = {0, 0};
        static const uint32_t none = 0;
        const long got = oracle_pq_search(s.flat.data(), s.r.size(), q.size(), p.codes.data(), p.chunk_ids.size(), p.m, lut.data(), p.keys.data(),
                                          rowOf.data(), s.rank.data(), q.data(), k, thr, rerank,
                                          candidates ? (candidates->empty() ? &none : candidates->data()) : nullptr,
                                          candidates ? candidates->size() : 0, 1, outRows.data(), outSims.data(), stats);
        for (long i = 0; i < got; ++i) a.hits.push_back({s.r[static_cast<size_t>(outRows[i])]->chunk_id, bitsOf(outSims[i])});
        a.visited = stats[0]; a.evaluated = stats[1]; a.returned = a.hits.size();
        return a;
    }

    void prepare(size_t dim) const { (void)snapshot(dim); }   // (before answering on several threads: the cache is filled by one)

private:
    struct Snap {                                   // a dense snapshot: rows in rowid order, chunk_id ranks (:4218-4223)
        std::vector<const Row*> r;
        std::vector<float> flat;
        std::vector<uint64_t> rank;
        void finish(size_t dim) {
            flat.resize(std::max<size_t>(r.size() * dim, 1));
            for (size_t i = 0; i < r.size(); ++i) std::copy(r[i]->embedding.begin(), r[i]->embedding.end(), flat.begin() + i * dim);
            std::vector<uint32_t> order(r.size());
            for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
            std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return r[a]->chunk_id < r[b]->chunk_id; });
            rank.assign(std::max<size_t>(r.size(), 1), 0);
            for (uint32_t p = 0; p < order.size(); ++p) rank[order[p]] = p;
        }
    };
    mutable std::map<size_t, std::pair<uint64_t, Snap>> cache_;
    const Snap& snapshot(size_t dim) const {
        auto& slot = cache_[dim];
        if (slot.first != version + 1) {
            slot.second = Snap{};
            for (const auto& [rowid, r] : rows) if (r.embedding.size() == dim) slot.second.r.push_back(&r);
            slot.second.finish(dim);
            slot.first = version + 1;
        }
        return slot.second;
    }
    Snap restricted(size_t dim, const std::optional<std::string>& doc, const std::vector<std::string>& cands) const {
        const std::unordered_set<std::string> set(cands.begin(), cands.end());
        Snap s;
        for (const auto& [rowid, r] : rows) {
            if (r.embedding.size() != dim) continue;
            if (doc && r.document_hash != *doc) continue;
            if (!set.empty() && !set.count(r.document_hash)) continue;
            s.r.push_back(&r);
        }
        s.finish(dim);
        return s;
    }
    void removeRow(int64_t rowid, std::vector<Change>& log) {
        auto it = rows.find(rowid);
        byId.erase(it->second.chunk_id);
        log.push_back({false, std::move(it->second)});
        rows.erase(it);
    }
    void addRow(const Rec& rec, std::vector<Change>& log) {
        Row r; static_cast<Rec&>(r) = rec; r.rowid = nextRowid++;
        byId[r.chunk_id] = r.rowid;
        log.push_back({true, r});
        rows.emplace(r.rowid, std::move(r));
    }
};

// ---- the operation stream ---------------------------------------------------------------------------------------------
struct Op {
    enum Kind { Insert, Erase, EraseDocument, Update, Search, SearchBatch, SearchDocuments, SearchPq, SetPq } kind = Insert;
    std::vector<Rec> recs;                          // Insert; Update: recs[0]
    std::string id;                                 // Erase / Update: chunk_id; EraseDocument: document_hash
    std::vector<std::vector<float>> queries;        // the searches
    size_t k = 10;
    float thr = -1.0f;
    std::optional<std::string> doc;
    std::vector<std::string> cands;
    std::map<std::string, std::string> meta;
    bool all = false;
    std::vector<std::vector<float>> luts;           // SearchPq
    bool useCandidates = false;
    std::vector<uint32_t> candidates;
    size_t rerank = 4;
    std::vector<uint8_t> codes; size_t m = 0; std::vector<std::string> pqIds; size_t dim = 0;   // SetPq
    bool repeatedId = false;                        // Insert: some chunk_id occurs twice in recs

    std::string describe() const {
        static const char* names[] = {"insert", "erase", "eraseDocument", "update", "search", "searchBatch", "searchDocuments", "searchPq", "setPq"};
        char buf[256];
        std::snprintf(buf, sizeof buf, "%s recs=%zu id=%s nq=%zu dim=%zu k=%zu thr=%g doc=%s cands=%zu meta=%zu all=%d pqcands=%d/%zu", names[kind],
                      recs.size(), id.c_str(), queries.size(), queries.empty() ? (recs.empty() ? dim : recs[0].embedding.size()) : queries[0].size(),
                      k, static_cast<double>(thr), doc ? doc->c_str() : "-", cands.size(), meta.size(), all ? 1 : 0, useCandidates ? 1 : 0, candidates.size());
        return buf;
    }
};

class OpGenerator {
public:
    explicit OpGenerator(uint64_t seed) : s_(seed * 0x9E3779B97F4A7C15ULL + 0x1234567ULL) {}
    // the shape of a phase: the bounded pools make replacements and re-inserts of deleted ids frequent
    struct Profile {
        std::vector<size_t> dims;
        uint32_t idPool = 8000, docPool = 60;
        size_t ascendingFirst = 300;                // so many inserts get ascending chunk ids, every later one a pool id
        bool tableApi = false;                      // AllMatching only without document_hash / metadata (searchSimilarRows)
        bool l2 = false;                            // vec0 engine: plain searches only
    };
    Profile profile;

    uint64_t next() { s_ += 0x9E3779B97F4A7C15ULL; uint64_t z = s_; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
    uint32_t below(uint32_t n) { return n ? static_cast<uint32_t>(next() % n) : 0; }
    bool chance(uint32_t percent) { return below(100) < percent; }
    float unit() { return static_cast<float>(static_cast<int32_t>(next() & 0xffffff) - 0x800000) / 8388608.0f; }
    std::vector<float> randomVector(size_t dim) { std::vector<float> v(dim); for (auto& x : v) x = unit(); return v; }

    std::string docName(uint32_t d) { char b[24]; std::snprintf(b, sizeof b, "doc%04u", d); return b; }
    std::string poolId() { char b[24]; std::snprintf(b, sizeof b, "c%06u", below(profile.idPool)); return b; }
    std::string freshId() {
        if (ascending_ < profile.ascendingFirst) { char b[24]; std::snprintf(b, sizeof b, "a%08zu", ascending_++); return b; }
        return poolId();
    }
    const Row* liveRow(const HostModel& m, size_t dim) {          // some live row of `dim` (nullptr: none found quickly)
        if (m.rows.empty()) return nullptr;
        for (int tries = 0; tries < 8; ++tries) {
            const int64_t at = static_cast<int64_t>(next() % static_cast<uint64_t>(m.nextRowid));
            auto it = m.rows.lower_bound(at);
            if (it == m.rows.end()) it = m.rows.begin();
            if (dim == 0 || it->second.embedding.size() == dim) return &it->second;
        }
        return nullptr;
    }
    Rec record(const HostModel& m, const std::string& id, size_t dim) {
        Rec r;
        r.chunk_id = id;
        r.document_hash = chance(2) ? std::string() : docName(below(profile.docPool));
        if (!chance(15)) r.metadata["lang"] = below(3) == 0 ? "en" : (below(2) ? "de" : "fr");
        if (chance(50)) r.metadata["kind"] = below(2) ? "code" : "prose";
        const uint32_t what = below(100);
        if (what < 10) {                                          // an exact duplicate of a live row's embedding: ties
            const Row* src = nullptr;
            if (!dups_.empty() && chance(50)) if (const Row* d = m.find(dups_[below(static_cast<uint32_t>(dups_.size()))]); d && d->embedding.size() == dim) src = d;
            if (!src) src = liveRow(m, dim);
            if (src) { r.embedding = src->embedding; dups_.push_back(src->chunk_id); dups_.push_back(id); return r; }
        }
        if (what < 12) { r.embedding.assign(dim, 0.0f); return r; }                      // zero norm
        if (what < 15) {                                          // norm^2 between the fast path's 1e-12 and the record path's 1e-10
            r.embedding.assign(dim, 0.0f);
            r.embedding[below(static_cast<uint32_t>(dim))] = chance(50) ? 5e-6f : -5e-6f;
            return r;
        }
        r.embedding = randomVector(dim);
        return r;
    }
    size_t pickDim() { return profile.dims[below(static_cast<uint32_t>(profile.dims.size()))]; }

    Op insert(const HostModel& m, size_t n) {
        Op op; op.kind = Op::Insert;
        for (size_t i = 0; i < n; ++i) {
            const size_t dim = inserted_ < profile.dims.size() ? profile.dims[inserted_] : pickDim();   // every dimension from the start
            ++inserted_;
            op.recs.push_back(record(m, freshId(), dim));
        }
        if (n >= 2 && chance(35)) {                               // a chunk_id repeated inside the batch: [a, b, a'] ...
            const size_t from = below(static_cast<uint32_t>(n - 1));
            const size_t to = from + 1 + below(static_cast<uint32_t>(n - 1 - from));
            Rec again = record(m, op.recs[from].chunk_id, chance(50) ? op.recs[from].embedding.size() : pickDim());   // ... and across dimensions
            if (chance(40) && again.embedding.size() == op.recs[to].embedding.size() && to != from) again.embedding = op.recs[to].embedding;   // a' equidistant with b
            op.recs.insert(op.recs.begin() + static_cast<std::ptrdiff_t>(to) + 1, again);
            op.repeatedId = true;
        }
        return op;
    }
    Op erase(const HostModel& m) {
        Op op; op.kind = Op::Erase;
        const Row* r = chance(85) ? liveRow(m, 0) : nullptr;
        op.id = r ? r->chunk_id : poolId();                       // (sometimes an id the table does not hold: NotFound)
        return op;
    }
    Op eraseDocument(const HostModel&) { Op op; op.kind = Op::EraseDocument; op.id = docName(below(profile.docPool)); return op; }
    Op update(const HostModel& m) {
        Op op; op.kind = Op::Update;
        const Row* r = chance(90) ? liveRow(m, 0) : nullptr;
        op.id = r ? r->chunk_id : poolId();
        op.recs.push_back(record(m, op.id, r ? r->embedding.size() : pickDim()));
        return op;
    }
    std::vector<float> query(const HostModel& m, size_t dim) {
        const uint32_t what = below(100);
        if (what < 35) {                                          // a live row (often one with a twin): exact ties at the top
            const Row* src = nullptr;
            if (!dups_.empty() && chance(70)) if (const Row* d = m.find(dups_[below(static_cast<uint32_t>(dups_.size()))]); d && d->embedding.size() == dim) src = d;
            if (!src) src = liveRow(m, dim);
            if (src) {
                double n = 0; for (float v : src->embedding) n += static_cast<double>(v) * v;
                if (n > 1e-6) return src->embedding;
            }
        }
        return randomVector(dim);
    }
    void restrictions(Op& op) {
        const uint32_t what = below(100);
        if (what < 30) op.doc = docName(below(profile.docPool + 2));
        if (what >= 20 && what < 55) {
            const uint32_t n = 1 + below(6);
            for (uint32_t i = 0; i < n; ++i) op.cands.push_back(docName(below(profile.docPool + 2)));
            if (op.doc && chance(50)) op.cands.push_back(*op.doc);
        }
    }
    static float threshold(uint32_t pick) { static const float t[] = {-1.0f, -1.0f, 0.0f, 0.05f, 0.3f}; return t[pick % 5]; }
    // One single-query search; `want`: 0 any, 1 document restriction, 2 metadata path, 3 AllMatching, 4 k above the limit
    Op search(const HostModel& m, int want = 0) {
        Op op; op.kind = Op::Search;
        const size_t dim = pickDim();
        op.queries.push_back(query(m, dim));
        op.thr = threshold(below(5));
        static const size_t ks[] = {1, 3, 10, 10, 25, 100, 1024};
        op.k = ks[below(7)];
        if (profile.l2) { if (want == 4 || chance(8)) op.k = 1025 + below(2500); return op; }
        if (want == 0) want = static_cast<int>(below(6));
        if (want == 1) { restrictions(op); if (!op.doc && op.cands.empty()) op.doc = docName(below(profile.docPool)); }
        else if (want == 2) {
            if (!profile.tableApi || chance(70)) { if (chance(40)) restrictions(op); }
            op.meta["lang"] = below(3) == 0 ? "en" : (below(2) ? "de" : "xx");
            if (chance(30)) op.meta["kind"] = "code";
            if (!profile.tableApi && chance(20)) op.all = true;
        } else if (want == 3) {
            op.all = true;
            if (chance(60)) { const uint32_t n = 1 + below(8); for (uint32_t i = 0; i < n; ++i) op.cands.push_back(docName(below(profile.docPool))); }
            if (!profile.tableApi && chance(30)) op.doc = docName(below(profile.docPool));
        } else if (want == 4) op.k = 1025 + below(2500);
        else if (chance(3)) op.queries[0].assign(dim, 0.0f);     // a zero query: InvalidArgument (:4127-4130)
        return op;
    }
    Op searchBatch(const HostModel& m, size_t nq) {
        Op op; op.kind = Op::SearchBatch;
        const size_t dim = pickDim();
        for (size_t i = 0; i < nq; ++i) op.queries.push_back(query(m, dim));
        static const size_t ks[] = {1, 10, 10, 32, 100};
        op.k = ks[below(5)];
        op.thr = threshold(below(5));
        return op;
    }
    Op searchDocuments(const HostModel& m) {
        Op op; op.kind = Op::SearchDocuments;
        op.queries.push_back(query(m, pickDim()));
        static const size_t ks[] = {1, 5, 10, 40, 1024};
        op.k = ks[below(5)];
        op.thr = threshold(below(5));
        if (chance(60)) { const uint32_t n = 1 + below(10); for (uint32_t i = 0; i < n; ++i) op.cands.push_back(docName(below(profile.docPool + 2))); }
        return op;
    }
    // random bytes and random floats: the engine needs no trained quantiser
    Op setPq(const HostModel& m, size_t dim, size_t msub) {
        Op op; op.kind = Op::SetPq; op.dim = dim; op.m = msub;
        for (const auto& [rowid, r] : m.rows) if (r.embedding.size() == dim) op.pqIds.push_back(r.chunk_id);
        for (size_t i = op.pqIds.size(); i > 1; --i) std::swap(op.pqIds[i - 1], op.pqIds[below(static_cast<uint32_t>(i))]);   // index order is not row order
        op.pqIds.push_back("never-inserted");                                            // an indexed id the table never held
        op.codes.resize(op.pqIds.size() * msub);
        for (auto& c : op.codes) c = static_cast<uint8_t>(chance(30) ? below(4) : below(256));   // few distinct codes: equal ADC scores
        return op;
    }
    Op searchPq(const HostModel& m, size_t nq, bool withCandidates) {
        Op op; op.kind = Op::SearchPq;
        const PqIndex& p = m.pqIndex;
        for (size_t i = 0; i < nq; ++i) {
            op.queries.push_back(query(m, p.dim));
            std::vector<float> lut(p.m * 256);
            for (auto& x : lut) x = chance(20) ? 0.25f * static_cast<float>(below(5)) : unit();
            op.luts.push_back(std::move(lut));
        }
        static const size_t ks[] = {1, 10, 20, 100};
        op.k = ks[below(4)];
        op.thr = threshold(below(5));
        op.rerank = 1 + below(8);
        if (withCandidates) {
            op.useCandidates = true;
            const uint32_t n = static_cast<uint32_t>(p.chunk_ids.size());
            const uint32_t want = chance(10) ? 0 : 1 + below(std::min<uint32_t>(n, 3000));
            std::set<uint32_t> pick;
            for (uint32_t i = 0; i < want; ++i) pick.insert(below(n));
            op.candidates.assign(pick.begin(), pick.end());                              // ascending (:3910-3937)
        }
        return op;
    }

private:
    uint64_t s_;
    size_t ascending_ = 0, inserted_ = 0;
    std::vector<std::string> dups_;
};

}  // namespace mirror_model
