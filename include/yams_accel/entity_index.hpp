// entity_index.hpp — IEntityStore (include/yams/vector/entity_store.h:17-39 in the reference) over the
// vector_scan_v1 + vector_entity_scan_v1 vtables.
//
// Mirrors the entity half of SqliteVecBackend (src/vector/sqlite_vec_backend.cpp): insertEntityVector (:2604-2645,
// INSERT OR REPLACE under UNIQUE(node_key, embedding_type), :479-507: the old row goes, the new one takes a fresh rowid at
// the end), deleteEntityVectorsByNode / ByDocument (:2703-2750), searchEntities (:2801-2887).  Everything but the search
// stays host data: the records live here, the embeddings additionally in HBM as one corpus per embedding dimension seen
// (a row whose blob holds another number of floats than the query is skipped, :2858: it lives in another corpus), next to
// the attribute columns the device predicate reads (embedding_type ordinal, interned node_type / document_hash ids).
// Rows are only ever appended to a corpus; a replaced or deleted row becomes a tombstone behind the row mask, and a corpus
// whose tombstones exceed a quarter of its rows is cleared and re-uploaded.
//
// Order of equal similarities: the reference's std::sort leaves it open; this is the rule served: table (rowid) order.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <unordered_map>
#include <vector>

#include "plugin.hpp"

#ifdef YAMS_ACCEL_USE_HOST_TYPES
#include <yams/vector/entity_store.h> // the host's own EntityVectorRecord / EntitySearchParams / IEntityStore
#endif

namespace yams::vector {

#ifndef YAMS_ACCEL_USE_HOST_TYPES
// this repository's own small types for builds outside the YAMS tree: what the adapter reads or fills
enum class EntityEmbeddingType { SIGNATURE, DOCUMENTATION, ALIAS, CONTEXT };

struct EntityVectorRecord {
    int64_t rowid = 0;
    std::string node_key;
    EntityEmbeddingType embedding_type = EntityEmbeddingType::SIGNATURE;
    std::vector<float> embedding;
    std::string content;
    bool is_stale = false;
    float relevance_score = 0.0f;
    std::string node_type;
    std::string document_hash;
};

struct EntitySearchParams {
    size_t k = 10;
    float similarity_threshold = 0.5f;
    std::optional<EntityEmbeddingType> embedding_type;
    std::optional<std::string> node_type;
    std::optional<std::string> document_hash;
    bool include_embeddings = false;
};
#endif

class AccelEntityIndex {
public:
    AccelEntityIndex(std::shared_ptr<accel::Plugin> plugin, yams_vector_scan_v1* vt, yams_vector_entity_scan_v1* evt)
        : plugin_(std::move(plugin)), vt_(vt), evt_(evt) {}
    ~AccelEntityIndex() {
        for (auto& kv : dims_) if (kv.second.corpus) vt_->corpus_destroy(vt_->self, kv.second.corpus);
    }
    AccelEntityIndex(const AccelEntityIndex&) = delete;
    AccelEntityIndex& operator=(const AccelEntityIndex&) = delete;

    Result<void> insertEntityVector(const EntityVectorRecord& record) { return insertEntityVectorsBatch({record}); }
    Result<void> insertEntityVectorsBatch(const std::vector<EntityVectorRecord>& records) {
        std::lock_guard<std::mutex> lk(mu_);
        for (const auto& r : records) {
            const Key key{r.node_key, static_cast<int>(r.embedding_type)};
            auto it = byKey_.find(key);
            if (it != byKey_.end()) kill(it->second);            // INSERT OR REPLACE: the old row goes ...
            Dim& d = dims_[r.embedding.size()];
            d.records.push_back(r);                               // ... the new one takes a fresh rowid at the end
            d.records.back().rowid = ++lastRowid_;
            d.alive.push_back(1);
            byKey_[key] = Loc{r.embedding.size(), d.records.size() - 1};
            intern(nodeTypes_, r.node_type);
            intern(docs_, r.document_hash);
        }
        return {};
    }
    Result<void> deleteEntityVectorsByNode(const std::string& node_key) {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto it = byKey_.begin(); it != byKey_.end();)
            if (it->first.first == node_key) { kill(it->second); it = byKey_.erase(it); } else ++it;
        return {};
    }
    Result<void> deleteEntityVectorsByDocument(const std::string& document_hash) {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto it = byKey_.begin(); it != byKey_.end();)
            if (at(it->second).document_hash == document_hash) { kill(it->second); it = byKey_.erase(it); } else ++it;
        return {};
    }

    // searchEntities (:2801-2887) = one search_entities call (rounds of YAMS_SCAN_MAX_K behind the mask above that: the
    // row-ordinal tie rule makes every round yield exactly the next best rows), ordinals mapped back to the records.
    Result<std::vector<EntityVectorRecord>> searchEntities(const std::vector<float>& query, const EntitySearchParams& params = {}) {
        std::lock_guard<std::mutex> lk(mu_);
        std::vector<EntityVectorRecord> out;
        if (query.empty() || params.k == 0) return out;           // (:2809-2811)
        auto di = dims_.find(query.size());
        if (di == dims_.end()) return out;                        // every row has another size: skipped (:2858)
        Dim& d = di->second;
        yams_scan_entity_filter_t f{0, 0, 0, 0};
        if (params.embedding_type) { f.fields |= YAMS_SCAN_ENTITY_FILTER_TYPE; f.embedding_type = static_cast<uint32_t>(*params.embedding_type); }
        if (params.node_type) {                                   // a string never interned equals no row: no device call
            auto it = nodeTypes_.find(*params.node_type);
            if (it == nodeTypes_.end()) return out;
            f.fields |= YAMS_SCAN_ENTITY_FILTER_NODE_TYPE; f.node_type = it->second;
        }
        if (params.document_hash) {
            auto it = docs_.find(*params.document_hash);
            if (it == docs_.end()) return out;
            f.fields |= YAMS_SCAN_ENTITY_FILTER_DOC; f.doc = it->second;
        }
        if (auto s = sync(d); !s) return s.error();
        if (d.records.empty()) return out;
        const size_t n = d.records.size();
        std::vector<uint32_t> mask;
        if (d.dead || params.k > YAMS_SCAN_MAX_K) {               // tombstones, and the rows earlier rounds returned
            mask.assign((n + 31) / 32, 0u);
            for (size_t r = 0; r < n; ++r) if (d.alive[r]) mask[r >> 5] |= 1u << (r & 31);
        }
        size_t remaining = params.k;
        while (remaining > 0) {
            const uint32_t kk = static_cast<uint32_t>(std::min<size_t>(remaining, YAMS_SCAN_MAX_K));
            yams_scan_hit_t* hits = nullptr; uint32_t* counts = nullptr;
            ++deviceCalls_;
            const yams_status_t st = evt_->search_entities(evt_->self, d.corpus, query.data(), f.fields ? &f : nullptr, 1,
                                                           static_cast<uint32_t>(query.size()), kk, params.similarity_threshold,
                                                           mask.empty() ? nullptr : mask.data(), &hits, &counts, nullptr, nullptr);
            if (st != YAMS_OK) return Error{accel::mapStatus(st), "search_entities failed"};
            const uint32_t got = counts[0];
            for (uint32_t i = 0; i < got; ++i) {
                const size_t row = static_cast<size_t>(hits[i].row);
                out.push_back(d.records[row]);
                out.back().relevance_score = hits[i].similarity;
                if (!params.include_embeddings) out.back().embedding.clear();
                if (!mask.empty()) mask[row >> 5] &= ~(1u << (row & 31));
            }
            evt_->free_entity_hits(evt_->self, hits, counts);
            if (got < kk) break;                                  // nothing left at or above the threshold
            remaining -= got;
        }
        return out;
    }

    Result<std::vector<EntityVectorRecord>> getEntityVectorsByNode(const std::string& node_key) {
        return collect([&](const EntityVectorRecord& r) { return r.node_key == node_key; });
    }
    Result<std::vector<EntityVectorRecord>> getEntityVectorsByDocument(const std::string& document_hash) {
        return collect([&](const EntityVectorRecord& r) { return r.document_hash == document_hash; });
    }
    Result<bool> hasEntityEmbedding(const std::string& node_key) {
        std::lock_guard<std::mutex> lk(mu_);
        for (const auto& kv : byKey_) if (kv.first.first == node_key) return true;
        return false;
    }
    Result<size_t> getEntityVectorCount() { std::lock_guard<std::mutex> lk(mu_); return byKey_.size(); }
    Result<void> markEntityAsStale(const std::string& node_key) {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto& kv : byKey_) if (kv.first.first == node_key) at(kv.second).is_stale = true;
        return {};
    }
    uint64_t deviceCalls() const { return deviceCalls_; }        // search_entities calls made (tests)

private:
    using Key = std::pair<std::string, int>;                      // UNIQUE(node_key, embedding_type)
    struct Loc { size_t dim, row; };
    struct Dim {
        uint64_t corpus = 0;
        std::vector<EntityVectorRecord> records;                  // row r of the corpus (tombstones included)
        std::vector<uint8_t> alive;
        size_t dead = 0, deviceRows = 0;
    };
    EntityVectorRecord& at(const Loc& l) { return dims_[l.dim].records[l.row]; }
    void kill(const Loc& l) {
        Dim& d = dims_[l.dim];
        if (d.alive[l.row]) { d.alive[l.row] = 0; ++d.dead; }
    }
    static void intern(std::unordered_map<std::string, uint32_t>& m, const std::string& s) {
        m.emplace(s, static_cast<uint32_t>(m.size()));
    }
    template <typename Pred> Result<std::vector<EntityVectorRecord>> collect(Pred pred) {
        std::lock_guard<std::mutex> lk(mu_);
        std::vector<EntityVectorRecord> out;
        for (const auto& kv : dims_)
            for (size_t r = 0; r < kv.second.records.size(); ++r)
                if (kv.second.alive[r] && pred(kv.second.records[r])) out.push_back(kv.second.records[r]);
        std::sort(out.begin(), out.end(), [](const EntityVectorRecord& a, const EntityVectorRecord& b) { return a.rowid < b.rowid; });
        return out;
    }
    // Brings the corpus of one dimension up to date: compaction when tombstones exceed a quarter of the rows (corpus_clear +
    // re-append), then the rows appended since the last upload and their attribute columns.
    Result<void> sync(Dim& d) {
        const size_t dim = d.records.empty() ? 0 : d.records.front().embedding.size();
        if (d.records.empty()) return {};
        if (!d.corpus) {
            const yams_status_t st = vt_->corpus_create(vt_->self, static_cast<uint32_t>(dim), &d.corpus);
            if (st != YAMS_OK) return Error{accel::mapStatus(st), "corpus_create failed"};
        }
        if (d.dead > 1024 && d.dead * 4 > d.records.size()) {
            std::vector<EntityVectorRecord> keep;
            keep.reserve(d.records.size() - d.dead);
            for (size_t r = 0; r < d.records.size(); ++r) if (d.alive[r]) keep.push_back(std::move(d.records[r]));
            d.records.swap(keep);
            d.alive.assign(d.records.size(), 1);
            d.dead = 0;
            for (size_t r = 0; r < d.records.size(); ++r)
                byKey_[Key{d.records[r].node_key, static_cast<int>(d.records[r].embedding_type)}] = Loc{dim, r};
            if (vt_->corpus_clear(vt_->self, d.corpus) != YAMS_OK) return Error{ErrorCode::InternalError, "corpus_clear failed"};
            d.deviceRows = 0;
        }
        const size_t first = d.deviceRows, n = d.records.size() - first;
        if (n == 0) return {};
        std::vector<float> flat(n * dim);
        std::vector<uint8_t> types(n);
        std::vector<uint32_t> nodes(n), docs(n);
        for (size_t i = 0; i < n; ++i) {
            const EntityVectorRecord& r = d.records[first + i];
            std::copy(r.embedding.begin(), r.embedding.end(), flat.begin() + i * dim);
            types[i] = static_cast<uint8_t>(r.embedding_type);
            nodes[i] = nodeTypes_.at(r.node_type);
            docs[i] = docs_.at(r.document_hash);
        }
        // (a failed upload leaves the rows pending here: every search fails with that code until one succeeds)
        if (const yams_status_t st = vt_->corpus_append(vt_->self, d.corpus, flat.data(), n); st != YAMS_OK)
            return Error{accel::mapStatus(st), "corpus_append failed"};
        d.deviceRows = d.records.size();
        if (const yams_status_t st = evt_->corpus_set_attributes(evt_->self, d.corpus, first, n, types.data(), nodes.data(), docs.data());
            st != YAMS_OK) {
            d.deviceRows = 0;                                     // the columns are behind the rows: start over next time
            (void)vt_->corpus_clear(vt_->self, d.corpus);
            return Error{accel::mapStatus(st), "corpus_set_attributes failed"};
        }
        return {};
    }

    std::shared_ptr<accel::Plugin> plugin_;
    yams_vector_scan_v1* vt_;
    yams_vector_entity_scan_v1* evt_;
    std::mutex mu_;
    std::map<size_t, Dim> dims_;                                  // one corpus per embedding dimension seen
    std::map<Key, Loc> byKey_;                                    // the live rows
    std::unordered_map<std::string, uint32_t> nodeTypes_, docs_;  // interned filter strings -> column ids
    int64_t lastRowid_ = 0;
    uint64_t deviceCalls_ = 0;
};

inline Result<std::unique_ptr<AccelEntityIndex>> createAccelEntityIndex(std::shared_ptr<accel::Plugin> plugin) {
    auto vt = plugin->getInterface<yams_vector_scan_v1>(YAMS_IFACE_VECTOR_SCAN_V1, 1);
    if (!vt) return vt.error();
    auto evt = plugin->getInterface<yams_vector_entity_scan_v1>(YAMS_IFACE_VECTOR_ENTITY_SCAN_V1, 1);
    if (!evt) return evt.error();
    return std::make_unique<AccelEntityIndex>(std::move(plugin), vt.value(), evt.value());
}

#ifdef YAMS_ACCEL_USE_HOST_TYPES
// The host's own seam: what an entity graph or symbol extractor holds an IEntityStore* to.
class AccelEntityStore final : public IEntityStore {
public:
    explicit AccelEntityStore(std::unique_ptr<AccelEntityIndex> index) : index_(std::move(index)) {}
    Result<void> insertEntityVector(const EntityVectorRecord& record) override { return index_->insertEntityVector(record); }
    Result<void> insertEntityVectorsBatch(const std::vector<EntityVectorRecord>& records) override { return index_->insertEntityVectorsBatch(records); }
    Result<void> deleteEntityVectorsByNode(const std::string& node_key) override { return index_->deleteEntityVectorsByNode(node_key); }
    Result<void> deleteEntityVectorsByDocument(const std::string& document_hash) override { return index_->deleteEntityVectorsByDocument(document_hash); }
    Result<std::vector<EntityVectorRecord>> searchEntities(const std::vector<float>& query_embedding, const EntitySearchParams& params = {}) override {
        return index_->searchEntities(query_embedding, params);
    }
    Result<std::vector<EntityVectorRecord>> getEntityVectorsByNode(const std::string& node_key) override { return index_->getEntityVectorsByNode(node_key); }
    Result<std::vector<EntityVectorRecord>> getEntityVectorsByDocument(const std::string& document_hash) override { return index_->getEntityVectorsByDocument(document_hash); }
    Result<bool> hasEntityEmbedding(const std::string& node_key) override { return index_->hasEntityEmbedding(node_key); }
    Result<size_t> getEntityVectorCount() override { return index_->getEntityVectorCount(); }
    Result<void> markEntityAsStale(const std::string& node_key) override { return index_->markEntityAsStale(node_key); }
private:
    std::unique_ptr<AccelEntityIndex> index_;
};
#endif

} // namespace yams::vector
