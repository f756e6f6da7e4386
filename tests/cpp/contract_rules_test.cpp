// contract_rules_test.cpp — the result contract's rules (yams_amd/csrc/contract_rules.h) held to the CPU oracle, bit for bit.
//
// Plain g++, no GPU, no ROCm include path: the header's functions are the ones the kernels inline.  Linked with
// oracle/_build/libyams_oracle.so, whose C restatement of the reference plays the reference (tests/test_oracle.py and
// tests/test_scan_ref_pin.py pin it to the reference-compiled code).  Inputs are tiny (dim 1-4); every comparison is of bits.
//
//   contract_rules_test           runs every case, prints one line per failure and "OK (0 failures)"
//   contract_rules_test admits    entity_admits for the cases on stdin, one per line:
//                                 "fields embedding_type node_type doc row_type row_node_type row_doc" -> "0" or "1" per line
//                                 (tests/test_contract_rules_cpu.py takes the expectations from tests/_entity_oracle.py)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../yams_amd/csrc/contract_rules.h"

extern "C" {
int oracle_query_invalid(const float* q, size_t dim);
double oracle_cosine_similarity(const float* a, const float* b, size_t dim);
long oracle_exact_scan_cosine(const float* corpus, size_t n_rows, size_t dim, const float* query, size_t k, float similarity_threshold,
                              const uint64_t* tie_rank, int64_t* out_rows, float* out_sims, uint64_t* rows_visited, uint64_t* evaluations);
long oracle_exact_scan_cosine_records(const float* corpus, size_t n_rows, size_t dim, const float* query, size_t k, int all_matching,
                                      float similarity_threshold, const uint64_t* tie_rank, const uint8_t* allow, int64_t* out_rows,
                                      float* out_sims, uint64_t* evaluations);
}

using namespace yams_accel;

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

const float kInf = std::numeric_limits<float>::infinity();
const float kNaN = std::numeric_limits<float>::quiet_NaN();

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
uint64_t bits(double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; }
using Vec = std::vector<float>;

double nsq_of(const Vec& v) {
    double nsq, dot;
    row_sums(v.data(), v.data(), static_cast<uint32_t>(v.size()), &nsq, &dot);
    return nsq;
}

// ---- fp32 vectors whose fp64 sum of squares sits at an edge ------------------------------------------------------------
// Greedy search over at most three free elements (dim 4 puts a fixed small element in front of them): the first runs over
// the floats below sqrt(what is left), the second is the float whose square best fills the rest (two neighbours each side
// tried too), the third likewise (one neighbour each side).  The sums are the rule's own chain.  Returns the vectors whose
// sum is the largest found below the target, equal to it (empty when no combination hits it), and the smallest found above;
// the search ends early once the doubles next to the target and the target itself are all reached.
struct Edge { Vec below, exact, above; double s_below = 0.0, s_above = std::numeric_limits<double>::infinity(); };
Edge find_edge(double target, int dim) {
    Edge e;
    auto consider = [&](const Vec& v) {
        const double s = nsq_of(v);
        if (s < target && s > e.s_below) { e.s_below = s; e.below = v; }
        if (s > target && s < e.s_above) { e.s_above = s; e.above = v; }
        if (s == target && e.exact.empty()) e.exact = v;
    };
    auto step_by = [](float f, int n) { for (int i = 0; i < (n < 0 ? -n : n); ++i) f = std::nextafterf(f, n < 0 ? 0.0f : kInf); return f; };
    const Vec prefix = dim > 3 ? Vec{1e-7f} : Vec{};
    const int n_free = dim - static_cast<int>(prefix.size());
    float x0 = std::nextafterf(static_cast<float>(std::sqrt(target - nsq_of(prefix))), kInf);
    for (int step = 0; step < 4000; ++step, x0 = std::nextafterf(x0, 0.0f)) {
        Vec v = prefix; v.push_back(x0);
        if (n_free == 1) { consider(v); continue; }
        const double left1 = target - nsq_of(v);
        if (left1 <= 0.0) continue;
        for (int dy = -2; dy <= 2; ++dy) {
            Vec w = v; w.push_back(step_by(static_cast<float>(std::sqrt(left1)), dy));
            if (n_free == 2) { consider(w); continue; }
            const double left2 = target - nsq_of(w);
            if (left2 <= 0.0) { w.push_back(0.0f); consider(w); continue; }
            for (int dz = -1; dz <= 1; ++dz) { Vec u = w; u.push_back(step_by(static_cast<float>(std::sqrt(left2)), dz)); consider(u); }
        }
        if (!e.exact.empty() && e.s_below == std::nextafter(target, 0.0) && e.s_above == std::nextafter(target, 1.0)) break;
    }
    return e;
}

// ---- query_flags against oracle_query_invalid ---------------------------------------------------------------------------
void query_case(const char* name, const Vec& q, int want_invalid /* -1: whatever the oracle says */) {
    const uint32_t f = query_flags(nsq_of(q));
    const int ref = oracle_query_invalid(q.data(), q.size());
    CHECK((f != 0) == (ref != 0), "%s: flags %u, oracle %d", name, f, ref);
    if (want_invalid >= 0) CHECK(ref == want_invalid, "%s: oracle %d, the case was built for %d", name, ref, want_invalid);
}

void test_query_flags() {
    query_case("ordinary", {0.5f, -0.25f, 3.0f}, 0);
    query_case("NaN", {1.0f, kNaN, 2.0f}, 1);
    query_case("inf", {1.0f, -kInf}, 1);
    query_case("zero vector", {0.0f, 0.0f, 0.0f, 0.0f}, 1);
    query_case("dim 1", {2.0f}, 0);
    query_case("dim 1 tiny", {1e-6f}, 1);
    CHECK(query_flags(nsq_of({1.0f, kNaN})) == 3u, "NaN sets both bits");
    CHECK(query_flags(nsq_of({kInf})) == 1u, "inf sets bit 0 only");
    CHECK(query_flags(nsq_of({0.0f})) == 2u, "zero sets bit 1 only");
    for (int dim = 1; dim <= 4; ++dim) {
        const Edge e = find_edge(1e-10, dim);
        CHECK(!e.below.empty() && !e.above.empty(), "dim %d: the search found no vector on one side", dim);
        if (e.below.empty() || e.above.empty()) continue;
        CHECK(nsq_of(e.below) < 1e-10 && nsq_of(e.above) > 1e-10, "dim %d: a vector landed on the wrong side", dim);
        std::printf("query edge 1e-10, dim %d: below %.17g (%lld doubles under), exact %s, above %.17g (%lld doubles over)\n", dim, e.s_below,
                    static_cast<long long>(bits(1e-10) - bits(e.s_below)), e.exact.empty() ? "not reachable by this search" : "found", e.s_above,
                    static_cast<long long>(bits(e.s_above) - bits(1e-10)));
        query_case("norm^2 below 1e-10", e.below, 1);
        query_case("norm^2 above 1e-10", e.above, 0);
        if (!e.exact.empty()) query_case("norm^2 == 1e-10", e.exact, 0);
    }
    // three free elements reach 1e-10 itself and the doubles next to it (dims 3 and 4; printed above for dim 3)
    const Edge e4 = find_edge(1e-10, 4);
    CHECK(e4.s_below == std::nextafter(1e-10, 0.0), "dim 4: the largest double below 1e-10 was not reached (%.17g)", e4.s_below);
    CHECK(e4.s_above == std::nextafter(1e-10, 1.0), "dim 4: the smallest double above 1e-10 was not reached (%.17g)", e4.s_above);
    CHECK(!e4.exact.empty(), "dim 4: the double 1e-10 was not reached");
}

// ---- compute_cosine_similarity over row_sums against oracle_cosine_similarity -------------------------------------------
void ccs_case(const char* name, const Vec& row, const Vec& q, const uint32_t* want_bits = nullptr) {
    double nsq, dot;
    row_sums(row.data(), q.data(), static_cast<uint32_t>(row.size()), &nsq, &dot);
    const float got = compute_cosine_similarity(dot, nsq, std::sqrt(nsq_of(q)));
    const float ref = static_cast<float>(oracle_cosine_similarity(q.data(), row.data(), row.size()));
    CHECK(bits(got) == bits(ref), "%s: %08x, oracle %08x", name, bits(got), bits(ref));
    if (want_bits) CHECK(bits(got) == *want_bits, "%s: %08x, built for %08x", name, bits(got), *want_bits);
}

void test_compute_cosine_similarity() {
    const uint32_t zero = 0u, neg_zero = 0x80000000u;
    ccs_case("zero row", {0.f, 0.f, 0.f}, {1.f, 2.f, 3.f}, &zero);
    ccs_case("zero query", {1.f, 2.f, 3.f}, {0.f, 0.f, 0.f}, &zero);
    ccs_case("both zero", {0.f, 0.f}, {0.f, 0.f}, &zero);
    ccs_case("ordinary", {0.3f, -1.25f, 2.0f, 0.125f}, {1.5f, 0.75f, -0.1f, 4.0f});
    ccs_case("ordinary dim 1", {-3.0f}, {0.5f});
    ccs_case("NaN in the row", {1.f, kNaN, 2.f}, {1.f, 1.f, 1.f});
    ccs_case("NaN in the query", {1.f, 1.f, 1.f}, {kNaN, 1.f, 2.f});
    ccs_case("inf in the row", {kInf, 1.f}, {1.f, 1.f});
    ccs_case("-inf in the row", {1.f, -kInf}, {1.f, 1.f});
    ccs_case("inf in the query", {1.f, 1.f}, {1.f, kInf});
    ccs_case("inf against zero", {kInf, 1.f}, {0.f, 1.f});
    ccs_case("inf on both sides", {kInf, 1.f}, {kInf, 1.f});
    // the construction of tests/stress_entity.py: the quotient underflows from below
    ccs_case("-0.0f", {-1e-40f, 1e6f, 0.f, 0.f}, {1.f, 0.f, 0.f, 0.f}, &neg_zero);
}

// ---- the fast-path rule against the oracle's scans of a one-row corpus --------------------------------------------------
// want_kept: -1 = whatever the oracle says.  Returns the score the rule gave (NaN when dropped).
float fast_case(const char* name, const Vec& row, const Vec& q, float thr, bool record_path, int want_kept, const uint32_t* want_bits = nullptr) {
    const uint32_t dim = static_cast<uint32_t>(row.size());
    int64_t out_row = -7; float out_sim = 0.f;
    const long ref = record_path
        ? oracle_exact_scan_cosine_records(row.data(), 1, dim, q.data(), 1, 0, thr, nullptr, nullptr, &out_row, &out_sim, nullptr)
        : oracle_exact_scan_cosine(row.data(), 1, dim, q.data(), 1, thr, nullptr, &out_row, &out_sim, nullptr, nullptr);
    CHECK(query_flags(nsq_of(q)) == 0 && ref >= 0, "%s: the query must be valid", name);
    double nsq, dot, sd = 0.0;
    row_sums(row.data(), q.data(), dim, &nsq, &dot);
    const double qn = std::sqrt(nsq_of(q));
    const uint64_t key = fast_cosine_key(dot, nsq, qn, record_path, thr, 5u);
    // the pieces, as rescore_select_kernel strings them together, must say the same as the whole
    const bool kept = fast_row_scored(nsq, record_path) && fast_quotient(dot, nsq, qn, &sd) && fast_kept(fast_cast(sd), thr);
    CHECK(kept == (key != 0), "%s: the pieces and fast_cosine_key disagree", name);
    CHECK(static_cast<long>(kept) == ref, "%s: kept %d, oracle %ld", name, static_cast<int>(kept), ref);
    if (want_kept >= 0) CHECK(static_cast<int>(kept) == want_kept, "%s: kept %d, the case was built for %d", name, static_cast<int>(kept), want_kept);
    if (!kept || ref != 1) return kNaN;
    const float sim = fast_cast(sd);
    CHECK(bits(sim) == bits(out_sim), "%s: score %08x, oracle %08x", name, bits(sim), bits(out_sim));
    CHECK(bits(exact_cosine_again(row.data(), q.data(), dim, qn)) == bits(out_sim), "%s: exact_cosine_again differs from the oracle", name);
    CHECK(key_idx(key) == 5u && key_score(key) == sim, "%s: the key does not carry the score and the rank", name);
    if (want_bits) CHECK(bits(sim) == *want_bits, "%s: %08x, built for %08x", name, bits(sim), *want_bits);
    return sim;
}

void test_fast_path() {
    const uint32_t neg_zero = 0x80000000u;
    for (int dim = 1; dim <= 4; ++dim) {
        Vec q(dim, 0.25f); q[0] = 1.0f;
        // :4267-4269: norm^2 <= 1e-12 is dropped — the largest value not above the edge goes, the next stays
        const Edge e = find_edge(1e-12, dim);
        CHECK(!e.below.empty() && !e.above.empty(), "dim %d: no vector on one side of 1e-12", dim);
        if (!e.below.empty()) fast_case("norm^2 just below 1e-12", e.below, q, -1.0f, false, 0);
        if (!e.exact.empty()) fast_case("norm^2 == 1e-12", e.exact, q, -1.0f, false, 0);
        if (!e.above.empty()) fast_case("norm^2 just above 1e-12", e.above, q, -1.0f, false, 1);
        // the record path: norm^2 < 1e-10 is dropped — the edge itself stays
        const Edge r = find_edge(1e-10, dim);
        if (!r.below.empty()) fast_case("record path, norm^2 just below 1e-10", r.below, q, -1.0f, true, 0);
        if (!r.exact.empty()) fast_case("record path, norm^2 == 1e-10", r.exact, q, -1.0f, true, 1);
        if (!r.above.empty()) fast_case("record path, norm^2 just above 1e-10", r.above, q, -1.0f, true, 1);
        // between the two edges the paths differ
        Vec mid(dim, 0.0f); mid[0] = 3e-6f;                          // norm^2 = 9e-12
        fast_case("norm^2 9e-12, fast path", mid, q, -1.0f, false, 1);
        fast_case("norm^2 9e-12, record path", mid, q, -1.0f, true, 0);
        if (dim == 4) {
            CHECK(!e.exact.empty() && e.s_below == std::nextafter(1e-12, 0.0) && e.s_above == std::nextafter(1e-12, 1.0),
                  "dim 4: the doubles at and next to 1e-12 were not all reached (%.17g, %.17g)", e.s_below, e.s_above);
        }
    }
    const Vec q{1.0f, 0.5f, -0.25f};
    for (int rp = 0; rp < 2; ++rp) {
        const bool record = rp != 0;
        fast_case("NaN row", {1.0f, kNaN, 1.0f}, q, -1.0f, record, 0);
        fast_case("inf row", {1.0f, kInf, 1.0f}, q, -1.0f, record, 0);
        fast_case("-inf row", {-kInf, 1.0f, 1.0f}, q, -1.0f, record, 0);
        const Vec row{0.75f, -0.5f, 2.0f};
        const float s = fast_case("ordinary", row, q, -1.0f, record, 1);
        fast_case("threshold == score", row, q, s, record, 1);
        fast_case("score one ulp below the threshold", row, q, std::nextafterf(s, kInf), record, 0);
        fast_case("threshold one ulp below the score", row, q, std::nextafterf(s, -kInf), record, 1);
        fast_case("NaN threshold", row, q, kNaN, record, 1);
        fast_case("-0.0f score under threshold +0.0f", {-1e-40f, 1e6f, 0.f}, {1.f, 0.f, 0.f}, 0.0f, record, 1, &neg_zero);
        fast_case("-0.0f score under the smallest denormal", {-1e-40f, 1e6f, 0.f}, {1.f, 0.f, 0.f}, std::numeric_limits<float>::denorm_min(), record, 0);
    }
    // one zero in the keys: equal ranks give the same key, whatever the sign — while the plain key tells them apart
    CHECK(pack_cosine_key(-0.0f, 9u) == pack_cosine_key(0.0f, 9u), "the two zeros must share a cosine key");
    CHECK(pack_key(-0.0f, 9u) < pack_key(0.0f, 9u), "pack_key orders -0.0f below +0.0f");
    CHECK(pack_cosine_key(-0.0f, 8u) > pack_cosine_key(0.0f, 9u), "among zeros the smaller rank wins");
    CHECK(bits(key_score(pack_cosine_key(-0.0f, 1u))) == 0u, "the cosine key holds the canonical zero");
    CHECK(pack_cosine_key(0.5f, 3u) == pack_key(0.5f, 3u) && pack_key(1e-45f, 0u) != 0, "non-zero scores keep their keys; no key is 0");
}

// ---- global_row_id ------------------------------------------------------------------------------------------------------
void test_global_row_id() {
    for (int64_t base : {int64_t{0}, int64_t{7}, int64_t{1} << 33})
        for (uint32_t row : {0u, 1u, 63u, 64u, 200u, 0xffffffffu})
            CHECK(global_row_id(base, 0, 0, 0, row) == base + static_cast<int64_t>(row), "unstriped, base %lld row %u", static_cast<long long>(base), row);
    // striped: stripe t of this shard is stripe t * n_stripes + stripe_index of the corpus
    for (int64_t base : {int64_t{0}, int64_t{7}, int64_t{1} << 33})
        for (uint32_t row : {0u, 63u, 64u, 200u}) {
            const int64_t want = base + (static_cast<int64_t>(row / 64) * 3 + 2) * 64 + row % 64;
            CHECK(global_row_id(base, 64, 3, 2, row) == want, "striped, base %lld row %u: %lld != %lld", static_cast<long long>(base), row,
                  static_cast<long long>(global_row_id(base, 64, 3, 2, row)), static_cast<long long>(want));
        }
    CHECK(global_row_id(0, 64, 3, 2, 0) == 128 && global_row_id(0, 64, 3, 2, 63) == 191 && global_row_id(0, 64, 3, 2, 64) == 320 &&
          global_row_id(0, 64, 3, 2, 200) == 712, "striped: the literal values");
}

// ---- row_allowed --------------------------------------------------------------------------------------------------------
void test_row_allowed() {
    for (uint32_t bit : {0u, 31u, 32u, 63u}) {
        uint32_t only[2] = {0u, 0u}, all_but[2] = {0xffffffffu, 0xffffffffu};
        only[bit >> 5] = 1u << (bit & 31); all_but[bit >> 5] = ~(1u << (bit & 31));
        for (uint32_t row = 0; row < 64; ++row) {
            CHECK(row_allowed(only, row) == (row == bit), "mask with bit %u only, row %u", bit, row);
            CHECK(row_allowed(all_but, row) == (row != bit), "mask without bit %u, row %u", bit, row);
        }
    }
}

// ---- write_empty_slot ---------------------------------------------------------------------------------------------------
void test_write_empty_slot() {
    const uint32_t guard32 = 0xa5a5a5a5u;
    const int64_t guard64 = 0x5a5a5a5a5a5a5a5all;
    for (int combo = 0; combo < 8; ++combo) {
        uint32_t scores[3], dist[3], ranks[3], docs[3];               // floats kept as bits: the guards are not numbers
        int64_t rows[3];
        for (int i = 0; i < 3; ++i) { scores[i] = dist[i] = ranks[i] = docs[i] = guard32; rows[i] = guard64; }
        const bool wd = combo & 1, wr = combo & 2, wc = combo & 4;
        write_empty_slot(1, reinterpret_cast<float*>(scores), rows, wd ? reinterpret_cast<float*>(dist) : nullptr, wr ? ranks : nullptr,
                         wc ? docs : nullptr);
        CHECK(scores[1] == 0xff800000u && rows[1] == -1, "combo %d: score -inf and row -1", combo);
        CHECK(dist[1] == (wd ? 0x7f800000u : guard32), "combo %d: distance +inf iff given", combo);
        CHECK(ranks[1] == (wr ? 0xffffffffu : guard32), "combo %d: rank 0xffffffff iff given", combo);
        CHECK(docs[1] == (wc ? YAMS_SCAN_NO_DOC : guard32), "combo %d: document NO_DOC iff given", combo);
        for (int i = 0; i < 3; i += 2)
            CHECK(scores[i] == guard32 && dist[i] == guard32 && ranks[i] == guard32 && docs[i] == guard32 && rows[i] == guard64,
                  "combo %d: the neighbours of the slot stay as they were", combo);
    }
}

int admits_from_stdin() {
    unsigned fields, et, nt, doc, rt, rn, rd;
    while (std::scanf("%u %u %u %u %u %u %u", &fields, &et, &nt, &doc, &rt, &rn, &rd) == 7) {
        yams_scan_entity_filter_t f{};
        f.fields = fields; f.embedding_type = static_cast<decltype(f.embedding_type)>(et); f.node_type = nt; f.doc = doc;
        // the row sits at ordinal 2 of its columns: the function indexes them
        const uint8_t row_type[3] = {static_cast<uint8_t>(~rt), static_cast<uint8_t>(~rt), static_cast<uint8_t>(rt)};
        const uint32_t row_node[3] = {~rn, ~rn, rn}, row_doc[3] = {~rd, ~rd, rd};
        std::printf("%d\n", entity_admits(f, row_type, row_node, row_doc, 2) ? 1 : 0);
    }
    return 0;
}

} // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "admits") == 0) return admits_from_stdin();
    test_query_flags();
    test_compute_cosine_similarity();
    test_fast_path();
    test_global_row_id();
    test_row_allowed();
    test_write_empty_slot();
    std::printf("%s (%d failures)\n", g_failures ? "FAILED" : "OK", g_failures);
    return g_failures ? 1 : 0;
}
