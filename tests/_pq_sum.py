"""The 25 orders of the product-quantised engine's ADC sum (YAMS_PQ_SUM_* in include/yams_mi355x_accel.h), restated in numpy:
the expected values of the device tests (tests/test_pq_sum_orders_gpu.py, tests/stress_pq_sum.py) and of the host probe's
tests (tests/test_pq_calibration_cpu.py).  Written from the header's text, not from the kernels or from pq_calibration.hpp:
  * adc_scores / adc_sum: one definition over many codes at once (every numpy operation is one IEEE fp32 add per element);
  * tree: the same definition as an expression tree over element indices — two definitions are the same FUNCTION at a given m
    exactly when their trees are equal (additions of a zero partial sum dropped, operands unordered: fp32 add commutes);
  * pq_search_flags: simeonPqSearchUnlocked (sqlite_vec_backend.cpp:3868-4056) with the sum pluggable;
  * probes / probe_codes: pq_calibration.hpp's probe generator (a 64-bit LCG), regenerated bit for bit;
  * make_case / discriminates: corpora on which the ORDER of the sum decides which rows are returned.
"""
import numpy as np

SEQ, X4, X8, X16 = 0, 1, 2, 3
LANES_MASK = 3
LTR, HALVES, PAIRS, HALVES4_PAIRS = 0 << 2, 1 << 2, 2 << 2, 3 << 2
COMBINE_MASK = 3 << 2
TAIL_SCALAR = 1 << 4
ORDER_MASK = 0x1F


def lanes(flags):
    return {SEQ: 1, X4: 4, X8: 8, X16: 16}[flags & LANES_MASK]


def definitions():
    """The 25 flag words in preference order: fewer lanes first, then the combine (left to right first), then no tail bit first."""
    out = [SEQ]
    for l in (X4, X8, X16):
        for c in (LTR, HALVES, PAIRS, HALVES4_PAIRS):
            for t in (0, TAIL_SCALAR):
                out.append(l | c | t)
    return out


def name(flags):
    if lanes(flags) == 1:
        return "seq"
    s = "x%d" % lanes(flags)
    s += {LTR: "", HALVES: "_halves", PAIRS: "_pairs", HALVES4_PAIRS: "_halves4_pairs"}[flags & COMBINE_MASK]
    return s + ("_tail" if flags & TAIL_SCALAR else "")


def by_name(nm):
    return {name(f): f for f in definitions()}[nm]


def _reduce(flags, m, zero, leaf, add):
    """The definition over abstract values: zero, leaf(j) and add(a, b)."""
    L = lanes(flags)
    if L == 1:
        s = zero
        for j in range(m):
            s = add(s, leaf(j))
        return s
    body = (m // L) * L if flags & TAIL_SCALAR else m
    p = [zero] * L
    for j in range(body):
        p[j % L] = add(p[j % L], leaf(j))
    comb = flags & COMBINE_MASK
    if comb == LTR:
        s = zero
        for l in range(L):
            s = add(s, p[l])
    elif comb == HALVES:
        w = L // 2
        while w >= 1:
            for l in range(w):
                p[l] = add(p[l], p[l + w])
            w //= 2
        s = p[0]
    elif comb == PAIRS:
        w = L
        while w > 1:
            p = [add(p[2 * l], p[2 * l + 1]) for l in range(w // 2)]
            w //= 2
        s = p[0]
    else:
        while len(p) > 4:
            h = len(p) // 2
            p = [add(p[l], p[l + h]) for l in range(h)]
        s = add(add(p[0], p[1]), add(p[2], p[3]))
    for j in range(body, m):
        s = add(s, leaf(j))
    return s


def table_values(lut, codes):
    """fp32 [n][m]: lut[j][codes[i][j]]."""
    lut = np.asarray(lut, np.float32)
    codes = np.asarray(codes, np.uint8)
    return lut[np.arange(codes.shape[1])[None, :], codes]


def adc_scores(flags, lut, codes, vals=None):
    """fp32 [n]: the sum of lut[j][codes[i][j]] over j under the definition `flags`, for every code i (vals: table_values(lut,
    codes), if the caller has them)."""
    if vals is None:
        vals = table_values(lut, codes)
    n, m = vals.shape
    zero = np.zeros(n, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = _reduce(flags, m, zero, lambda j: vals[:, j], lambda a, b: (a + b).astype(np.float32))
    assert s.dtype == np.float32
    return s


def adc_sum(flags, table, code):
    return adc_scores(flags, np.asarray(table, np.float32).reshape(-1, 256), np.asarray(code, np.uint8)[None, :])[0]


def tree(flags, m):
    """The definition at this m as a hashable expression tree.  x + 0 is x (exact for every x but -0.0); a + b is b + a."""
    def add(a, b):
        if a is None:
            return b
        if b is None:
            return a
        return frozenset((a, b)) if a != b else (a, b)
    return _reduce(flags, m, None, lambda j: j, add)


def classes(m):
    """The definitions grouped into the classes that are one function at this m, each in preference order."""
    groups = {}
    for f in definitions():
        groups.setdefault(tree(f, m), []).append(f)
    return list(groups.values())


def class_of(flags, m):
    t = tree(flags, m)
    return [f for f in definitions() if tree(f, m) == t]


# ---- the whole pipeline -----------------------------------------------------------------------------------------------------
def exact_sims(corpus, query):
    """VectorDatabase::computeCosineSimilarity(query, row) for every row: fp64, sequential over the elements, rounded to fp32."""
    a = query.astype(np.float64)
    b = corpus.astype(np.float64)
    dp = np.zeros(corpus.shape[0]); na = 0.0; nb = np.zeros(corpus.shape[0])
    for i in range(corpus.shape[1]):
        dp = dp + a[i] * b[:, i]
        na = na + a[i] * a[i]
        nb = nb + b[:, i] * b[:, i]
    na = np.sqrt(na); nb = np.sqrt(nb)
    with np.errstate(divide="ignore", invalid="ignore"):
        sim = np.where((na == 0) | (nb == 0), 0.0, dp / (na * nb))
    return sim.astype(np.float32)


def pq_search_flags(corpus, codes, lut, query, k, thr, rerank_factor, tie_keys=None, row_of_index=None, chunk_rank=None,
                    candidates=None, flags=SEQ, sims=None, vals=None, n_items=None):
    """simeonPqSearchUnlocked with the ADC sum of `flags`: (rows, similarities).  A code whose score is not a number is left
    out (it sorts nowhere in the reference's comparator).  `sims`: exact_sims(corpus, query), `vals`: table_values(lut, codes[candidates]), if the caller has them.
    n_items: the length of the candidate list approxK is cut to, when `candidates` is only the part of it that can_reach()."""
    n, m = codes.shape
    if k == 0 or n == 0 or not float((query.astype(np.float64) ** 2).sum()) > 1e-20:
        return [], []
    idxs = np.arange(n, dtype=np.int64) if candidates is None else np.asarray(candidates, np.int64)
    if idxs.size == 0:
        return [], []
    approx = min(idxs.size if n_items is None else n_items, max(k, k * max(1, rerank_factor)))
    sc = adc_scores(flags, lut, codes[idxs] if vals is None else None, vals)
    ok = ~np.isnan(sc)
    idxs, sc = idxs[ok], sc[ok]
    tie = np.asarray(tie_keys, np.uint64)[idxs] if tie_keys is not None else idxs.astype(np.uint64)
    order = np.lexsort((idxs, tie, -sc.astype(np.float64)))[:approx]
    if sims is None:
        sims = exact_sims(corpus, query)
    recs = []
    for i in idxs[order]:
        row = int(row_of_index[i]) if row_of_index is not None else int(i)
        if row >= corpus.shape[0]:
            continue
        sim = sims[row]
        if sim < np.float32(thr):
            continue
        recs.append((-float(sim), int(chunk_rank[row]) if chunk_rank is not None else row, row, sim))
    recs.sort()
    recs = recs[:k]
    return [r[2] for r in recs], [r[3] for r in recs]


# ---- pq_calibration.hpp's probes ---------------------------------------------------------------------------------------------
PROBE_TABLES, CODES_PER_TABLE = 8, 16
_MASK64 = (1 << 64) - 1


class _Lcg:
    def __init__(self, seed):
        self.s = seed & _MASK64

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & _MASK64
        return self.s >> 33


def probes(m):
    """[(table fp32 [m][256], code u8 [m])]: 8 tables x 16 codes, the draws in the header's order."""
    g = _Lcg(0x9E3779B97F4A7C15 ^ ((m * 0xD1B54A32D192ED03) & _MASK64))
    out = []
    for _ in range(PROBE_TABLES):
        tab = np.empty(m * 256, np.float32)
        for i in range(m * 256):
            u = np.float32(g.next() & 0xFFFFFF) / np.float32(16777216.0) - np.float32(0.5)
            tab[i] = u * np.float32(2.0 ** (int(g.next() % 6) - 3))
        tab = tab.reshape(m, 256)
        for _ in range(CODES_PER_TABLE):
            out.append((tab, np.array([g.next() & 255 for _ in range(m)], np.uint8)))
    return out


def probe_codes(m):
    g = _Lcg(0xC2B2AE3D27D4EB4F ^ ((m * 0xD1B54A32D192ED03) & _MASK64))
    return [np.array([g.next() & 255 for _ in range(m)], np.uint8) for _ in range(PROBE_TABLES * CODES_PER_TABLE)]


# ---- corpora on which the order of the sum decides the result ------------------------------------------------------------------
HOT = 64      # centroid ids 256 - HOT .. 255 hold the family's values: positive, the upper three of the six binades


class Case:
    pass


def make_case(seed, m, n, family, nq, k, rf, dim=8, n_rows=1024, with_maps=False, n_cand=None):
    """An index of n codes: n - family random ones, and a family of permutations of one base code, put at random places.
    Every query's table has equal rows across j (lut[j][c] = v[c]; |v| spread over six binades, signs and binades shared by
    the queries, mantissas their own), so the members of the family have the SAME sum in exact arithmetic — far above the
    random codes', since the base code's bytes name the HOT centroids — and the approxK cut runs through the family: the
    rounding alone, that is the order of the additions, decides which members are re-ranked.  The corpus rows are random;
    with rerank_factor 1 every shortlisted row is returned, with 2 the better half.  with_maps: tie keys, an index -> row
    map with lost rows, a chunk-id ranking; n_cand: a candidate list of that many indices that holds the whole family."""
    rng = np.random.default_rng(seed)
    c = Case()
    c.seed, c.m, c.n, c.family, c.nq, c.k, c.rf, c.dim = seed, m, n, family, nq, k, rf, dim
    sign = np.where(rng.random(256) < 0.5, -1.0, 1.0)
    expo = rng.integers(-3, 3, 256)
    sign[256 - HOT:] = 1.0
    expo[256 - HOT:] = rng.integers(0, 3, HOT)
    mant = 0.5 + rng.integers(0, 1 << 23, (nq, 256)) / float(1 << 24)                    # [0.5, 1): 24-bit mantissas
    v = (sign * np.exp2(expo) * mant).astype(np.float32)                                  # exact in fp32
    c.luts = np.ascontiguousarray(np.repeat(v[:, None, :], m, axis=1))                    # [nq][m][256]
    c.codes = rng.integers(0, 256, (n, m)).astype(np.uint8)
    base = rng.integers(256 - HOT, 256, m).astype(np.uint8)
    c.members = np.sort(rng.choice(n, family, replace=False))
    for i in c.members:
        c.codes[i] = base[rng.permutation(m)]
    c.corpus = rng.standard_normal((n_rows, dim)).astype(np.float32)
    c.queries = rng.standard_normal((nq, dim)).astype(np.float32)
    c.keys = c.roi = c.rank = c.cand = None
    if with_maps:
        c.keys = rng.integers(0, 1 << 63, n, dtype=np.uint64)
        c.keys[c.members[::7]] = c.keys[c.members[0]]                                     # equal tie keys: the index decides
        c.rank = rng.permutation(n_rows).astype(np.uint32)
    c.roi = rng.integers(0, n_rows, n).astype(np.uint32)                                  # many codes per row
    if with_maps:
        c.roi[rng.random(n) < 0.02] = n_rows + 5                                          # rows the table lost
    if n_cand is not None:
        others = np.setdiff1d(np.arange(n), c.members)
        c.cand = np.sort(np.concatenate([c.members, rng.choice(others, n_cand - family, replace=False)])).astype(np.uint32)
    c.thr = -1.0
    c._sims, c._vals = None, {}
    return c


def can_reach(vals, approx):
    """Which codes can be among the best `approx` under ANY order of the additions (finite tables).  Any fp32 summation of
    the m values v_j is within B = g * sum |v_j| of the exact sum, g = (m - 1) u / (1 - (m - 1) u), u = 2^-24 (Higham,
    Accuracy and Stability of Numerical Algorithms, 4.2: the bound holds for every order).  With e the exact sum (fp64 holds
    it to far below B; B is doubled for that) a code's score lies in [e - B, e + B] under every definition; at least `approx`
    codes score >= T, the approx-th largest e - B, so a code with e + B < T is in nobody's shortlist."""
    n, m = vals.shape
    if n <= approx:
        return np.ones(n, bool)
    v64 = vals.astype(np.float64)
    e = v64.sum(axis=1)
    u = 2.0 ** -24
    b = 2.0 * ((m - 1) * u / (1 - (m - 1) * u)) * np.abs(v64).sum(axis=1) + 1e-300
    t = np.partition(e - b, n - approx)[n - approx]
    return e + b >= t


def expected(case, flags, queries=None, prune=True):
    """[(rows, sims)] per query under the definition `flags`.  prune: score only the codes that can_reach() the shortlist."""
    if case._sims is None:
        case._sims = [exact_sims(case.corpus, q) for q in case.queries]
    idxs = np.arange(case.n) if case.cand is None else case.cand.astype(np.int64)
    approx = min(idxs.size, max(case.k, case.k * max(1, case.rf)))
    out = []
    for qi in (range(case.nq) if queries is None else queries):
        if (qi, prune) not in case._vals:
            vals = table_values(case.luts[qi], case.codes[idxs])
            keep = can_reach(vals, approx) if prune else np.ones(idxs.size, bool)
            case._vals[(qi, prune)] = (idxs[keep], np.ascontiguousarray(vals[keep]))
        sub, vals = case._vals[(qi, prune)]
        out.append(pq_search_flags(case.corpus, case.codes, case.luts[qi], case.queries[qi], case.k, case.thr, case.rf, case.keys,
                                   case.roi, case.rank, sub, flags, case._sims[qi], vals, idxs.size))
    return out


# ---- the scripted cases of tests/test_pq_sum_orders_gpu.py (test_pq_calibration_cpu.py holds each to discriminates()) -----------
UNFILTERED_M = (32, 40, 7, 100, 128)
FILTERED_M = (32, 40)


def unfiltered_case(m):
    """2048 codes, a family of 512, 5 queries (a partial query group), k = 256, rerank factor 1: approxK 256 cuts the family."""
    return make_case(1000 + m, m, 2048, 512, 5, 256, 1)


def filtered_case(m):
    """70 000 random codes and a family of 400 on top (the filtered form starts at 65 536), 9 queries, k = 100, rerank factor 2."""
    return make_case(2000 + m, m, 70_400, 400, 9, 100, 2)


COMBINED_FLAGS = X8 | HALVES | TAIL_SCALAR


def combined_case():
    """candidates + tie keys + an index -> row map with lost rows + a chunk-id ranking, m = 40 under x8_halves_tail."""
    return make_case(3000, 40, 6000, 300, 6, 120, 1, with_maps=True, n_cand=2500)


def discriminates(case, flags, cache=None):
    """True when the rows expected under `flags` differ, on at least one query, from the rows expected under EVERY definition
    that is another function at this m.  cache: {representative flags: expected(...)}, shared between calls on one case."""
    cache = {} if cache is None else cache

    def rows_of(f):
        rep = class_of(f, case.m)[0]
        if rep not in cache:
            cache[rep] = [r for r, _ in expected(case, rep)]
        return cache[rep]
    mine = rows_of(flags)
    own = tree(flags, case.m)
    for cls in classes(case.m):
        if tree(cls[0], case.m) == own:
            continue
        if rows_of(cls[0]) == mine:
            return False
    return True


OVERFLOW_FLAGS = (SEQ, X4 | HALVES, X4 | PAIRS, X8 | HALVES | TAIL_SCALAR, X16 | HALVES4_PAIRS)


def overflow_case():
    """m = 8; centroid 255 of sub-quantisers 0, 1 holds +3e38 and of 2, 3 holds -3e38.  The 40 codes that name it there sum to
    +inf sequentially (3e38 + 3e38 overflows and stays), to a finite number where the lanes meet as halves (3e38 - 3e38
    first), and to inf - inf = NaN where neighbours meet first (x4 pairs): those rows are left out."""
    c = make_case(4000, 8, 3000, 40, 3, 50, 2)
    rng = np.random.default_rng(4001)
    c.luts = (rng.standard_normal((c.nq, 8, 256)) * 0.5).astype(np.float32)
    c.luts[:, 0:2, 255] = np.float32(3e38)
    c.luts[:, 2:4, 255] = np.float32(-3e38)
    c.codes = rng.integers(0, 255, (c.n, 8)).astype(np.uint8)               # (255 nowhere ...)
    c.codes[c.members, :4] = 255                                            # (... but in the family's first four bytes)
    c._vals = {}
    return c
