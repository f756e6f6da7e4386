"""Score edges of the exact scan, shared by tests/stress_small.py, tests/test_score_edges_cpu.py and
tests/test_score_edges_gpu.py (numpy only):

  zero_plateau     a corpus whose top-k cut runs through a plateau of similarities that are +0.0f and -0.0f.  The reference
                   orders with FLOAT compares (sqlite_vec_backend.cpp:4218-4223, :4296-4298, :100-120): the two zeros are one
                   score and the chunk id (tie rank) decides; an order by the bits of the score puts every +0.0 first.
  packed_key_order what such an order by bits returns for an oracle answer: the restatement of the fault, to prove on the
                   CPU that a case tells the two apart.
  restated_path    the contract stated at yams_scan_diag_t.path (include/yams_mi355x_accel.h) restated: which calls the
                   fused one-launch scan answers; restated_diag_path: the value of diag.path itself, which is 1 for the
                   exhaustive multi-launch pipeline too.
  compare          a device answer against the oracle's, query by query: None or the first difference.
"""
import numpy as np

SCAN_COSINE, SCAN_L2 = 0, 1
# include/yams_mi355x_accel.h, YAMS_SCAN_FLAG_* (restated: this module imports nothing of the product)
FLAG_DEFER_THRESHOLD, FLAG_FORCE_EXACT, FLAG_F32_FILTER, FLAG_SPLIT_FILTER, FLAG_RECORD_PATH = 1, 2, 4, 8, 16
FLAG_WIDE_TILE, FLAG_NO_I8_FILTER, FLAG_RESIDENT_QUERIES = 32, 64, 128
FLAG_L2_ACC_MASK = 768
_TIER_OR_EXACT = FLAG_FORCE_EXACT | FLAG_F32_FILTER | FLAG_SPLIT_FILTER | FLAG_WIDE_TILE | FLAG_NO_I8_FILTER | FLAG_RESIDENT_QUERIES

TINY = np.float32(1e-30)
DENORM_MIN = float(np.float32(1e-45))     # the smallest positive denormal: a threshold that drops both zeros


def restated_path(n, dim, nq, k, metric, flags, aligned=True):
    """1 when the fused one-launch scan answers the call, else 0 (the rule stated at yams_scan_diag_t.path)."""
    if not (1 <= n <= 16384 and nq <= 16):
        return 0
    if dim % 32 != 0 or dim > 1024 or not aligned:
        return 0
    if k > 256 or -(-n // 256) * min(k, 256) > 1024:
        return 0
    if flags & _TIER_OR_EXACT:
        return 0
    if metric == SCAN_L2 and (flags & FLAG_L2_ACC_MASK):
        return 0
    return 1


def restated_diag_path(n, n_allowed, dim, nq, k, metric, flags, aligned=True):
    """yams_scan_diag_t.path as the header states it: 1 when every allowed row is scored in fp64 — by the fused scan, or
    by the exhaustive pipeline (FORCE_EXACT, fewer than 4096 rows, rows not 16-byte aligned or dim % 4 != 0, an allow-mask
    that admits fewer than 16384 rows; n_allowed is None without a mask) — else 0.  (Queries whose norm is outside
    [1e-15, 1e15) under L2 are not modelled: no caller here draws one.)"""
    if restated_path(n, dim, nq, k, metric, flags, aligned):
        return 1
    if (flags & FLAG_FORCE_EXACT) or not aligned or dim % 4 != 0 or n < 4096:
        return 1
    if n_allowed is not None and n_allowed < 16384:
        return 1
    return 0


def zero_plateau(seed, n, dim, nq, k, P, Z, row_order=False):
    """Query j = e_{2j} + 1e-30 e_{2j+1}.  P rows have a positive similarity with every query; Z rows have x_{2j} = 0 and
    x_{2j+1} = s 1e-30, s in {-1, 0, +1} drawn per row (the dot is s 1e-60: the fp64 quotient becomes -0.0f or +0.0f in the
    cast to float), their other coordinates random — distinct norms, one score; every other row has similarity <= -0.05.
    tie_rank is a seeded permutation of the rows in which, inside the plateau, -0.0 rows hold the best rank, the best rank
    behind the cut and — drawn — most of the others, while a +0.0 row sits right behind each of the two: both signs occur
    inside the returned k and outside it, and an order by score BITS returns a different row set.  Needs P <= k - 2,
    Z >= k - P + 2 (for exactly that), n >= P + Z, dim >= 2 nq + 1.  row_order=True: the tie rank of a row is its ordinal
    (callers without rank tables) and the plateau's signs follow the row order instead.

    Returns dict(corpus, queries, tie_rank, positives, plateau (rows in rank order), neg_zero (bool per plateau row))."""
    c = k - P
    assert 0 <= P and c >= 2 and Z >= c + 2 and n >= P + Z and dim >= 2 * nq + 1 and nq >= 1, (n, dim, nq, k, P, Z)
    rng = np.random.default_rng([seed, n, dim, nq, k, P, Z])
    rest = dim - 2 * nq
    corpus = np.zeros((n, dim), np.float32)
    # negatives everywhere first: x_{2j} = -u_j, u in [0.5, 1]; the rest uniform / sqrt(rest): |x| <= sqrt(nq + 1), so the
    # similarity -u_j / |x| is <= -0.5 / sqrt(17) = -0.12 for nq <= 16
    corpus[:, 0:2 * nq:2] = -rng.uniform(0.5, 1.0, (n, nq)).astype(np.float32)
    corpus[:, 2 * nq:] = (rng.uniform(-1.0, 1.0, (n, rest)) / np.sqrt(rest)).astype(np.float32)
    special = rng.choice(n, P + Z, replace=False)          # spread over the whole corpus: every workgroup holds some
    positives, plateau = special[:P], special[P:]
    if row_order:
        plateau = np.sort(plateau)
    corpus[positives, 0:2 * nq:2] = rng.uniform(0.1, 1.0, (P, nq)).astype(np.float32)
    corpus[plateau, 0:2 * nq:2] = 0.0
    # signs along the plateau's rank order: position 0 and c are -0.0, 1 and c + 1 are +0.0, the others drawn
    sign = rng.choice([-1, -1, 0, 1], Z)
    sign[[0, c]] = -1
    sign[1] = rng.choice([0, 1]); sign[c + 1] = rng.choice([0, 1])
    for j in range(nq):
        corpus[plateau, 2 * j + 1] = sign.astype(np.float32) * TINY
    # distinct norms along the plateau (a plateau of one score, not of one row)
    corpus[plateau, 2 * nq] = (1.0 + np.arange(Z) * 0.5).astype(np.float32)
    queries = np.zeros((nq, dim), np.float32)
    for j in range(nq):
        queries[j, 2 * j] = 1.0
        queries[j, 2 * j + 1] = TINY
    tie_rank = np.arange(n, dtype=np.uint32) if row_order else rng.permutation(n).astype(np.uint32)
    tie_rank[plateau] = np.sort(tie_rank[plateau])         # plateau[i] holds the i-th best rank of the plateau
    return {"corpus": corpus, "queries": queries, "tie_rank": tie_rank, "positives": positives, "plateau": plateau,
            "neg_zero": sign < 0}


def f2ord(bits):
    """The order-preserving key of a float's bits (yams_amd/csrc/common.h f2ord), vectorised over uint32."""
    bits = np.asarray(bits, np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def packed_key_order(rows, sims, ranks, k):
    """What an order by (bits of the score desc, tie rank asc) keeps of the scored rows (rows / sims / ranks: every row
    that passed the threshold, any order): the first k rows and scores.  +0.0f sorts above -0.0f there."""
    rows, sims, ranks = np.asarray(rows), np.asarray(sims, np.float32), np.asarray(ranks, np.uint64)
    key = (f2ord(sims.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - ranks)
    o = np.argsort(key)[::-1][:k]
    return rows[o], sims[o]


def compare(counts, rows, scores, dist, rows_visited, expected, k, metric, expect_visited, row_map=None):
    """counts [nq], rows / scores / dist [nq][k] (dist may be None under cosine) and diag.rows_visited of one call against
    `expected` = per query (rows, sims, dist | None) of the oracle.  row_map: oracle row -> the id the caller sees.
    Per query: the count, the rows in order, the score bits (under L2 the distance bits too), the padding behind the count
    (-1, -inf, +inf); then rows_visited.  None, or a short description of the first difference."""
    for qi, e in enumerate(expected):
        e_rows, e_sims, e_dist = e
        e_rows = np.asarray(e_rows, np.int64)
        if row_map is not None:
            e_rows = np.asarray(row_map(e_rows), np.int64)
        c = int(counts[qi])
        if c != len(e_rows):
            return "q%d: count %d != %d" % (qi, c, len(e_rows))
        got = np.asarray(rows[qi, :c], np.int64)
        if not np.array_equal(got, e_rows):
            i = int(np.flatnonzero(got != e_rows)[0])
            return "q%d: row[%d] %d != %d" % (qi, i, got[i], e_rows[i])
        gb, eb = np.asarray(scores[qi, :c], np.float32).view(np.uint32), np.asarray(e_sims, np.float32).view(np.uint32)
        if not np.array_equal(gb, eb):
            i = int(np.flatnonzero(gb != eb)[0])
            return "q%d: score bits[%d] %08x != %08x" % (qi, i, gb[i], eb[i])
        if metric == SCAN_L2:
            gd, ed = np.asarray(dist[qi, :c], np.float32).view(np.uint32), np.asarray(e_dist, np.float32).view(np.uint32)
            if not np.array_equal(gd, ed):
                i = int(np.flatnonzero(gd != ed)[0])
                return "q%d: distance bits[%d] %08x != %08x" % (qi, i, gd[i], ed[i])
        if c < k:
            if not (np.asarray(rows[qi, c:k]) == -1).all():
                return "q%d: padding of rows behind %d" % (qi, c)
            if not np.isneginf(np.asarray(scores[qi, c:k])).all():
                return "q%d: padding of scores behind %d" % (qi, c)
            if dist is not None and not np.isposinf(np.asarray(dist[qi, c:k])).all():
                return "q%d: padding of distances behind %d" % (qi, c)
    if int(rows_visited) != int(expect_visited):
        return "rows_visited %d != %d" % (int(rows_visited), int(expect_visited))
    return None


# The scripted zero-plateau shapes of tests/test_score_edges_gpu.py (n, dim, nq, k, P, Z), by the path they are for;
# tests/test_score_edges_cpu.py proves from the oracle alone that each of them tells the two orders apart.
SCRIPTED = {
    "fused_nq1": (3000, 64, 1, 50, 20, 200),
    "fused_nq5": (3000, 64, 5, 50, 20, 200),
    "general": (20000, 64, 3, 50, 20, 200),
    "general_wide_plateau": (20000, 64, 3, 50, 20, 5000),   # wider than the re-score's 2048 slots and the candidate lists
    "int8": (20000, 256, 3, 50, 20, 200),
    "doc": (2000, 32, 2, 50, 20, 200),
    "pq": (100, 32, 2, 50, 20, 60),                         # n_codes <= k * rerank_factor: everything is shortlisted
    "sharded": (24000, 256, 3, 50, 20, 200),
}


def discriminates(oracle, z, k, thr=-1.0):
    """None when, for every query of the zero-plateau case z, zeros of both signs occur inside the oracle's top k and
    behind it, and the order by score bits keeps a different row SET; else what is missing."""
    n = z["corpus"].shape[0]
    rank = z["tie_rank"].astype(np.uint64)
    for qi, q in enumerate(z["queries"]):
        rows, sims, _, _ = oracle.scan_cosine(z["corpus"], q, n, thr, rank)
        bits = sims.view(np.uint32)
        for name, part in (("inside", bits[:k]), ("behind", bits[k:])):
            if not {0, 0x80000000} <= set(part.tolist()):
                return "q%d: not both zeros %s the top %d" % (qi, name, k)
        prow, _ = packed_key_order(rows, sims, z["tie_rank"][rows], k)
        if set(prow.tolist()) == set(rows[:k].tolist()):
            return "q%d: the order by score bits keeps the same row set" % qi
    return None
