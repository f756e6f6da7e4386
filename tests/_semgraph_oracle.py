"""The semantic-neighbour graph's pair loop restated in numpy (EmbeddingService::updateSemanticNeighborGraphUnlocked,
src/daemon/components/EmbeddingService.cpp of the reference; the contract is restated in include/yams_mi355x_accel.h above
yams_graph_semantic_neighbors_device):

  inverse norm  norm = sequential fp64 chain of x * x; inv = norm <= 0 ? 0.0f : float(1.0 / sqrt(norm))         (:405-415)
  similarity    dot = sequential fp64 chain of double(a[i]) * double(b[i]);
                sim = float((dot * double(inv_source)) * double(inv_neighbour))                                  (:417-431)
  corpus        rows with inv <= 0 are neither candidates nor sources                                            (:876-878)
  admission     adaptive: sim <= 0 dropped; explicit: sim < threshold dropped                                    (:991-997)
  order         sim descending by the float compare (one zero), then hash rank ascending; the best K, sorted     (:949-1017)
  counts        pairs scored (similarityPairCount), pairs admitted (candidateNeighborCount)

The chains are walked element by element over whole matrices: a product of two floats is exact in fp64, so numpy's multiply
followed by add rounds as the C loop's `+=` does.  Also here: the named cases tests/golden/semantic_neighbors.json records
(make_semgraph_golden.py ran the reference's own loop over them) and the generators of the GPU tests and the stress harness."""
import hashlib

import numpy as np

EMPTY_ROW = 0xffffffff
FLT_MAX = np.float32(3.4028234663852886e38)


class InvalidArg(Exception):
    """What the entry refuses with YAMS_ERR_INVALID_ARG."""


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def inverse_norms(x):
    """(inv [n] float32); raises InvalidArg for a non-finite element or an infinite inverse."""
    x = np.ascontiguousarray(x, np.float32)
    xd = x.astype(np.float64)
    s = np.zeros(x.shape[0], np.float64)
    with np.errstate(all="ignore"):
        for i in range(x.shape[1]):
            s = s + xd[:, i] * xd[:, i]
        if not np.isfinite(s).all():
            raise InvalidArg("non-finite element")
        inv = np.where(s <= 0.0, np.float32(0.0), (1.0 / np.sqrt(np.where(s <= 0.0, 1.0, s))).astype(np.float32)).astype(np.float32)
    if np.isinf(inv).any():
        raise InvalidArg("infinite inverse norm")
    return inv


def rank_of_hashes(hashes):
    """tie_rank[row] = the position of the row's hash in std::string order (ASCII hashes: Python's str order)."""
    order = sorted(range(len(hashes)), key=lambda i: hashes[i])
    rank = np.zeros(len(hashes), np.uint32)
    rank[order] = np.arange(len(hashes), dtype=np.uint32)
    return rank


def neighbors(x, k, tie_rank=None, source_rows=None, threshold=None, block=256):
    """Returns dict(rows [S][k] uint32, sims [S][k] float32, counts [S] uint32, inv [n] float32, pairs_scored, pairs_admitted).
    threshold=None: adaptive mode."""
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    inv = inverse_norms(x)
    src = np.arange(n, dtype=np.int64) if source_rows is None else np.asarray(source_rows, np.int64)
    if (src < 0).any() or (src >= n).any():
        raise InvalidArg("source index out of range")
    rank = np.arange(n, dtype=np.int64) if tie_rank is None else np.asarray(tie_rank, np.int64)
    S = len(src)
    out_rows = np.full((S, k), EMPTY_ROW, np.uint32)
    out_sims = np.full((S, k), -np.inf, np.float32)
    counts = np.zeros(S, np.uint32)
    scored = admitted = 0
    if k == 0 or n < 2:
        return dict(rows=out_rows, sims=out_sims, counts=counts, inv=inv, pairs_scored=0, pairs_admitted=0)
    xd = x.astype(np.float64)
    invd = inv.astype(np.float64)
    valid = inv > 0
    for b0 in range(0, S, block):
        sb = src[b0:b0 + block]
        a = xd[sb]
        dot = np.zeros((len(sb), n), np.float64)
        with np.errstate(all="ignore"):
            for i in range(dim):
                dot += a[:, i, None] * xd[None, :, i]
            sim = ((dot * invd[sb][:, None]) * invd[None, :]).astype(np.float32)
        pair = valid[sb][:, None] & valid[None, :] & (sb[:, None] != np.arange(n)[None, :])
        adm = pair & ((sim >= np.float32(threshold)) if threshold is not None else (sim > 0))
        scored += int(pair.sum())
        admitted += int(adm.sum())
        for j in range(len(sb)):
            c = np.nonzero(adm[j])[0]
            if not len(c):
                continue
            s = sim[j, c]
            order = np.lexsort((rank[c], -(s + np.float32(0.0))))[:k]      # (+ 0.0f: the two zeros are one score)
            m = len(order)
            out_rows[b0 + j, :m] = c[order]
            out_sims[b0 + j, :m] = s[order]
            counts[b0 + j] = m
    return dict(rows=out_rows, sims=out_sims, counts=counts, inv=inv, pairs_scored=scored, pairs_admitted=admitted)


def effective_thresholds(res, threshold):
    """Per source: the explicit threshold, or the last kept similarity (:1018-1019); None for a source without neighbours."""
    return [None if c == 0 else (np.float32(threshold) if threshold is not None else res["sims"][i, c - 1]) for i, c in enumerate(res["counts"])]


# ---- the golden cases ------------------------------------------------------------------------------------------------------
def _hashes(n, tag, reverse=False):
    h = [hashlib.sha256(f"{tag}:{i}".encode()).hexdigest() for i in range(n)]
    if reverse:      # hash order opposite to row order
        h = sorted(h, reverse=True)
    return h


def _rng_rows(seed, n, dim, scale=1.0):
    r = np.random.default_rng(seed)
    return (r.standard_normal((n, dim)) * scale).astype(np.float32)


def golden_cases():
    """name -> dict(rows [n][dim] float32, hashes [n], k, threshold (None = adaptive), sources (None = every row))."""
    c = {}
    c["basic"] = dict(rows=_rng_rows(1, 12, 6), k=3)
    d = _rng_rows(2, 5, 4)
    c["duplicates"] = dict(rows=np.concatenate([d, d, d[:2]]), k=4)                       # identical bits, different hashes
    z = _rng_rows(3, 9, 5); z[2] = 0; z[6] = 0
    c["zero_rows"] = dict(rows=z, k=3)
    q = FLT_MAX / np.float32(4)
    c["flt_max_quarter"] = dict(rows=np.array([[q, q, -q, q], [q, -q, -q, q], [-q, q, q, -q], [q, q, q, q], [1, 2, -3, 4], [q, 1, 1, 1]], np.float32), k=4)
    c["denormal_cosine"] = dict(rows=np.array([[1, 0], [np.float32(1e-40), 1], [0.5, 0.5], [np.float32(1e-40), np.float32(3e-39)], [0, 2]], np.float32), k=4)
    # cosines of row 0 against rows 1..6: +0 (underflow from above), -0 (from below), exact +0, and real values
    plateau = np.array([[1, 0], [np.float32(1e-40), 1e10], [np.float32(-1e-40), 1e10], [0, 1], [np.float32(-1e-40), 3e10], [np.float32(1e-40), 2e10], [1, 1], [-1, 1]], np.float32)
    c["zero_plateau_explicit0"] = dict(rows=plateau, k=6, threshold=0.0, reverse=True)
    c["zero_plateau_adaptive"] = dict(rows=plateau, k=6)
    c["fewer_than_k"] = dict(rows=_rng_rows(4, 5, 7), k=8)
    c["k1"] = dict(rows=_rng_rows(5, 10, 3), k=1)
    e = _rng_rows(6, 4, 3)
    c["hash_reverse"] = dict(rows=np.concatenate([e, e, e]), k=5, reverse=True)           # ties decided against row order
    cl = _rng_rows(7, 3, 8)
    c["explicit_half"] = dict(rows=(np.repeat(cl, 5, axis=0) + _rng_rows(8, 15, 8, 0.4)).astype(np.float32), k=6, threshold=0.5)
    c["explicit_one"] = dict(rows=np.concatenate([e, e * np.float32(2), _rng_rows(9, 3, 3)]), k=3, threshold=1.0)
    c["negatives_adaptive"] = dict(rows=np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 1, 0], [-1, -1, 0], [0, 0, 1]], np.float32), k=8)
    c["source_subset"] = dict(rows=z, k=4, sources=[7, 2, 0, 4])                          # unordered, one of them a zero row
    for name, v in c.items():
        v["rows"] = np.ascontiguousarray(v["rows"], np.float32)
        v.setdefault("threshold", None)
        v.setdefault("sources", None)
        v["hashes"] = _hashes(len(v["rows"]), name, v.pop("reverse", False))
    return c


def run_case(v):
    return neighbors(v["rows"], v["k"], rank_of_hashes(v["hashes"]), v["sources"], v["threshold"])


# ---- generators of the GPU tests and the stress harness ----------------------------------------------------------------------
def uniform_rows(seed, n, dim):
    return _rng_rows(seed, n, dim)


def clustered_rows(seed, n, dim, clusters=7, spread=0.05):
    r = np.random.default_rng(seed)
    cent = r.standard_normal((clusters, dim))
    return (cent[r.integers(0, clusters, n)] + spread * r.standard_normal((n, dim))).astype(np.float32)


def duplicate_rows(seed, n, dim, distinct=5):
    """n rows drawn from `distinct` vectors: every score is a plateau and the tie rank decides."""
    r = np.random.default_rng(seed)
    base = r.standard_normal((distinct, dim)).astype(np.float32)
    return base[r.integers(0, distinct, n)]


def shuffled_rank(seed, n):
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)
