"""Restatement of the reference's spherical k-means (src/topology/topology_alternate_engines.cpp:288-478 and
topology_build_utils.h:27-56) in numpy: vectorised over (row, centroid) pairs, LOOPING over the dimension, so every fp64 chain
keeps the CPU loop's order; the fp32 mean is one running sum per cluster over its members in ascending row order.

    kmeans(rows, k, max_iterations)       -> membership [n] uint32, centroids [k_eff][dim] float32, k_eff, iterations run
    nearest(rows, centroids, empty)       -> assign [n] uint32, distance [n] float64 (DBL_MAX where no centroid won)
    run_shell(embeddings, k, max_iter)    -> runKMeans' outer shell (:343-365, :468-477) over ragged rows: assignment [n] int64
    case_rows(name)                       -> the inputs of a golden case (tests/golden/kmeans.json), from its recipe
"""
import hashlib

import numpy as np

DBL_MAX = np.finfo(np.float64).max
FLT_MAX = np.finfo(np.float32).max


def same_f32(x, y):
    """Bit equality of two float32 arrays; a NaN equals a NaN (its sign and payload are the platform's, not the contract's)."""
    x = np.ascontiguousarray(x, np.float32); y = np.ascontiguousarray(y, np.float32)
    if x.shape != y.shape or not np.array_equal(np.isnan(x), np.isnan(y)):
        return False
    ok = ~np.isnan(x)
    return np.array_equal(x.view(np.uint32)[ok], y.view(np.uint32)[ok])


def same_f64(x, y):
    x = np.ascontiguousarray(x, np.float64); y = np.ascontiguousarray(y, np.float64)
    if x.shape != y.shape or not np.array_equal(np.isnan(x), np.isnan(y)):
        return False
    ok = ~np.isnan(x)
    return np.array_equal(x.view(np.uint64)[ok], y.view(np.uint64)[ok])


def _dots(a, b):
    """dot[i][j] = the fp64 chain over the dimension of float(a[i][d]) * float(b[j][d]) (:292-299)."""
    a64 = np.asarray(a, np.float32).astype(np.float64); b64 = np.asarray(b, np.float32).astype(np.float64)
    dot = np.zeros((a64.shape[0], b64.shape[0]), np.float64)
    with np.errstate(all="ignore"):
        for d in range(a64.shape[1]):
            dot += a64[:, d:d + 1] * b64[:, d][None, :]
    return dot


def sumsq(a):
    a64 = np.asarray(a, np.float32).astype(np.float64)
    s = np.zeros(a64.shape[0], np.float64)
    with np.errstate(all="ignore"):
        for d in range(a64.shape[1]):
            s += a64[:, d] * a64[:, d]
    return s


def distances(a, b, na=None, nb=None):
    """cosineDistance (:288-305) of every row of a to every row of b."""
    na = sumsq(a) if na is None else na
    nb = sumsq(b) if nb is None else nb
    dot = _dots(a, b)
    with np.errstate(all="ignore"):
        cos = dot / (np.sqrt(na)[:, None] * np.sqrt(nb)[None, :])
        cl = np.where(cos < -1.0, -1.0, np.where(1.0 < cos, 1.0, cos))      # std::clamp: a NaN passes through
        d = 1.0 - cl
    two = (na <= 0.0)[:, None] | (nb <= 0.0)[None, :]
    return np.where(two, 2.0, d)


def pair_distances(a, b, na=None):
    """cosineDistance of row i of a to row i of b."""
    a64 = np.asarray(a, np.float32).astype(np.float64); b64 = np.asarray(b, np.float32).astype(np.float64)
    na = sumsq(a) if na is None else na
    nb = sumsq(b)
    dot = np.zeros(a64.shape[0], np.float64)
    with np.errstate(all="ignore"):
        for d in range(a64.shape[1]):
            dot += a64[:, d] * b64[:, d]
        cos = dot / (np.sqrt(na) * np.sqrt(nb))
        dist = 1.0 - np.where(cos < -1.0, -1.0, np.where(1.0 < cos, 1.0, cos))
    return np.where((na <= 0.0) | (nb <= 0.0), 2.0, dist)


def normalized(v):
    """:307-319"""
    v = np.asarray(v, np.float32).copy()
    norm = sumsq(v[None, :])[0]
    if norm > 0.0:
        with np.errstate(all="ignore"):
            inv = np.float32(1.0 / np.sqrt(norm))
            v = (v * inv).astype(np.float32)
    return v


def nearest(rows, centroids, empty=None, na=None):
    """nearestCentroid (:321-336) per row: strict <, so the lowest index among the minima; NaN never wins."""
    rows = np.asarray(rows, np.float32)
    n = rows.shape[0]
    best = np.zeros(n, np.uint32); best_d = np.full(n, DBL_MAX)
    centroids = np.asarray(centroids, np.float32).reshape(-1, rows.shape[1])
    if centroids.shape[0] == 0:
        return best, best_d
    d = distances(rows, centroids, na=na)
    for c in range(centroids.shape[0]):
        if empty is not None and empty[c]:
            continue
        with np.errstate(invalid="ignore"):
            win = d[:, c] < best_d
        best[win] = c; best_d[win] = d[win, c]
    return best, best_d


def _mean_centroids(rows, membership, k, centroids):
    """centroidOf (:403-410) of every cluster with members: fp32 running sums in ascending row order, / float(count)."""
    sums = np.zeros((k, rows.shape[1]), np.float32)
    counts = np.zeros(k, np.int64)
    with np.errstate(all="ignore"):
        for u in range(rows.shape[0]):
            c = membership[u]
            sums[c] += rows[u]
            counts[c] += 1
        for c in range(k):
            if counts[c]:
                centroids[c] = normalized((sums[c] / np.float32(counts[c])).astype(np.float32))
    return counts


def _centroid_of(rows, members):
    s = np.zeros(rows.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for u in members:
            s += rows[u]
        return normalized((s / np.float32(len(members))).astype(np.float32))


def effective_k(n, k):
    if k == 0:
        k = int(np.floor(np.sqrt(float(n)) + 0.5))        # std::round of a non-negative value
    return min(max(k, 2), n)


REPAIRS = [0]     # rows moved by the empty-cluster repair since the module was loaded (the harnesses' coverage counter)


def kmeans(rows, k=0, max_iterations=0):
    rows = np.ascontiguousarray(rows, np.float32)
    n, dim = rows.shape
    assert n >= 2 and dim >= 1
    k = effective_k(n, k)
    na = sumsq(rows)
    # ---- farthest-first initialisation (:373-401)
    centroids = np.zeros((k, dim), np.float32)
    centroids[0] = normalized(rows[0])
    selected = np.zeros(n, bool); selected[0] = True
    min_dist = np.full(n, DBL_MAX)
    have = 1
    while have < k:
        d = distances(rows, centroids[have - 1:have], na=na)[:, 0]
        with np.errstate(invalid="ignore"):
            upd = ~selected & (d < min_dist)
        min_dist[upd] = d[upd]
        cand = np.where(~selected)[0]
        if cand.size == 0:
            break
        far = cand[np.argmax(min_dist[cand])]                 # argmax: the first of the largest (min_dist is never NaN)
        selected[far] = True
        centroids[have] = normalized(rows[far]); have += 1
    k = have
    centroids = centroids[:k]
    # ---- Lloyd iterations (:412-466)
    membership = np.zeros(n, np.uint32)
    iterations = 10 if max_iterations == 0 else max_iterations
    ran = 0
    for _ in range(iterations):
        ran += 1
        new, _d = nearest(rows, centroids, na=na)
        changed = bool((new != membership).any())
        membership = new
        counts = _mean_centroids(rows, membership, k, centroids)
        for c in range(k):
            if counts[c]:
                continue
            own = pair_distances(rows, centroids[membership], na)     # every row's distance to its own, updated centroid
            eligible = np.where(counts[membership] > 1)[0]
            worst, donor = n, k
            if eligible.size:
                cand = np.where(np.isnan(own[eligible]), -np.inf, own[eligible])
                best = int(np.argmax(cand))                           # the first of the strictly largest
                if cand[best] > -1.0:
                    worst = int(eligible[best]); donor = int(membership[worst])
            if worst == n:
                continue
            membership[worst] = c; counts[donor] -= 1; counts[c] = 1
            REPAIRS[0] += 1
            centroids[c] = normalized(rows[worst])
            centroids[donor] = _centroid_of(rows, np.where(membership == donor)[0])
            changed = True
        if not changed:
            break
    return membership, centroids, k, ran


def usable_rows(embeddings):
    """:349-361: the rows that are not empty and have the first non-empty row's dimension."""
    dim = 0
    usable = []
    for i, e in enumerate(embeddings):
        if len(e):
            if dim == 0:
                dim = len(e)
            if len(e) == dim:
                usable.append(i)
    return usable, dim


def run_shell(embeddings, k=0, max_iterations=0, core=kmeans):
    """runKMeans (:341-478) over ragged embeddings; `core` clusters the usable rows."""
    n = len(embeddings)
    assignment = np.full(n, -1, np.int64)
    if n == 0:
        return assignment
    usable, dim = usable_rows(embeddings)
    if len(usable) < 2 or dim == 0:
        return np.arange(n, dtype=np.int64)
    rows = np.array([np.asarray(embeddings[i], np.float32) for i in usable], np.float32)
    membership, _, ke, _ = core(rows, k, max_iterations)
    assignment[usable] = membership.astype(np.int64)
    nxt = ke
    for i in range(n):
        if assignment[i] < 0:
            assignment[i] = nxt; nxt += 1
    return assignment


def partition(assignment):
    """The partition an assignment induces: sorted list of sorted row lists."""
    groups = {}
    for i, a in enumerate(np.asarray(assignment).tolist()):
        groups.setdefault(a, []).append(i)
    return sorted(sorted(g) for g in groups.values())


# ---- golden cases: inputs from recipes (raw bits are pinned by a SHA-256 in the golden file) ------------------------------------
def uniform_rows(seed, n, dim):
    """Deterministic floats in [-1, 1) with 24 significant bits (splitmix64 of seed and position): exact in fp32."""
    idx = np.arange(n * dim, dtype=np.uint64) + (np.uint64(seed) << np.uint64(40))
    with np.errstate(over="ignore"):
        z = idx + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32).reshape(n, dim)


def clustered_rows(seed, n, dim, groups, spread=0.25):
    """Rows around `groups` seeded directions, so the clustering has structure."""
    centres = uniform_rows(seed, groups, dim)
    noise = uniform_rows(seed + 1, n, dim)
    pick = (uniform_rows(seed + 2, n, 1)[:, 0].astype(np.float64) * 0.5 + 0.5) * groups
    return (centres[np.minimum(pick.astype(np.int64), groups - 1)] + np.float32(spread) * noise).astype(np.float32)


# name -> (k, max_iterations); the inputs are case_rows(name)
CASES = {
    "random_2000x64": (0, 0), "explicit_k": (7, 0), "one_iteration": (0, 1), "duplicates": (20, 0), "all_duplicates_of_three": (6, 0),
    "zero_rows": (0, 0), "flt_max_quarter": (4, 0), "denormal_rows": (3, 0), "dim_1": (0, 0), "dim_3": (5, 0), "dim_50": (0, 0),
    "n_2": (0, 0), "k_above_n": (50, 0), "ragged_shell": (3, 0), "one_usable_row": (0, 0),
}


def case_rows(name):
    """The embeddings of a golden case: a list of float32 arrays (ragged only for the adapter-shell cases)."""
    if name == "random_2000x64":
        rows = clustered_rows(11, 2000, 64, 30)
    elif name == "explicit_k":
        rows = clustered_rows(12, 300, 32, 9)
    elif name == "one_iteration":
        rows = clustered_rows(13, 300, 32, 9)
    elif name == "duplicates":                     # 14 distinct rows among 120, k = 20: duplicate centroids, ties, the repair path
        base = uniform_rows(14, 14, 16)
        rows = base[(np.arange(120) * 5) % 14]
    elif name == "all_duplicates_of_three":
        base = uniform_rows(15, 3, 8)
        rows = base[np.arange(40) % 3]
    elif name == "zero_rows":
        rows = clustered_rows(16, 60, 8, 4)
        rows[[0, 7, 8, 30, 59]] = 0.0
    elif name == "flt_max_quarter":                # the fp32 mean of a few such rows overflows
        sign = np.where(uniform_rows(17, 24, 6) < 0, np.float32(-1), np.float32(1))
        rows = (sign * np.float32(FLT_MAX / 4)).astype(np.float32)
        rows[3] = uniform_rows(18, 1, 6)[0]
    elif name == "denormal_rows":                  # 1 / sqrt(norm) overflows fp32: infinite and NaN centroids
        rows = uniform_rows(19, 30, 5)
        rows[::3] = (rows[::3] * np.float32(1e-42)).astype(np.float32)
    elif name == "dim_1":
        rows = uniform_rows(20, 40, 1)
    elif name == "dim_3":
        rows = clustered_rows(21, 50, 3, 4)
    elif name == "dim_50":
        rows = clustered_rows(22, 90, 50, 6)
    elif name == "n_2":
        rows = uniform_rows(23, 2, 4)
    elif name == "k_above_n":
        rows = uniform_rows(24, 10, 4)
    elif name == "ragged_shell":                   # an empty row first, rows of another dimension, an empty row last
        r = clustered_rows(25, 14, 6, 3)
        out = [r[i] for i in range(14)]
        out[0] = np.zeros(0, np.float32); out[4] = np.ones(5, np.float32); out[9] = np.ones(7, np.float32); out[13] = np.zeros(0, np.float32)
        return out
    elif name == "one_usable_row":
        return [np.zeros(0, np.float32), np.ones(4, np.float32), np.ones(3, np.float32)]
    else:
        raise KeyError(name)
    return [np.ascontiguousarray(r, np.float32) for r in rows]


def rows_digest(embeddings):
    h = hashlib.sha256()
    for e in embeddings:
        h.update(np.uint32(len(e)).tobytes()); h.update(np.asarray(e, np.float32).tobytes())
    return h.hexdigest()
