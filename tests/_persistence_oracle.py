"""A restatement of computePersistenceH0 (the contract in include/yams_mi355x_accel.h) in both chain forms, returning the
intermediates the device entry exposes: the distance matrix, the percentile and its index, the merge weights, the value.

Two implementations that must agree bit for bit:
  persistence_py    numpy for the separate form (a multiply ufunc, then an add ufunc: two roundings), the exact fma of
                    tests/_artifacts_oracle.py for the fused one; the reference's real Kruskal over a stable sort
  persistence_cpp   tests/cpp/persistence_oracle.cpp through ctypes, for the cases the pure-Python fma is too slow for
prim_weights is a third, independent tree construction: the sorted weights of any minimum spanning tree equal Kruskal's."""
import ctypes as C
import hashlib

import numpy as np

from _artifacts_oracle import fma

SEPARATE, FUSED = 0, 1
FORMS = {"separate": SEPARATE, "fused": FUSED}
MAX_POINTS = 16384


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def hex64(v):
    return "%016x" % int(np.float64(v).view(np.uint64))


def from_hex64(s):
    return float(np.uint64(int(s, 16)).view(np.float64))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def percentile_index(edges):
    """size_t(std::clamp(0.95 * double(E - 1), 0.0, double(E - 1)))"""
    if edges == 0:
        return 0
    hi = float(edges - 1)
    return int(min(max(0.95 * hi, 0.0), hi))


def distances_py(x, form):
    x = np.ascontiguousarray(x, np.float32).astype(np.float64)
    m, dim = x.shape
    acc = np.zeros((m, m))
    if form == SEPARATE:
        for k in range(dim):
            d = x[:, k][:, None] - x[:, k][None, :]
            p = d * d
            acc = acc + p
    else:
        for i in range(m):
            for j in range(i + 1, m):
                a = 0.0
                for k in range(dim):
                    d = float(x[i, k]) - float(x[j, k])
                    a = fma(d, d, a)
                acc[i, j] = acc[j, i] = a
    return np.sqrt(acc)


def kruskal(dist):
    """The reference's loop: edges in (i, j) generation order, stably sorted by distance, union by rank with path halving.
    Returns every merge's weight, in merge order (m - 1 of them: the loop is not stopped at m - 2)."""
    m = dist.shape[0]
    iu, ju = np.triu_indices(m, 1)
    w = dist[iu, ju]
    order = np.argsort(w, kind="stable")
    parent, rank = list(range(m)), [0] * m

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    out = []
    for e in order:
        if len(out) + 1 >= m:
            break
        ra, rb = find(int(iu[e])), find(int(ju[e]))
        if ra == rb:
            continue
        if rank[ra] < rank[rb]:
            ra, rb = rb, ra
        parent[rb] = ra
        if rank[ra] == rank[rb]:
            rank[ra] += 1
        out.append(float(w[e]))
    return np.array(out, np.float64)


def prim_weights(dist):
    """Prim from vertex 0, ties to the lower vertex; the tree's weights sorted ascending."""
    m = dist.shape[0]
    if m < 2:
        return np.zeros(0)
    key = dist[0].copy()
    inside = np.zeros(m, bool)
    inside[0] = True
    out = []
    for _ in range(m - 1):
        k = np.where(inside, np.inf, key)
        v = int(np.argmin(k))
        out.append(float(k[v]))
        inside[v] = True
        key = np.minimum(key, dist[v])
    return np.sort(np.array(out, np.float64))


def _finish(m, dist, weights):
    edges = m * (m - 1) // 2
    idx = percentile_index(edges)
    norm = 0.0
    if edges:
        iu, ju = np.triu_indices(m, 1)
        norm = float(np.sort(dist[iu, ju])[idx])
    value, merges = 0.0, 0
    if m >= 2 and norm > 0.0:
        for w in weights[:m - 2]:
            value += float(w) / norm
            merges += 1
    return {"distances": dist, "norm": norm, "norm_index": idx, "n_edges": edges, "n_points": m, "weights": weights,
            "value": value, "n_merges": merges}


def persistence_py(x, form):
    x = np.ascontiguousarray(x, np.float32)
    m = x.shape[0]
    if m < 2:
        return _finish(m, np.zeros((m, m)), np.zeros(0))
    dist = distances_py(x, form)
    return _finish(m, dist, kruskal(dist))


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        import _persistence_build
        _LIB = C.CDLL(_persistence_build.build_oracle())
        _LIB.persistence_oracle.restype = C.c_uint64
        _LIB.persistence_oracle.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    return _LIB


def persistence_cpp(x, form, want_distances=True):
    x = np.ascontiguousarray(x, np.float32)
    m, dim = x.shape
    dist = np.zeros((m, m)) if want_distances else None
    w = np.zeros(max(m - 1, 0))
    norm, idx, value = C.c_double(), C.c_uint64(), C.c_double()
    merges = _lib().persistence_oracle(x.ctypes.data, m, dim, int(form), dist.ctypes.data if want_distances else None,
                                       w.ctypes.data, C.byref(norm), C.byref(idx), C.byref(value))
    return {"distances": dist, "norm": norm.value, "norm_index": idx.value, "n_edges": m * (m - 1) // 2, "n_points": m,
            "weights": w, "value": value.value, "n_merges": int(merges)}


def same(got, want, what=("norm", "value")):
    """Bit for bit on every field both carry."""
    for k in ("norm_index", "n_edges", "n_points", "n_merges"):
        if int(got[k]) != int(want[k]):
            return False
    for k in what:
        if hex64(got[k]) != hex64(want[k]):
            return False
    for k in ("distances", "weights"):
        if got.get(k) is not None and want.get(k) is not None:
            if got[k].shape != want[k].shape or not (bits64(got[k]) == bits64(want[k])).all():
                return False
    return True


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def mixed_points(seed, m, dim):
    """Floats with mixed exponents: differences carry many significant bits, so d * d is inexact."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m, dim)) * np.exp2(rng.integers(-6, 7, (m, dim)))).astype(np.float32)


def lattice_points(seed, m, dim, side=4):
    """Integer lattice: many exactly equal distances, duplicate points among them."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, side, (m, dim)).astype(np.float32)


def duplicated_points(seed, copies, others, dim):
    """`copies` copies of one point and `others` further points: with copies >> others almost every distance is 0."""
    rng = np.random.default_rng(seed)
    p = mixed_points(seed, 1 + others, dim)
    x = np.concatenate([np.repeat(p[:1], copies, 0), p[1:]])
    return x[rng.permutation(len(x))]


def cluster_points(seed, clusters, per, dim, spread=64.0):
    """Well-separated clusters: long edges in the tree, the heaviest left out."""
    rng = np.random.default_rng(seed)
    centres = (rng.standard_normal((clusters, dim)) * spread).astype(np.float32)
    x = np.repeat(centres, per, 0) + mixed_points(seed + 1, clusters * per, dim) * np.float32(1.0 / 64)
    return x.astype(np.float32)[rng.permutation(clusters * per)]


def plateau_is_strictly_inside(x):
    r = persistence_py(x, SEPARATE)
    iu, ju = np.triu_indices(len(x), 1)
    s = np.sort(r["distances"][iu, ju])
    i = r["norm_index"]
    return 0 < i < len(s) - 1 and s[i - 1] == s[i] == s[i + 1] and s[0] != s[-1]


def _golden_cases():
    cases = {}
    for k in range(40):      # three- to six-point clouds, dims 1 .. 12
        m, dim = 3 + k % 4, 1 + (k * 5) % 12
        cases["mixed_%02d_m%d_d%d" % (k, m, dim)] = (lambda k=k, m=m, dim=dim: mixed_points(1000 + k, m, dim))
    cases["lattice_2d_m24"] = lambda: lattice_points(1, 24, 2)
    cases["lattice_3d_m40"] = lambda: lattice_points(2, 40, 3)
    cases["lattice_plateau_m30"] = lambda: lattice_points(3, 30, 2, side=3)      # the index falls strictly inside a plateau
    cases["duplicates_some_m20"] = lambda: duplicated_points(4, 8, 12, 5)
    cases["duplicates_norm_zero_m41"] = lambda: duplicated_points(5, 40, 1, 7)    # > 95 % of the distances are 0: norm = 0
    cases["all_the_same_point_m6"] = lambda: np.repeat(mixed_points(6, 1, 4), 6, 0)
    cases["clusters_4x6_d9"] = lambda: cluster_points(7, 4, 6, 9)
    cases["clusters_3x11_d33"] = lambda: cluster_points(8, 3, 11, 33)
    cases["two_points"] = lambda: mixed_points(9, 2, 5)
    cases["two_equal_points"] = lambda: np.repeat(mixed_points(10, 1, 3), 2, 0)
    return cases


GOLDEN_CASES = _golden_cases()


def write_case(path, x):
    x = np.ascontiguousarray(x, np.float32)
    with open(path, "wb") as f:
        f.write(np.array(x.shape, np.uint32).tobytes())
        f.write(x.tobytes())


def golden_record(r):
    """What the golden file keeps of a restatement's result."""
    return {"value": hex64(r["value"]), "norm": hex64(r["norm"]), "norm_index": int(r["norm_index"]), "n_merges": int(r["n_merges"]),
            "distances_sha256": digest(r["distances"]), "weights_sha256": digest(r["weights"])}
