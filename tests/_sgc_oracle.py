"""numpy restatement of SGC smoothing over a given neighbour list (include/yams_mi355x_accel.h,
yams_graph_sgc_smooth_device):

    deg[i] = 1.0 + the fp64 chain of double(w) over row i's edges in list order;  inv[i] = 1.0 / sqrt(deg[i])
    one hop: acc = float((inv[i] * inv[i]) * double(x[i][d])); for each edge (to, w) of row i IN LIST ORDER:
             scale = (double(w) * inv[i]) * inv[to]; scale == 0.0: the edge is skipped; otherwise
             acc = acc +f32 float(scale * double(x[to][d]))
    hop h + 1 reads the output of hop h

The walk is vectorised over rows and dimensions, never over a row's edges: step k handles the k-th edge of every row that has
one, so every element sees its row's edges one at a time and in list order.  numpy's float64 -> float32 cast rounds to nearest
even and its float32 add keeps denormals.

Also here: the recipes of the golden cases (documents with neighbour lists, as applySGCSmoothing takes them;
tests/golden/make_sgc_golden.py runs the reference on them) and the seeded list-level cases of the GPU tests and the stress
harness."""
import hashlib

import numpy as np

MAX_DIM, HUB_DEGREE = 4096, 512
FLT_MAX = np.float32(3.4028234663852886e38)


class InvalidArg(Exception):
    pass


class Unsupported(Exception):
    pass


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f32(b):
    return np.asarray(b, np.uint32).view(np.float32)


def same_bits(got, want):
    """Bit for bit, but a NaN matches any NaN (the only tolerance anywhere)."""
    got = np.ascontiguousarray(got, np.float32); want = np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def check_lists(n, off, cols, w):
    off = np.asarray(off, np.uint64)
    if len(off) != n + 1 or (n and off[0] != 0) or (np.diff(off.astype(np.int64)) < 0).any():
        raise InvalidArg("row_offsets")
    nnz = int(off[n]) if n else 0
    if nnz >= 1 << 32:
        raise Unsupported("nnz")
    cols = np.asarray(cols, np.uint32)[:nnz]; w = np.asarray(w, np.float32)[:nnz]
    if (cols >= n).any():
        raise InvalidArg("column")
    if not (np.isfinite(w) & (w >= 0)).all():
        raise InvalidArg("weight")
    return off.astype(np.int64), cols.astype(np.int64), w


def inverse_sqrt_degrees(off, w):
    n = len(off) - 1
    cnt = np.diff(off)
    deg = np.ones(n, np.float64)
    for k in range(int(cnt.max()) if n else 0):
        sel = np.nonzero(cnt > k)[0]
        deg[sel] = deg[sel] + w[off[sel] + k].astype(np.float64)
    return 1.0 / np.sqrt(deg)


def smooth(x, off, cols, w, hops, skip_zero_scale=True, with_diag=False):
    """out [n][dim] float32.  skip_zero_scale=False is the WRONG loop that adds an edge of scale 0.0 anyway (what the tests
    compare against to show a case reaches the skip)."""
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    if n >= 1 << 31 or dim > MAX_DIM:
        raise Unsupported("limits")
    if n == 0:
        return (x.copy(), dict(nnz=0, edges_skipped_zero_scale=0, max_degree=0, hops=0, hub_rows=0)) if with_diag else x.copy()
    if dim == 0:
        raise InvalidArg("dim")
    if hops == 0:
        return (x.copy(), dict(nnz=0, edges_skipped_zero_scale=0, max_degree=0, hops=0, hub_rows=0)) if with_diag else x.copy()
    off, cols, w = check_lists(n, off, cols, w)
    if not np.isfinite(x).all():
        raise InvalidArg("rows")
    cnt = np.diff(off)
    inv = inverse_sqrt_degrees(off, w)
    row_of_edge = np.repeat(np.arange(n), cnt)
    scale = (w.astype(np.float64) * inv[row_of_edge]) * inv[cols]
    self_scale = inv * inv
    max_deg = int(cnt.max())
    steps = []
    for k in range(max_deg):
        sel = np.nonzero(cnt > k)[0]
        e = off[sel] + k
        if skip_zero_scale:
            live = scale[e] != 0.0
            sel, e = sel[live], e[live]
        steps.append((sel, cols[e], scale[e][:, None]))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for _ in range(hops):
            acc = (self_scale[:, None] * x.astype(np.float64)).astype(np.float32)
            for sel, to, s in steps:
                if len(sel):
                    acc[sel] = acc[sel] + (s * x[to].astype(np.float64)).astype(np.float32)
            x = acc
    if with_diag:
        return x, dict(nnz=int(off[n]), edges_skipped_zero_scale=int((scale == 0.0).sum()), max_degree=max_deg, hops=hops,
                       hub_rows=int((cnt >= HUB_DEGREE).sum()))
    return x


def sort_rows(off, cols, w):
    """The same lists with every row's edges sorted by column (a stable sort): another sum order."""
    off = np.asarray(off, np.int64); cols = np.asarray(cols, np.uint32).copy(); w = np.asarray(w, np.float32).copy()
    for i in range(len(off) - 1):
        a, b = off[i], off[i + 1]
        o = np.argsort(cols[a:b], kind="stable")
        cols[a:b] = cols[a:b][o]; w[a:b] = w[a:b][o]
    return cols, w


# ---- seeded list-level cases -----------------------------------------------------------------------------------------------------
def random_lists(rng, n, max_degree=8, zero_weight=0.1, empty_rows=0.1, hub=None):
    """(row_offsets uint64 [n + 1], cols uint32, weights float32): every row draws up to max_degree edges to any row (itself
    and repeats included); a share of the weights is 0; a share of the rows is empty; hub = (row, degree) plants one long row."""
    cnt = rng.integers(0, max_degree + 1, n)
    cnt[rng.random(n) < empty_rows] = 0
    if hub is not None:
        cnt[hub[0]] = hub[1]
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(cnt)
    nnz = int(off[n])
    cols = rng.integers(0, n, nnz).astype(np.uint32)
    w = rng.random(nnz).astype(np.float32)
    w[rng.random(nnz) < zero_weight] = 0.0
    return off, cols, w


def random_rows(rng, n, dim, specials=True):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    if specials and x.size >= 8:
        flat = x.reshape(-1)
        idx = rng.choice(flat.size, min(flat.size // 2, 12), replace=False)
        vals = np.array([-0.0, 0.0, 1e-40, -1e-40, 1.4e-45, float(FLT_MAX) / 4, -float(FLT_MAX) / 4, 1.1754944e-38], np.float32)
        flat[idx] = vals[np.arange(len(idx)) % len(vals)]
    return x


def seeded_case(seed, n, dim, max_degree=8, hub=None, specials=True):
    rng = np.random.default_rng(seed)
    off, cols, w = random_lists(rng, n, max_degree, hub=hub)
    return random_rows(rng, n, dim, specials), off, cols, w


# ---- the golden cases: documents as applySGCSmoothing takes them ------------------------------------------------------------------
def doc(h, emb, nbrs=()):
    """nbrs: (hash, score, reciprocal)."""
    return dict(hash=h, emb=np.asarray(emb, np.float32), nbrs=[(a, np.float32(s), bool(r)) for a, s, r in nbrs])


def two_clusters():
    e = [[1.0, 0.0, 0.0], [0.95, 0.05, 0.0], [0.9, 0.1, 0.0], [0.0, 1.0, 0.0], [0.05, 0.95, 0.0], [0.1, 0.9, 0.0]]
    names = "abcdef"
    docs = []
    for i, h in enumerate(names):
        grp = names[:3] if i < 3 else names[3:]
        docs.append(doc(h, e[i], [(o, 0.9, True) for o in grp if o != h]))
    return docs


def ragged():
    d = two_clusters()
    d[1]["emb"] = np.zeros(0, np.float32)
    d[2]["emb"] = np.array([0.9, 0.1], np.float32)
    d[3]["nbrs"].append(("missing", np.float32(0.95), True))
    d.append(doc("", [42.0]))
    return d


def seeded_docs(seed, n, dim, k=8, ragged_share=0.05):
    rng = np.random.default_rng(seed)
    docs = []
    for i in range(n):
        emb = rng.standard_normal(dim).astype(np.float32)
        r = rng.random()
        if r < ragged_share / 2:
            emb = emb[:0]
        elif r < ragged_share:
            emb = rng.standard_normal(dim + 1).astype(np.float32)
        others = rng.choice(n, k, replace=False)
        nb = [("h%05d" % j, np.float32(rng.random() * 1.2 - 0.1), bool(rng.random() < 0.8)) for j in others]
        docs.append(doc("h%05d" % i, emb, nb))
    if len(docs[0]["emb"]) != dim:
        docs[0]["emb"] = rng.standard_normal(dim).astype(np.float32)      # the first non-empty embedding sets dim
    return docs


def _mixed():
    # four documents in a ring plus chords; scores and reciprocal flags of every kind
    return [doc("p", [1.0, -2.0, 0.5, 3.0], [("q", 0.8, True), ("r", 0.3, False), ("s", 0.5, True)]),
            doc("q", [0.25, 4.0, -1.5, 0.0], [("p", 0.6, True), ("r", 0.7, True)]),
            doc("r", [-3.0, 0.125, 2.0, 1.0], [("q", 0.7, False), ("s", 0.49999997, True), ("p", 0.9, False)]),
            doc("s", [0.5, 0.5, -0.5, -4.0], [("p", 0.5, True), ("r", 0.2, True)])]


GOLDEN_CASES = {
    # name: (documents, minEdgeScore, reciprocalOnly, hops)
    "two_clusters_hops0": (two_clusters, 0.0, True, 0),
    "two_clusters_hops1": (two_clusters, 0.0, True, 1),
    "two_clusters_hops2": (two_clusters, 0.0, True, 2),
    "ragged_hops3": (ragged, 0.0, True, 3),
    "duplicate_hashes": (lambda: [doc("a", [1.0, 2.0], [("b", 0.9, True)]), doc("b", [3.0, -1.0], [("a", 0.8, True)]),
                                  doc("a", [-2.0, 0.5], [("b", 0.4, True)]), doc("c", [0.25, 8.0], [("a", 0.7, True)])], 0.0, True, 2),
    "reciprocal_only": (_mixed, 0.0, True, 2),
    "reciprocal_off": (_mixed, 0.0, False, 2),
    "min_edge_at_a_score": (_mixed, 0.5, False, 1),        # 0.5 stays, 0.49999997 goes
    "nan_score": (lambda: [doc("a", [1.0, -1.0, 2.0], [("b", np.nan, True), ("c", 0.5, True)]), doc("b", [-0.0, 3.0, 0.5]),
                           doc("c", [4.0, 0.25, -2.0])], 0.0, True, 2),
    "two_sided_scores": (lambda: [doc("a", [1.0, 2.0], [("b", 0.3, True)]), doc("b", [-1.0, 0.5], [("a", 0.75, True), ("c", 0.6, True)]),
                                  doc("c", [0.125, -3.0], [("b", 0.2, True)])], 0.0, True, 3),
    "zero_weight_beside_negative_zero": (lambda: [doc("a", [-0.0, 1.0, -0.0], [("b", 0.0, True)]), doc("b", [2.0, -0.0, 0.0]),
                                                  doc("c", [-0.0, -0.0, 5.0], [("a", -0.25, True)])], -1.0, True, 2),
    "seeded_300x37": (lambda: seeded_docs(11, 300, 37), 0.05, True, 2),
    "seeded_200x64_all_edges": (lambda: seeded_docs(12, 200, 64, k=6), -1.0, False, 3),
}
RAW_BITS_MAX = 512        # floats: cases up to this size carry their raw bits


def docs_digest(docs):
    h = hashlib.sha256()
    for d in docs:
        h.update(d["hash"].encode()); h.update(b"\0"); h.update(bits(d["emb"]).tobytes())
        for a, s, r in d["nbrs"]:
            h.update(a.encode()); h.update(b"\0"); h.update(bits([s]).tobytes()); h.update(b"\1" if r else b"\0")
    return h.hexdigest()


def embeddings_digest(embs):
    h = hashlib.sha256()
    for e in embs:
        h.update(bits(e).tobytes()); h.update(b"|")
    return h.hexdigest()


def feature_matrix(docs):
    """(x [n][dim] with +0.0f rows for embeddings of another size, the mask of rows that are written back), or (None, None)
    when no embedding is non-empty."""
    dim = next((len(d["emb"]) for d in docs if len(d["emb"])), 0)
    if dim == 0:
        return None, None
    x = np.zeros((len(docs), dim), np.float32)
    live = np.array([len(d["emb"]) == dim for d in docs])
    for i, d in enumerate(docs):
        if live[i]:
            x[i] = d["emb"]
    return x, live


def apply_to_docs(docs, off, cols, w, hops):
    """The embeddings after applySGCSmoothing, given the lists its symmetrisation produced."""
    embs = [d["emb"].copy() for d in docs]
    x, live = feature_matrix(docs)
    if hops == 0 or len(docs) < 2 or x is None:
        return embs
    y = smooth(x, off, cols, w, hops)
    return [y[i].copy() if live[i] else embs[i] for i in range(len(docs))]
