"""A numpy / pure-Python restatement of the contract include/yams_mi355x_accel.h gives for the cluster router's dense signal
(SparseGuidedClusterRouter::route, reference src/topology/topology_baseline.cpp:669-689, :771-981), and of the host-side lines
around it (seeds, blend, scoring modes, sort), so that whole route lists can be held against the reference's own.

Every float step is a numpy float32 operation (IEEE single, round to nearest, denormals kept); every chain is an fp64 sum in
element order.  Nothing here is the code under test."""
import hashlib
import math
import struct

import numpy as np

F32 = np.float32
CENTROID = 0xFFFF            # position of a centroid row in a table
MODES = ("current", "size_weighted", "seed_coverage")


def f32(bits):
    return np.frombuffer(struct.pack("<I", bits), F32)[0]


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def same_bits(a, b):
    """Bit equality of two float32 arrays, where a NaN matches any NaN."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---- the helpers (:669-689) ----------------------------------------------------------------------------------------------------
def chains(a, b):
    """dot[i][j] = the fp64 chain of a[i] and b[j] in element order (before the float cast).  a [m][dim], b [n][dim] float32."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float64)
    with np.errstate(all="ignore"):
        for i in range(a.shape[1]):
            acc += a[:, i].astype(np.float64)[:, None] * b[:, i].astype(np.float64)[None, :]
    return acc


def norms(x):
    """vectorNorm of every row: float(sqrt(chain of squares))."""
    x = np.ascontiguousarray(x, F32)
    acc = np.zeros(x.shape[0], np.float64)
    with np.errstate(all="ignore"):
        for i in range(x.shape[1]):
            v = x[:, i].astype(np.float64)
            acc += v * v
        return np.sqrt(acc).astype(F32)


def map_cosine(dot64, qn, vn):
    """dense of one vector: float(dot) / (qn * vn), (cos + 1) * 0.5, std::clamp's comparisons (a NaN passes through)."""
    with np.errstate(all="ignore"):
        d = np.asarray(dot64, np.float64).astype(F32)
        cos = d / (np.asarray(qn, F32) * np.asarray(vn, F32))
        v = (cos + F32(1.0)) * F32(0.5)
        return np.where(v < F32(0.0), F32(0.0), np.where(F32(1.0) < v, F32(1.0), v)).astype(F32)


def scan_cosine(dot64, q_nsq64, v_nsq64):
    """What the scan's similarity would give for the same pair: dot / (|row| * |q|) in fp64, rounded once — NOT the router."""
    with np.errstate(all="ignore"):
        cos = (np.asarray(dot64, np.float64) / (np.sqrt(v_nsq64) * np.sqrt(q_nsq64))).astype(F32)
        v = (cos + F32(1.0)) * F32(0.5)
        return np.where(v < F32(0.0), F32(0.0), np.where(F32(1.0) < v, F32(1.0), v)).astype(F32)


# ---- the table -----------------------------------------------------------------------------------------------------------------
class Table:
    """vectors [v][dim] cluster after cluster (the centroid first where has_centroid), offsets [c + 1], has_centroid [c],
    position [v] (a representative's place in the reference's list)."""

    def __init__(self, vectors, offsets, has_centroid, position):
        self.vectors = np.ascontiguousarray(vectors, F32)
        self.offsets = np.ascontiguousarray(offsets, np.uint32)
        self.has_centroid = np.ascontiguousarray(has_centroid, np.uint8)
        self.position = np.ascontiguousarray(position, np.uint16)
        self.n_clusters = len(self.offsets) - 1
        self.dim = self.vectors.shape[1]
        self._norms = None

    @property
    def norms(self):
        if self._norms is None:
            self._norms = norms(self.vectors)
        return self._norms

    def is_centroid(self):
        c = np.zeros(self.vectors.shape[0], bool)
        starts = self.offsets[:-1][(self.has_centroid != 0) & (self.offsets[1:] > self.offsets[:-1])]
        c[starts] = True
        return c


def pair_values(table, queries, rep_limit=0, candidates=None):
    """(value [q][v] float32, evaluated [q][v] bool): what the reference computes for every (query, row) it evaluates."""
    q = np.ascontiguousarray(queries, F32).reshape(-1, table.dim)
    qn, vn = norms(q), table.norms
    cen = table.is_centroid()
    owner = np.repeat(np.arange(table.n_clusters), np.diff(table.offsets.astype(np.int64)))
    with np.errstate(all="ignore"):
        ev_cen = (qn[:, None] > 0) & (vn[None, :] > 0)                      # :879 (a NaN norm fails it)
        ev_rep = ~((qn[:, None] <= 0) | (vn[None, :] <= 0))                  # :906 (a NaN norm passes it)
    inside = cen | (table.position < (rep_limit - 1 if rep_limit else CENTROID))
    ev = np.where(cen[None, :], ev_cen, ev_rep) & inside[None, :]
    if candidates is not None:
        ev &= np.asarray(candidates, bool).reshape(q.shape[0], table.n_clusters)[:, owner]
    val = map_cosine(chains(q, table.vectors), qn[:, None], vn[None, :])
    return val, ev


def dense_signal(table, queries, rep_limit=0, candidates=None):
    """(dense [q][c] float32, observed [q][c] bool, evaluations [q] uint32) — the loop :873-920, segment rank by segment rank."""
    val, ev = pair_values(table, queries, rep_limit, candidates)
    nq, c = val.shape[0], table.n_clusters
    dense = np.zeros((nq, c), F32)
    observed = np.zeros((nq, c), bool)
    off = table.offsets.astype(np.int64)
    size = np.diff(off)
    cen = table.is_centroid()
    for rank in range(int(size.max()) if c else 0):
        cl = np.nonzero(size > rank)[0]
        rows = off[cl] + rank
        d, e = val[:, rows], ev[:, rows]
        cur = dense[:, cl]
        with np.errstate(all="ignore"):
            folded = np.where(cur < d, d, cur)                               # std::max(cur, d)
        new = np.where(cen[rows][None, :], d, folded)                        # the centroid assigns
        dense[:, cl] = np.where(e, new, cur)
        observed[:, cl] |= e
    return dense, observed, ev.sum(axis=1).astype(np.uint32)


def dense_signal_scalar(table, query, rep_limit=0, candidates=None):
    """The same for one query, as the reference's loop reads (scalar, row by row): the cross-check of the vectorised form."""
    q = np.ascontiguousarray(query, F32)
    qn = norms(q[None, :])[0]
    dense, observed, evals = [], [], 0
    for k in range(table.n_clusters):
        cur, obs = F32(0.0), False
        if candidates is None or candidates[k]:
            for r in range(int(table.offsets[k]), int(table.offsets[k + 1])):
                vn = table.norms[r]
                centroid = bool(table.has_centroid[k]) and r == table.offsets[k]
                if centroid:
                    if not (qn > 0 and vn > 0):
                        continue
                else:
                    if rep_limit and table.position[r] >= rep_limit - 1:
                        continue
                    if qn <= 0 or vn <= 0:
                        continue
                d = map_cosine(chains(q[None, :], table.vectors[r][None, :])[0, 0], qn, vn)[()]
                cur = d if centroid else (d if cur < d else cur)
                obs = True
                evals += 1
        dense.append(cur)
        observed.append(obs)
    return np.array(dense, F32), np.array(observed, bool), evals


# ---- a host's artifacts -> the table (what the shell does) -------------------------------------------------------------------
def table_of(clusters, dim):
    """clusters: [{"centroid": float32 array (may be empty), "reps": [float32 arrays]}].  Vectors of another size than dim are
    left out and their positions still count; a non-empty centroid of another size cannot be served (None)."""
    vec, off, has, pos = [], [0], [], []
    for cl in clusters:
        cen = np.asarray(cl["centroid"], F32)
        if cen.size and cen.size != dim:
            return None
        has.append(1 if cen.size else 0)
        if cen.size:
            vec.append(cen); pos.append(0)
        for p, r in enumerate(cl["reps"]):
            r = np.asarray(r, F32)
            if r.size == dim:
                vec.append(r); pos.append(p)
        off.append(len(vec))
    v = np.stack(vec) if vec else np.zeros((0, dim), F32)
    return Table(v, off, has, pos)


# ---- the whole route (:771-981) -------------------------------------------------------------------------------------------------
def route(case, ann=None):
    """case: {"clusters": [{"id", "centroid", "reps", "members": [hash], "member_count", "persistence", "cohesion"}],
    "request": {"query", "alpha", "max_reps", "ann_limit", "limit", "mode", "seeds": [hash], "weighted": [[hash, weight]]}}.
    ann(query, limit) -> (hit ids, distance evaluations) or None (no index / refused).  Returns {"routes": [...], "work": {...}}."""
    clusters, rq = case["clusters"], case["request"]
    c = len(clusters)
    work = {"seed_lookups": 0, "query_norms": 0, "evaluations": 0, "exact_evaluations": 0, "ann_used": False, "ann_candidates": 0,
            "ann_evaluations": 0}
    by_hash = {}
    for k, cl in enumerate(clusters):
        for h in cl["members"]:
            by_hash.setdefault(h, []).append(k)
    mass = [0.0] * c
    weighted = {}
    for h, w in rq["weighted"]:
        w = F32(w)
        if not h or not np.isfinite(w) or w <= 0:
            continue
        weighted[h] = max(weighted[h], w) if h in weighted else w
    if weighted:
        for h, w in weighted.items():
            work["seed_lookups"] += 1
            for k in by_hash.get(h, []):
                mass[k] += float(w)
    else:
        for h in set(rq["seeds"]):
            work["seed_lookups"] += 1
            for k in by_hash.get(h, []):
                mass[k] += 1.0
    max_mass = max([0.0] + mass)
    alpha = F32(min(max(F32(rq["alpha"]), F32(0.0)), F32(1.0)))
    query = np.asarray(rq["query"], F32)
    qn = norms(query[None, :])[0] if query.size else F32(0.0)
    if query.size:
        work["query_norms"] += 1
    cand = [True] * c
    cnorm = [norms(np.asarray(cl["centroid"], F32)[None, :])[0] if len(cl["centroid"]) else F32(0.0) for cl in clusters]
    has_index = ann is not None and c > 0 and all(len(cl["centroid"]) and cnorm[k] > 0 for k, cl in enumerate(clusters))
    if alpha < 1 and qn > 0 and rq["limit"] > 0 and rq["ann_limit"] > 0 and has_index and c > rq["ann_limit"]:
        res = ann(query, min(c, max(rq["ann_limit"], rq["limit"])))
        if res is not None:
            hits, n_eval = res
            cand = [False] * c
            for h in hits:
                if h < c:
                    cand[h] = True
            for k in range(c):
                if mass[k] > 0.0:
                    cand[k] = True
            work.update(ann_used=True, ann_candidates=len(hits), ann_evaluations=n_eval)
            work["evaluations"] += n_eval
    dense = np.zeros(c, F32)
    observed = np.zeros(c, bool)
    if alpha < 1 and c:
        # the reference's own loop, with its own size tests (:670, :879, :907)
        for k, cl in enumerate(clusters):
            if not cand[k]:
                continue
            cen = np.asarray(cl["centroid"], F32)
            if qn > 0 and cnorm[k] > 0 and cen.size:
                dot = chains(query[None, :], cen[None, :])[0, 0] if cen.size == query.size else 0.0
                dense[k] = map_cosine(dot, qn, cnorm[k])[()]
                observed[k] = True
                work["evaluations"] += 1; work["exact_evaluations"] += 1
            limit = len(cl["reps"]) if rq["max_reps"] == 0 else min(len(cl["reps"]), rq["max_reps"] - 1)
            for p in range(limit):
                r = np.asarray(cl["reps"][p], F32)
                rn = norms(r[None, :])[0] if r.size else F32(0.0)
                if qn <= 0 or rn <= 0 or r.size != query.size:
                    continue
                d = map_cosine(chains(query[None, :], r[None, :])[0, 0], qn, rn)[()]
                dense[k] = d if dense[k] < d else dense[k]
                observed[k] = True
                work["evaluations"] += 1; work["exact_evaluations"] += 1
    index_norms = []
    for k, cl in enumerate(clusters):
        index_norms.append(cnorm[k])
        index_norms += [norms(np.asarray(r, F32)[None, :])[0] if len(r) else F32(0.0) for r in cl["reps"]]
    return {"routes": finish_route(case, cand, mass, max_mass, alpha, dense, observed), "work": work, "norms": index_norms,
            "dense": dense, "observed": observed, "candidates": cand}


def finish_route(case, cand, mass, max_mass, alpha, dense, observed):
    """:922-980 — blend, scoring mode, sort by (routeScore desc, clusterId asc), cut."""
    rq = case["request"]
    routes = []
    with np.errstate(all="ignore"):
        for k, cl in enumerate(case["clusters"]):
            if not cand[k]:
                continue
            d = F32(dense[k])
            sparse = F32(mass[k] / max_mass) if max_mass > 0.0 else F32(0.0)
            blended = float(F32(F32(alpha * sparse) + F32(F32(F32(1.0) - alpha) * d)))
            cohesion = min(max(cl["cohesion"], 0.0), 1.0)
            stability = min(max(cl["persistence"], 0.0), 1.0)
            damp = 1.0 / (1.0 + math.log1p(float(cl["member_count"])))
            score = blended + cl["persistence"] * 0.05
            if rq["mode"] == "size_weighted":
                score = (blended + 0.05 * stability + 0.05 * cohesion) * damp
            elif rq["mode"] == "seed_coverage":
                score = float(sparse) + 0.10 * float(d) + cl["persistence"] * 0.05
            routes.append({"id": cl["id"], "score": float(score), "semantic_cost": (1.0 - float(d)) if observed[k] else None,
                           "sparse_cost": (1.0 - float(sparse)) if max_mass > 0.0 else None})
    routes.sort(key=lambda r: r["id"])
    routes.sort(key=lambda r: -r["score"] if r["score"] == r["score"] else 0.0)     # (golden cases keep a NaN score alone)
    if rq["limit"] > 0 and len(routes) > rq["limit"]:
        routes = routes[:rq["limit"]]
    return routes


def hexd(x):
    return None if x is None else ("nan" if x != x else float(x).hex())


def routes_hex(result):
    """The form the golden file keeps: doubles as hex strings, a NaN as "nan"."""
    return {"routes": [[r["id"], hexd(r["score"]), hexd(r["semantic_cost"]), hexd(r["sparse_cost"])] for r in result["routes"]],
            "work": result["work"], "norms": [int(b) for b in bits(np.array(result["norms"], F32))]}


# ---- seeded shapes for the device tests --------------------------------------------------------------------------------------
def random_table(rng, dim, sizes, centroid_prob=0.85, special=False):
    """A table with segment sizes `sizes` (rows per cluster, centroid included where it has one)."""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    v = int(off[-1])
    x = rng.standard_normal((v, dim)).astype(F32)
    has = np.array([1 if (s > 64 or (s > 0 and rng.random() < centroid_prob)) else 0 for s in sizes], np.uint8)      # (65 rows need a centroid)
    pos = np.zeros(v, np.uint16)
    for k, s in enumerate(sizes):
        n_rep = s - int(has[k])
        # places in the reference's list: increasing, with gaps where the reference skipped a vector of another size
        p = np.cumsum(rng.integers(1, 3, n_rep)) - 1 if n_rep else np.zeros(0, np.int64)
        pos[off[k] + int(has[k]):off[k + 1]] = p
    if special and v:
        for r in rng.choice(v, size=min(v, max(1, v // 8)), replace=False):
            kind = rng.integers(0, 6)
            if kind == 0: x[r] = 0.0
            elif kind == 1: x[r, rng.integers(0, dim)] = np.nan
            elif kind == 2: x[r, rng.integers(0, dim)] = np.inf
            elif kind == 3: x[r] *= F32(1e-30)
            elif kind == 4: x[r] = np.where(rng.random(dim) < 0.5, 1, -1).astype(F32) * F32(8.5e37)
            else: x[r] *= F32(1e-23)
    return Table(x, off, has, pos)


# ---- the golden cases (tests/golden/cluster_route.json: what the REFERENCE'S route returns for them) --------------------------
def _cluster(cid, centroid, reps, members=(), member_count=None, persistence=0.0, cohesion=0.0):
    return {"id": cid, "centroid": np.asarray(centroid, F32), "reps": [np.asarray(r, F32) for r in reps], "members": list(members),
            "member_count": len(members) if member_count is None else member_count, "persistence": persistence, "cohesion": cohesion}


def _request(query, alpha=0.0, max_reps=0, ann_limit=0, limit=8, mode="current", seeds=(), weighted=()):
    return {"query": np.asarray(query, F32), "alpha": alpha, "max_reps": max_reps, "ann_limit": ann_limit, "limit": limit, "mode": mode,
            "seeds": list(seeds), "weighted": [list(w) for w in weighted]}


def _plain_clusters(seed=5, c=5, dim=8, reps=3):
    rng = np.random.default_rng(seed)
    return [_cluster("c%02d" % k, rng.standard_normal(dim), [rng.standard_normal(dim) for _ in range(reps)],
                     members=["doc-%d-%d" % (k, i) for i in range(k + 1)], persistence=0.1 * k, cohesion=1.0 - 0.15 * k)
            for k in range(c)]


def _query(seed=6, dim=8):
    return np.random.default_rng(seed).standard_normal(dim).astype(F32)


def _golden_cases():
    cases = {}

    def add(name, clusters, request, ann_builds=False):
        cases[name] = {"clusters": clusters, "request": request, "ann_builds": ann_builds}

    add("plain", _plain_clusters(), _request(_query()))
    cl = _plain_clusters()
    cl[1]["centroid"] = np.zeros(0, F32)
    add("empty_centroid_with_representatives", cl, _request(_query()))
    for m in (0, 1, 2, 3, 10):
        add("max_representatives_%d" % m, _plain_clusters(), _request(_query(), max_reps=m))
    # a zero-norm representative in front of a live one: position 0 is looked at and skipped, and it still uses up the limit
    for m in (2, 3):
        cl = _plain_clusters(c=3)
        for k in cl:
            k["reps"][0] = np.zeros(8, F32)
            k["reps"][1] = (_query() * F32(3.0)).astype(F32)      # the live one is the query's direction: dense 1.0 when reached
        add("zero_representative_first_max_%d" % m, cl, _request(_query(), max_reps=m))
    # a representative of another size: not scored, its place still counts
    for m in (0, 3):
        cl = _plain_clusters(c=3)
        for k in cl:
            k["reps"][1] = np.ones(4, F32)
        add("representative_of_another_size_max_%d" % m, cl, _request(_query(), max_reps=m))
    # NaN / inf elements.  A NaN norm fails the centroid's test and passes the representatives': observed, counted, ignored.
    q = _query(); q[2] = np.nan
    add("nan_in_query", _plain_clusters(), _request(q))
    q = _query(); q[2] = np.inf                                     # every dense is a NaN: one cluster, the sort has nothing to do
    add("inf_in_query", _plain_clusters(c=1), _request(q))
    cl = _plain_clusters(); cl[2]["centroid"][1] = np.nan
    add("nan_in_centroid", cl, _request(_query()))
    cl = _plain_clusters(c=1); cl[0]["centroid"][1] = np.inf       # the centroid assigns a NaN, which survives the representatives
    add("inf_in_centroid", cl, _request(_query()))
    cl = _plain_clusters(); cl[2]["reps"][0][1] = np.nan; cl[3]["reps"][2][0] = -np.inf
    add("nan_and_inf_in_representatives", cl, _request(_query()))
    cl = _plain_clusters(); cl[0]["centroid"] = np.zeros(0, F32); cl[0]["reps"] = [r * F32(np.nan) for r in cl[0]["reps"]]
    add("only_nan_representatives", cl, _request(_query()))        # observed with dense 0.0
    # norms whose float product is a denormal (1e-40): the divide must keep it
    tiny = np.zeros(8, F32); tiny[0] = F32(1e-20); tiny[3] = F32(-2e-21)
    cl = [_cluster("c00", tiny * F32(2), [tiny, -tiny]), _cluster("c01", -tiny, [np.roll(tiny, 1)])]
    add("norm_product_denormal", cl, _request(tiny))
    # ... and zero (1e-60): 0 / 0 with positive norms
    t2 = np.zeros(8, F32); t2[0] = F32(1e-30)
    add("norm_product_zero", [_cluster("c00", t2, [t2 * F32(2)])], _request(t2))
    # a dot that rounds to a float denormal between unit vectors
    a = np.zeros(8, F32); a[0] = 1.0
    b = np.zeros(8, F32); b[0] = F32(1e-40); b[1] = 1.0
    add("dot_denormal", [_cluster("c00", b, [-b]), _cluster("c01", -b, [b, a])], _request(a))
    # +-FLT_MAX / 4 rows: the float cast of the dot is inf, the norms' product too
    big = np.where(np.arange(8) % 2 == 0, 1, -1).astype(F32) * F32(np.finfo(F32).max / 4)
    add("flt_max_quarter", [_cluster("c00", big, [-big, np.abs(big)])], _request(big))
    # a candidate mask: the ANN shortlist (the stand-in answers with the first clusters) united with the weighted seeds' clusters
    cl = _plain_clusters(c=7)
    w = [["doc-5-0", 0.5], ["doc-5-1", 2.0], ["doc-3-0", 1.0], ["doc-5-1", 1.0], ["nobody", 4.0], ["doc-6-0", -1.0], ["", 1.0]]
    add("candidate_mask_weighted_seeds", cl, _request(_query(), alpha=0.25, ann_limit=2, limit=2, weighted=w), ann_builds=True)
    add("candidate_mask_plain_seeds_limit", cl, _request(_query(), alpha=0.5, ann_limit=1, limit=3, seeds=["doc-4-0", "doc-4-1", "doc-6-2"]),
        ann_builds=True)
    for mode in MODES:
        add("mode_" + mode, _plain_clusters(), _request(_query(), alpha=0.5, mode=mode, seeds=["doc-1-0", "doc-4-2", "doc-4-3"], limit=4))
    add("alpha_one_scores_nothing", _plain_clusters(), _request(_query(), alpha=1.0, seeds=["doc-2-0"]))
    return cases


GOLDEN_CASES = _golden_cases()


def standin_ann(case):
    """The golden maker's stand-in ANN index: it builds only where the case says so, and answers with the first `limit`
    clusters and 3 evaluations per cluster of the index."""
    if not case["ann_builds"]:
        return None
    c = len(case["clusters"])
    return lambda query, limit: (list(range(min(limit, c))), 3 * c)


def case_digest(case):
    arrays = []
    for cl in case["clusters"]:
        arrays += [cl["centroid"]] + cl["reps"]
    rq = case["request"]
    meta = [[cl["id"], cl["members"], cl["member_count"], cl["persistence"], cl["cohesion"]] for cl in case["clusters"]]
    meta += [float(rq["alpha"]), rq["max_reps"], rq["ann_limit"], rq["limit"], rq["mode"], rq["seeds"], rq["weighted"], case["ann_builds"]]
    import json
    return digest(*arrays, rq["query"], np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8))


def write_case(path, case):
    """The binary form tests/cpp/route_shell_test.cpp reads."""
    def s(x):
        b = x.encode()
        return struct.pack("<I", len(b)) + b

    def v(x):
        x = np.ascontiguousarray(x, F32)
        return struct.pack("<I", x.size) + x.tobytes()
    out = [struct.pack("<I", len(case["clusters"]))]
    for cl in case["clusters"]:
        out += [s(cl["id"]), v(cl["centroid"]), struct.pack("<I", len(cl["reps"]))]
        out += [s("rep-%d" % i) + v(r) for i, r in enumerate(cl["reps"])]
        out += [struct.pack("<I", len(cl["members"]))] + [s(h) for h in cl["members"]]
        out += [struct.pack("<Qdd", cl["member_count"], cl["persistence"], cl["cohesion"])]
    rq = case["request"]
    out += [v(rq["query"]), struct.pack("<fQQQB", rq["alpha"], rq["max_reps"], rq["ann_limit"], rq["limit"], MODES.index(rq["mode"]))]
    out += [struct.pack("<I", len(rq["seeds"]))] + [s(h) for h in rq["seeds"]]
    out += [struct.pack("<I", len(rq["weighted"]))] + [s(h) + struct.pack("<f", w) for h, w in rq["weighted"]]
    out += [struct.pack("<B", 1 if case["ann_builds"] else 0)]
    with open(path, "wb") as f:
        f.write(b"".join(out))


def parse_driver(text):
    """The driver's lines -> the form routes_hex gives."""
    def h(tok):
        if tok == "none":
            return None
        return "nan" if "nan" in tok else float.fromhex(tok).hex()
    routes, work, out = [], None, {}
    for line in text.splitlines():
        t = line.split()
        if t and t[0] == "route":
            routes.append([t[1], h(t[2]), h(t[3]), h(t[4])])
        elif t and t[0] == "work":
            n = [int(x) for x in t[1:]]
            work = {"seed_lookups": n[0], "query_norms": n[1], "evaluations": n[2], "exact_evaluations": n[3], "ann_used": bool(n[4]),
                    "ann_candidates": n[5], "ann_evaluations": n[6]}
        elif t and t[0] == "norms":
            out["norms"] = [int(x) for x in t[1:]]
        elif t and t[0] == "error":
            out["error"] = line
    out.update(routes=routes, work=work)
    return out


def same_result(got, want):
    """Two results in the golden file's form: everything equal, where a NaN norm matches any NaN norm."""
    gn, wn = np.array(got["norms"], np.uint32).view(F32), np.array(want["norms"], np.uint32).view(F32)
    return got["routes"] == want["routes"] and got["work"] == want["work"] and same_bits(gn, wn)
