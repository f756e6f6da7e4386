"""Restatement of the tail every topology engine of the reference runs after clustering, for the tests of
yams_cluster_centroids / _representatives / _residuals and of the shell include/yams_accel/topology_artifacts.hpp:

  detail::meanEmbedding                      src/topology/topology_build_utils.h:27-56
  cosineDistance, the selection loop         src/topology/topology_representatives.cpp:13-29, :33-91
  applyOrthogonalBoundarySpill               :93-287 (the path without the centroid ANN index: every cluster is a candidate)

Every chain is computed in the reference's order.  The residual chains exist in both forms a host compiler can give them:
SEPARATE (a rounded multiply, then a rounded add) and FUSED (one fma per `+=`); the fma is exact integer arithmetic (fma()
below), because this Python has no math.fma.  The only tolerance anywhere: a NaN matches any NaN.
"""
import functools
import hashlib
import math

import numpy as np

NONE = 0xFFFFFFFF
SEPARATE, FUSED = 0, 1
MAX_REPRESENTATIVES = 64
F32_MAX = float(np.finfo(np.float32).max)


def f32(a):
    return np.ascontiguousarray(a, np.uint32).view(np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- an exact fma ------------------------------------------------------------------------------------------------------------
def _round_scaled(n, e):
    """The double nearest n * 2**e (ties to even), n a non-zero integer; overflow gives +-inf."""
    sign = -1.0 if n < 0 else 1.0
    n = abs(n)
    lsb = max(e + n.bit_length() - 53, -1074)
    shift = lsb - e
    if shift > 0:
        q, r = divmod(n, 1 << shift)
        half = 1 << (shift - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
    else:
        q, lsb = n, e
    try:
        return sign * math.ldexp(float(q), lsb)
    except OverflowError:
        return sign * math.inf


def fma(a, b, c):
    """a * b + c with one rounding."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)) or a == 0.0 or b == 0.0:
        return a * b + c      # a product that is exact (a zero) or special: the IEEE add decides, signs included
    ma, ea = math.frexp(a)
    mb, eb = math.frexp(b)
    p, e = int(ma * (1 << 53)) * int(mb * (1 << 53)), ea + eb - 106
    if c != 0.0:
        mc, ec = math.frexp(c)
        ic, ec = int(mc * (1 << 53)), ec - 53
        e0 = min(e, ec)
        p, e = (p << (e - e0)) + (ic << (ec - e0)), e0
        if p == 0:
            return 0.0      # an exact cancellation of non-zero terms: +0.0 under round to nearest
    return _round_scaled(p, e)


# ---- centroids ---------------------------------------------------------------------------------------------------------------
def centroids(x, off, members):
    """meanEmbedding per cluster: (centroids [c][dim] float32 (zeros for an empty cluster), counts [c] uint32)."""
    x = np.ascontiguousarray(x, np.float32)
    off = np.asarray(off, np.int64)
    c, dim = len(off) - 1, x.shape[1]
    out = np.zeros((c, dim), np.float32)
    with np.errstate(all="ignore"):
        for k in range(c):
            lst = members[off[k]:off[k + 1]]
            if len(lst) == 0:
                continue
            s = np.zeros(dim, np.float32)
            for m in lst:
                s = s + x[int(m)]
            out[k] = s / np.float32(len(lst))
    return out, np.diff(off).astype(np.uint32)


# ---- the selection -----------------------------------------------------------------------------------------------------------
def chain_sq(v):
    """lhsNorm of every row of v [m][dim]: fp64, element order (the products are exact)."""
    v = np.ascontiguousarray(v, np.float32).astype(np.float64)
    s = np.zeros(v.shape[0])
    with np.errstate(all="ignore"):
        for d in range(v.shape[1]):
            s = s + v[:, d] * v[:, d]
    return s


def cosine_distance(a, t):
    """cosineDistance(a[i], t) for every row of a [m][dim] against one vector t [dim]."""
    a = np.ascontiguousarray(a, np.float32).astype(np.float64)
    t = np.ascontiguousarray(t, np.float32).astype(np.float64)
    dot = np.zeros(a.shape[0])
    with np.errstate(all="ignore"):
        for d in range(a.shape[1]):
            dot = dot + a[:, d] * t[d]
        na, nb = chain_sq(a.astype(np.float32)), float(chain_sq(t.astype(np.float32)[None, :])[0])
        c = dot / (np.sqrt(na) * np.sqrt(nb))
        cl = np.where(c < -1.0, -1.0, np.where(1.0 < c, 1.0, c))      # std::clamp: a NaN passes
        d = 1.0 - cl
    d[(na <= 0.0) | (nb <= 0.0)] = 2.0
    return d


def select_positions(x, cand_rows, centroid, n_extra):
    """The loop of :58-90: positions in cand_rows, in selection order."""
    m = len(cand_rows)
    limit = min(n_extra, m)
    rows = np.ascontiguousarray(x, np.float32)[np.asarray(cand_rows, np.int64)] if m else np.zeros((0, len(centroid)), np.float32)
    used = np.zeros(m, bool)
    min_d = np.full(m, np.finfo(np.float64).max)
    sel = []
    for s in range(limit):
        target = centroid if s == 0 else rows[sel[-1]]
        d = cosine_distance(rows, target)
        upd = ~used & (d < min_d)      # std::min(minDist, d) = d < minDist ? d : minDist
        min_d[upd] = d[upd]
        best, best_d = m, -1.0
        for i in range(m):
            if not used[i] and min_d[i] > best_d:
                best, best_d = i, min_d[i]
        if best == m:
            break
        used[best] = True
        sel.append(best)
    return sel


def representatives(x, off, cand, cents, n_extra, empty=None):
    """(selected [c][n_extra] uint32, NONE in unused slots; counts [c])"""
    off = np.asarray(off, np.int64)
    c = len(off) - 1
    out = np.full((c, n_extra), NONE, np.uint32)
    cnt = np.zeros(c, np.uint32)
    for k in range(c):
        if empty is not None and empty[k]:
            continue
        sel = select_positions(x, cand[off[k]:off[k + 1]], cents[k], n_extra)
        out[k, :len(sel)] = sel
        cnt[k] = len(sel)
    return out, cnt


# ---- residuals ---------------------------------------------------------------------------------------------------------------
def _chains(e, pc, cc, form):
    """e, cc [p][dim] float32 (document, candidate centroid), pc [p][dim] float32 or None (primary centroid).  Returns
    (candidateNormSquared [p], residualDot [p]) in the given form."""
    e64, c64 = e.astype(np.float64), cc.astype(np.float64)
    with np.errstate(all="ignore"):
        r = e64 - c64
        q = (e64 - pc.astype(np.float64)) if pc is not None else np.zeros_like(r)
        p, dim = r.shape
        if form == SEPARATE:
            nrm, dot = np.zeros(p), np.zeros(p)
            for d in range(dim):
                nrm = nrm + r[:, d] * r[:, d]
                dot = dot + q[:, d] * r[:, d]
            return nrm, dot
    nrm, dot = np.zeros(p), np.zeros(p)
    for i in range(p):
        a = b = 0.0
        ri, qi = r[i].tolist(), q[i].tolist()
        for d in range(dim):
            a = fma(ri[d], ri[d], a)
            b = fma(qi[d], ri[d], b)
        nrm[i], dot[i] = a, b
    return nrm, dot


def residuals(x, cents, primary=None, cand_off=None, cand=None, form=SEPARATE):
    """(primary_norm_sq [n] or None, cand_norm_sq [pairs], residual_dot [pairs] or None).  Dense (cand_off None): pair
    (u, c) at u * n_clusters + c."""
    x = np.ascontiguousarray(x, np.float32)
    cents = np.ascontiguousarray(cents, np.float32).reshape(-1, x.shape[1])
    n, c = x.shape[0], cents.shape[0]
    if cand_off is None:
        doc = np.repeat(np.arange(n), c)
        cl = np.tile(np.arange(c), n)
    else:
        cand_off = np.asarray(cand_off, np.int64)
        doc = np.repeat(np.arange(n), np.diff(cand_off))
        cl = np.asarray(cand, np.int64)[:cand_off[-1]]
    zeros = np.zeros((1, x.shape[1]), np.float32)
    cz = np.vstack([cents, zeros])
    if primary is None:
        nrm, _ = _chains(x[doc], None, cents[cl], form)
        return None, nrm, None
    pri = np.asarray(primary, np.int64)
    has = pri != NONE
    pidx = np.where(has, pri, c)
    pn, _ = _chains(x, None, cz[pidx], form)      # primaryNormSquared is the candidate chain against the primary centroid
    pn[~has] = 0.0
    nrm, dot = _chains(x[doc], cz[pidx[doc]], cents[cl], form)
    dot[~has[doc]] = 0.0
    return pn, nrm, dot


# ---- the two public functions, restated over documents (for the golden file and the shell's tests) -----------------------------
def select_diverse(docs, members, centroid, count):
    """selectDiverseRoutingRepresentatives: the hashes selected.  docs: [{"hash", "emb"}]."""
    if count <= 1 or len(centroid) == 0:
        return []
    cands = [m for m in members if m < len(docs) and docs[m]["hash"] and len(docs[m]["emb"]) == len(centroid)
             and np.isfinite(np.asarray(docs[m]["emb"], np.float32)).all()]
    cands.sort(key=lambda m: docs[m]["hash"].encode())      # (std::sort is not stable: the cases use distinct hashes)
    x = np.array([docs[m]["emb"] for m in cands], np.float32).reshape(len(cands), len(centroid))
    sel = select_positions(x, list(range(len(cands))), np.asarray(centroid, np.float32), count - 1)
    return [docs[cands[i]]["hash"] for i in sel]


def mean_embedding(docs, members):
    """detail::meanEmbedding: the first non-empty member fixes the size, members of another size are skipped."""
    rows = []
    for m in members:
        if m >= len(docs) or len(docs[m]["emb"]) == 0:
            continue
        if rows and len(docs[m]["emb"]) != len(rows[0]):
            continue
        rows.append(np.asarray(docs[m]["emb"], np.float32))
    if not rows:
        return np.zeros(0, np.float32)
    cent, _ = centroids(np.array(rows, np.float32), [0, len(rows)], list(range(len(rows))))
    return cent[0]


def boundary_spill(docs, cfg, clusters, memberships, form=SEPARATE):
    """applyOrthogonalBoundarySpill without an ANN index.  clusters: [{"id", "members": [hash], "centroid"}]; memberships:
    [{"hash", "cluster", "role_outlier", "overlap": []}] — both edited in place.  Returns the assignment count."""
    ratio, penalty, limit = cfg["ratio"], cfg["penalty"], cfg["limit"]
    if (not cfg.get("allow", True) or limit == 0 or len(clusters) < 2 or not math.isfinite(ratio) or ratio < 1.0
            or not math.isfinite(penalty) or penalty < 0.0):
        return 0
    by_hash = {}
    for d in docs:
        if d["hash"] and len(d["emb"]) and d["hash"] not in by_hash:
            by_hash[d["hash"]] = d
    index_of = {}
    for i, cl in enumerate(clusters):
        if cl["id"] and cl["id"] not in index_of:
            index_of[cl["id"]] = i
    eps = 1e-12

    def chains(emb, pc, cc):
        e = np.asarray(emb, np.float32)[None, :]
        n, d = _chains(e, None if pc is None else np.asarray(pc, np.float32)[None, :], np.asarray(cc, np.float32)[None, :], form)
        return float(n[0]), float(d[0])

    radius = [0.0] * len(clusters)
    for i, cl in enumerate(clusters):
        for h in cl["members"]:
            d = by_hash.get(h)
            if d is None or len(d["emb"]) != len(cl["centroid"]):
                continue
            r2 = chains(d["emb"], None, cl["centroid"])[0] if len(cl["centroid"]) else 0.0
            if math.isfinite(r2):
                radius[i] = max(radius[i], r2)
    assignments = 0
    ratio2 = ratio * ratio
    for ms in memberships:
        if ms["overlap"]:
            continue
        d = by_hash.get(ms["hash"])
        if d is None or ms["cluster"] not in index_of:
            continue
        pi = index_of[ms["cluster"]]
        emb, pc = d["emb"], clusters[pi]["centroid"]
        if len(emb) != len(pc) or len(emb) == 0:
            continue
        pn = chains(emb, None, pc)[0]
        if not math.isfinite(pn):
            continue
        observed = pn > eps
        if not observed and not ms["role_outlier"]:
            continue
        cands = []
        for ci, cl in enumerate(clusters):
            if ci == pi or len(cl["centroid"]) != len(emb):
                continue
            cn, rd = chains(emb, pc, cl["centroid"])
            if not math.isfinite(cn):
                continue
            loss = cn
            if observed:
                if cn > pn * ratio2:
                    continue
                loss += penalty * ((rd * rd) / pn)
            else:
                if radius[ci] <= eps or cn > radius[ci] * ratio2:
                    continue
            if math.isfinite(loss):
                cands.append((ci, loss))

        def before(a, b):
            if abs(a[1] - b[1]) > eps:
                return a[1] < b[1]
            return clusters[a[0]]["id"].encode() < clusters[b[0]]["id"].encode()
        cands.sort(key=functools.cmp_to_key(lambda a, b: -1 if before(a, b) else (1 if before(b, a) else 0)))
        for ci, _ in cands[:limit]:
            sec = clusters[ci]
            if ms["hash"] not in sec["members"]:
                sec["members"].append(ms["hash"])
                sec["members"].sort(key=lambda h: h.encode())
            ms["overlap"].append(sec["id"])
            assignments += 1
    return assignments


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------
def random_rows(rng, n, dim, scale=1.0):
    return (rng.standard_normal((n, dim)) * scale).astype(np.float32)


def clustered_case(seed, sizes, dim, order="scrambled", specials=True):
    """Rows and CSR member lists with the given cluster sizes (0 allowed).  order: the order inside a list ("scrambled",
    "descending", "ascending").  specials: some rows become exact duplicates of their neighbour, one a zero row."""
    rng = np.random.default_rng(seed)
    n = max(int(sum(sizes)), 1)
    x = random_rows(rng, n, dim)
    if specials and n >= 6:
        x[3] = x[2]; x[n - 1] = x[n - 2]
        x[4] = 0.0
    perm = rng.permutation(n)
    off, members, at = [0], [], 0
    for s in sizes:
        lst = perm[at:at + s]
        at += s
        lst = np.sort(lst) if order == "ascending" else (np.sort(lst)[::-1] if order == "descending" else lst)
        members.extend(int(v) for v in lst)
        off.append(len(members))
    return x, np.array(off, np.uint64), np.array(members, np.uint32)


def residual_case(seed, n, c, dim, list_len=None):
    """Rows near c centroids, a primary per document (some NONE), and, with list_len, scrambled candidate lists with repeats
    and the primary included."""
    rng = np.random.default_rng(seed)
    cents = random_rows(rng, c, dim)
    pri = rng.integers(0, c, n).astype(np.uint32)
    x = (cents[pri] + rng.standard_normal((n, dim)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    pri[rng.random(n) < 0.1] = NONE
    if list_len is None:
        return x, cents, pri, None, None
    off, cand = [0], []
    for u in range(n):
        m = list_len if u % 5 else int(rng.integers(0, list_len))
        lst = rng.integers(0, c, m)
        if m >= 2 and pri[u] != NONE:
            lst[int(rng.integers(0, m))] = pri[u]
        cand.extend(int(v) for v in lst)
        off.append(len(cand))
    return x, cents, pri, np.array(off, np.uint64), np.array(cand, np.uint32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---- the golden cases: whole documents through mean -> representatives -> spill (tests/golden/cluster_artifacts.json) ---------
def _hash(i):
    return hashlib.sha256(b"doc%d" % i).hexdigest()[:12]


def golden_case(seed, sizes, dim, count, limit=1, ratio=1.05, penalty=1.0, special=None):
    """Documents in clusters (blobs near `len(sizes)` centres), hashes in no row order.  special: "duplicates" (exact duplicate
    rows and a zero row), "huge" (one cluster of +-FLT_MAX/4 rows: its fp32 mean overflows), "ragged" (a document of another
    size, one without a hash, one non-finite, an unknown member hash)."""
    rng = np.random.default_rng(seed)
    centres = random_rows(rng, len(sizes), dim)
    docs, clusters, memberships = [], [], []
    for k, size in enumerate(sizes):
        members = []
        for _ in range(size):
            i = len(docs)
            emb = (centres[k] + rng.standard_normal(dim).astype(np.float32) * np.float32(0.6)).astype(np.float32)
            docs.append({"hash": _hash(i), "emb": emb})
            members.append(i)
        if special == "duplicates" and size >= 6:
            docs[members[1]]["emb"] = docs[members[0]]["emb"].copy(); docs[members[3]]["emb"] = docs[members[0]]["emb"].copy()
            docs[members[4]]["emb"] = np.zeros(dim, np.float32)
        if special == "huge" and k == 0:
            for j, m in enumerate(members):
                docs[m]["emb"] = np.full(dim, F32_MAX / 4 * (1 if j % 5 else -1), np.float32) * np.float32(1 - j / 1000)
        if special == "ragged" and size >= 5:
            docs[members[0]]["emb"] = docs[members[0]]["emb"][:max(1, dim - 1)].copy() if k else docs[members[0]]["emb"]
            if k == 0:
                docs[members[2]]["emb"] = np.where(np.arange(dim) == 1, np.float32(np.inf), docs[members[2]]["emb"]).astype(np.float32)
        hashes = sorted(docs[m]["hash"] for m in members)      # the reference sorts a cluster's members by hash
        if special == "ragged" and k == 1:
            hashes.append("zz-unknown")
        clusters.append({"id": "c%02d" % ((k * 7) % len(sizes)) if len(sizes) > 1 else "c00", "members": hashes})
        for j, m in enumerate(members):
            memberships.append({"hash": docs[m]["hash"], "cluster": clusters[-1]["id"], "role_outlier": bool(j == 1 and special == "duplicates"),
                                "overlap": []})
    return docs, clusters, memberships, {"limit": limit, "ratio": ratio, "penalty": penalty, "count": count}


GOLDEN_CASES = {
    "blobs_r3": lambda: golden_case(1, [40, 35, 30, 25], 16, 3, limit=2, ratio=1.5),
    "blobs_r2_dim1": lambda: golden_case(2, [20, 20, 9], 1, 2, limit=1, ratio=2.0),
    "duplicates_and_zero_rows": lambda: golden_case(3, [12, 7, 65], 5, 4, limit=2, ratio=1.3, penalty=0.5, special="duplicates"),
    "huge_cluster_overflows": lambda: golden_case(4, [8, 10, 6], 4, 3, limit=1, ratio=1.2, special="huge"),
    "r_beyond_the_cluster": lambda: golden_case(5, [3, 1, 2, 30], 7, 64, limit=3, ratio=1.4, penalty=0.0),
    "ragged_documents": lambda: golden_case(6, [9, 8, 7], 6, 3, limit=2, ratio=4.0, special="ragged"),
    "wide_64": lambda: golden_case(7, [100, 90, 60, 50], 64, 5, limit=2, ratio=3.0, penalty=2.0),
}


def write_case(path, docs, clusters, memberships, cfg):
    import struct
    s = lambda t: struct.pack("<I", len(t.encode())) + t.encode()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(docs)))
        for d in docs:
            f.write(s(d["hash"])); f.write(struct.pack("<I", len(d["emb"]))); f.write(np.asarray(d["emb"], np.float32).tobytes())
        f.write(struct.pack("<I", len(clusters)))
        for c in clusters:
            f.write(s(c["id"])); f.write(struct.pack("<I", len(c["members"])))
            for h in c["members"]:
                f.write(s(h))
        f.write(struct.pack("<I", len(memberships)))
        for m in memberships:
            f.write(s(m["hash"])); f.write(s(m["cluster"])); f.write(b"\1" if m["role_outlier"] else b"\0")
        f.write(struct.pack("<QddQ", cfg["limit"], cfg["ratio"], cfg["penalty"], cfg["count"]))


def run_case(docs, clusters, memberships, cfg, form):
    """What the driver prints for a case: {"mean_bits", "selected", "assignments", "overlap", "members"}."""
    index_of = {}
    for i, d in enumerate(docs):
        index_of.setdefault(d["hash"], i)
    means, selected = [], []
    for c in clusters:
        members = [index_of.get(h, len(docs) + 7) for h in c["members"]]
        c["centroid"] = mean_embedding(docs, members)
        means.append(bits(c["centroid"]).tolist())
        selected.append(select_diverse(docs, members, c["centroid"], cfg["count"]))
    n = boundary_spill(docs, cfg, clusters, memberships, form)
    return {"mean_bits": means, "selected": selected, "assignments": n, "overlap": [m["overlap"] for m in memberships],
            "members": [c["members"] for c in clusters]}


def parse_driver(text):
    out = {"probe": None, "mean_bits": [], "selected": [], "assignments": None, "overlap": [], "members": []}
    for line in text.splitlines():
        tag, _, rest = line.partition(" ")
        vals = rest.split()
        if tag == "PROBE": out["probe"] = rest
        elif tag == "MEAN": out["mean_bits"].append([int(v) for v in vals])
        elif tag == "SEL": out["selected"].append(vals)
        elif tag == "ASSIGN": out["assignments"] = int(rest)
        elif tag == "OVL": out["overlap"].append(vals)
        elif tag == "MEM": out["members"].append(vals)
    return out
