"""The plugin door's own contract, in one place and at the smallest shapes that reach each branch: the seven doors that hand
out malloc'd result arrays (order of judgements, out pointers nulled first, optional outs, the matching free), the two handle
families (dedup sets, route indexes: unknown / destroyed ids, independence, ids across a shutdown) and the entries that only
lease a work context and forward.  Every value that comes through a vtable equals the flat entry's on the same input, bit for
bit."""
import ctypes as C
import json

import numpy as np
import pytest

from yams_amd import _lib

pytestmark = pytest.mark.gpu
OK, INVALID, NOT_FOUND, UNSUPPORTED = _lib.YAMS_OK, _lib.YAMS_ERR_INVALID_ARG, _lib.YAMS_ERR_NOT_FOUND, _lib.YAMS_ERR_UNSUPPORTED
f32p, u8p, u32p, u64p, f64p, vp = _lib.f32p, _lib.u8p, _lib.u32p, _lib.u64p, _lib.f64p, C.c_void_p
SENTINEL = 0xDEAD0      # an address no door may keep, free or write through: a refusal leaves it or nulls it, per the contract
TABLES = {"topology_cluster_v1": _lib.TopologyClusterV1, "semantic_graph_v1": _lib.SemanticGraphV1,
          "topology_smooth_v1": _lib.TopologySmoothV1, "topology_artifacts_v1": _lib.TopologyArtifactsV1,
          "topology_route_v1": _lib.TopologyRouteV1, "topology_quality_v1": _lib.TopologyQualityV1,
          "topology_features_v1": _lib.TopologyFeaturesV1, "late_interaction_rerank_v1": _lib.LateInteractionRerankV1,
          "embedding_pool_v1": _lib.EmbeddingPoolV1, "content_hash_v1": _lib.ContentHashV1,
          "content_checksum_v1": _lib.ContentChecksumV1, "vector_scan_v1": _lib.VectorScanV1}


class Door:
    def __init__(self, L):
        self.L = L
        for name, cls in TABLES.items():
            p = C.c_void_p()
            assert L.yams_plugin_get_interface(name.encode(), 1, C.byref(p)) == 0
            setattr(self, name[:-3], C.cast(p, C.POINTER(cls)).contents)


@pytest.fixture(scope="module")
def door():
    L = _lib.load()
    L.yams_plugin_shutdown()                  # (a test that failed half-way leaves the plugin initialised)
    assert L.yams_plugin_init(b'{"device":0}', None) == 0
    yield Door(L)
    L.yams_plugin_shutdown()


def sent(tp):
    return C.cast(C.c_void_p(SENTINEL), tp)


def addr(p):
    return C.cast(p, C.c_void_p).value


def ptr(a, tp):
    return a.ctypes.data_as(tp)


def take(p, dtype, shape):
    return np.ctypeslib.as_array(p, (int(np.prod(shape)),)).view(dtype).reshape(shape).copy()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rows_of(seed, n, dim):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


# ---- topology_cluster_v1.kmeans ---------------------------------------------------------------------------------------------
def test_kmeans_door(door, acc):
    vt, x = door.topology_cluster, rows_of(1, 6, 4)

    def call(n, dim, mem, cent, k=2):
        ke, it = C.c_uint32(7), C.c_uint32(7)
        st = vt.kmeans(None, ptr(x, f32p), n, dim, k, 0, mem, cent, C.byref(ke), C.byref(it))
        return st, ke.value, it.value
    cent = sent(f32p)
    assert call(6, 4, None, C.byref(cent))[0] == INVALID and addr(cent) == SENTINEL      # the mandatory out is judged first
    for n, dim, want in ((0, 4, OK), (0, 0, OK), (6, 0, INVALID), (1, 4, INVALID), (6, 4097, UNSUPPORTED)):      # n == 0 before dim
        mem, cent = sent(u32p), sent(f32p)
        assert call(n, dim, C.byref(mem), C.byref(cent)) == (want, 0, 0), (n, dim)
        assert not mem and not cent, (n, dim)
    w_mem, w_cent, w_k, w_it = acc.cluster_kmeans(x, 2, 0, host_entry=True)
    for want_cent in (True, False):
        mem, cent = sent(u32p), sent(f32p)
        assert call(6, 4, C.byref(mem), C.byref(cent) if want_cent else None) == (OK, w_k, w_it)
        assert same(take(mem, np.uint32, (6,)), w_mem)
        assert addr(cent) == SENTINEL if not want_cent else same(take(cent, np.float32, (w_k, 4)), w_cent)
        vt.free_clusters(None, mem, cent if want_cent else None)
    vt.free_clusters(None, None, None)


# ---- topology_cluster_v1.assign ---------------------------------------------------------------------------------------------
def test_assign_door(door, acc):
    vt, x, c = door.topology_cluster, rows_of(2, 5, 4), rows_of(3, 3, 4)

    def call(n, dim, nc, asg, dist):
        return vt.assign(None, ptr(x, f32p), n, dim, ptr(c, f32p), nc, None, asg, dist)
    dist = sent(f64p)
    assert call(5, 4, 3, None, C.byref(dist)) == INVALID and addr(dist) == SENTINEL
    for n, dim, nc, want in ((0, 4, 3, OK), (0, 0, 3, OK), (5, 0, 3, INVALID), (5, 4, 65537, UNSUPPORTED), (5, 4097, 3, UNSUPPORTED)):
        asg, dist = sent(u32p), sent(f64p)
        assert call(n, dim, nc, C.byref(asg), C.byref(dist)) == want, (n, dim, nc)
        assert not asg and not dist, (n, dim, nc)
    w_asg, w_dist = acc.cluster_assign(x, c)
    for want_dist in (True, False):
        asg, dist = sent(u32p), sent(f64p)
        assert call(5, 4, 3, C.byref(asg), C.byref(dist) if want_dist else None) == OK
        assert same(take(asg, np.uint32, (5,)), w_asg)
        assert addr(dist) == SENTINEL if not want_dist else same(take(dist, np.float64, (5,)), w_dist)
        vt.free_assignment(None, asg, dist if want_dist else None)
    vt.free_assignment(None, None, None)


# ---- semantic_graph_v1.neighbors --------------------------------------------------------------------------------------------
def test_neighbors_door(door, acc):
    vt, x = door.semantic_graph, rows_of(4, 6, 4)

    def call(n, dim, k, outs, inv, diag=None, flags=0):
        return vt.neighbors(None, ptr(x, f32p), n, dim, None, None, 0, k, flags, 0.0, *outs, inv, diag)

    def fresh():
        return sent(u32p), sent(f32p), sent(u32p), sent(f32p)
    r, s, c, iv = fresh()
    assert call(6, 4, 3, (C.byref(r), None, C.byref(c)), C.byref(iv)) == INVALID and addr(r) == addr(iv) == SENTINEL
    # an empty result still goes to the flat entry, which judges the flags; dim == 0 is the flat entry's verdict too
    for n, dim, k, flags, want in ((6, 4, 0, 0, OK), (1, 4, 3, 0, OK), (6, 4, 0, 1 << 31, INVALID), (6, 0, 3, 0, INVALID), (6, 4, 65, 0, UNSUPPORTED)):
        r, s, c, iv = fresh()
        diag = _lib.GraphDiag(9, 9, 9, 9)
        assert call(n, dim, k, (C.byref(r), C.byref(s), C.byref(c)), C.byref(iv), C.byref(diag), flags) == want, (n, dim, k, flags)
        assert not r and not s and not c and not iv, (n, dim, k, flags)
        assert diag.pairs_scored == 0 and diag.stripes == 0      # zeroed before any refusal
    w_r, w_s, w_c, w_iv, w_diag = acc.semantic_neighbors(x, 3, host_entry=True)
    for want_inv in (True, False):
        r, s, c, iv = fresh()
        diag = _lib.GraphDiag()
        assert call(6, 4, 3, (C.byref(r), C.byref(s), C.byref(c)), C.byref(iv) if want_inv else None, C.byref(diag)) == OK
        assert same(take(r, np.uint32, (6, 3)), w_r) and same(take(s, np.float32, (6, 3)), w_s) and same(take(c, np.uint32, (6,)), w_c)
        assert diag.as_dict() == w_diag
        assert addr(iv) == SENTINEL if not want_inv else same(take(iv, np.float32, (6,)), w_iv)
        vt.free_neighbors(None, r, s, c, iv if want_inv else None)
    vt.free_neighbors(None, None, None, None, None)


# ---- topology_artifacts_v1 --------------------------------------------------------------------------------------------------
OFF = np.array([0, 3, 8], np.uint64)
MEM = np.array([5, 1, 7, 0, 2, 3, 4, 6], np.uint32)


def test_centroids_door(door, acc):
    vt, x = door.topology_artifacts, rows_of(5, 8, 4)

    def call(dim, nc, cent, cnt):
        return vt.centroids(None, ptr(x, f32p), 8, dim, ptr(OFF, u64p), ptr(MEM, u32p), nc, cent, cnt)
    cent = sent(f32p)
    assert call(4, 2, C.byref(cent), None) == INVALID and addr(cent) == SENTINEL
    # the limits before dim == 0, dim == 0 before the empty case
    for dim, nc, want in ((4, 0, OK), (0, 0, INVALID), (0, 2, INVALID), (0, 65537, UNSUPPORTED), (4, 65537, UNSUPPORTED), (4097, 2, UNSUPPORTED)):
        cent, cnt = sent(f32p), sent(u32p)
        assert call(dim, nc, C.byref(cent), C.byref(cnt)) == want, (dim, nc)
        assert not cent and not cnt, (dim, nc)
    cent, cnt = sent(f32p), sent(u32p)
    assert call(4, 2, C.byref(cent), C.byref(cnt)) == OK
    w_cent, w_cnt = acc.cluster_centroids(x, OFF, MEM, host_entry=True)
    assert same(take(cent, np.float32, (2, 4)), w_cent) and same(take(cnt, np.uint32, (2,)), w_cnt)
    vt.free_centroids(None, cent, cnt)
    vt.free_centroids(None, None, None)


def test_representatives_door(door, acc):
    vt, x = door.topology_artifacts, rows_of(6, 8, 4)
    cen = acc.cluster_centroids(x, OFF, MEM, host_entry=True)[0]

    def call(dim, nc, extra, sel, cnt):
        return vt.representatives(None, ptr(x, f32p), 8, dim, ptr(OFF, u64p), ptr(MEM, u32p), ptr(cen, f32p), None, nc, extra, sel, cnt)
    cnt = sent(u32p)
    assert call(4, 2, 2, None, C.byref(cnt)) == INVALID and addr(cnt) == SENTINEL
    for dim, nc, extra, want in ((4, 0, 2, OK), (0, 2, 2, INVALID), (0, 2, 65, UNSUPPORTED), (4, 2, 65, UNSUPPORTED), (4, 65537, 2, UNSUPPORTED)):
        sel, cnt = sent(u32p), sent(u32p)
        assert call(dim, nc, extra, C.byref(sel), C.byref(cnt)) == want, (dim, nc, extra)
        assert not sel and not cnt, (dim, nc, extra)
    for extra in (2, 0):      # n_extra == 0: no selection array, the counts alone
        sel, cnt = sent(u32p), sent(u32p)
        assert call(4, 2, extra, C.byref(sel), C.byref(cnt)) == OK
        w_sel, w_cnt = acc.cluster_representatives(x, OFF, MEM, cen, extra, host_entry=True)
        assert same(take(cnt, np.uint32, (2,)), w_cnt)
        assert not sel if extra == 0 else same(take(sel, np.uint32, (2, extra)), w_sel)
        vt.free_representatives(None, sel, cnt)
    vt.free_representatives(None, None, None)


def test_residuals_door(door, acc):
    vt, x, cen = door.topology_artifacts, rows_of(7, 5, 4), rows_of(8, 3, 4)
    pri = np.array([0, 2, 1, 0xFFFFFFFF, 1], np.uint32)
    lists = np.array([0, 2, 2, 3, 3, 4], np.uint64), np.array([1, 2, 0, 2], np.uint32)
    empty = np.zeros(6, np.uint64), np.zeros(1, np.uint32)

    def call(n, dim, nc, primary, cand, outs):
        return vt.residuals(None, ptr(x, f32p), n, dim, ptr(cen, f32p), nc, None if primary is None else ptr(primary, u32p),
                            None if cand is None else ptr(cand[0], u64p), None if cand is None else ptr(cand[1], u32p), 1, *outs)

    def fresh():
        return sent(f64p), sent(f64p), sent(f64p)
    pn, cn, rd = fresh()
    assert call(5, 4, 3, None, None, (C.byref(pn), None, C.byref(rd))) == INVALID and addr(pn) == SENTINEL
    assert call(5, 4, 3, pri, None, (None, C.byref(cn), C.byref(rd))) == INVALID and addr(cn) == SENTINEL
    assert call(5, 4, 3, pri, None, (C.byref(pn), C.byref(cn), None)) == INVALID and addr(cn) == SENTINEL
    falling = np.array([0, 2, 1, 3, 3, 4], np.uint64), lists[1]
    from_one = np.array([1, 2, 2, 3, 3, 4], np.uint64), lists[1]
    for n, dim, nc, cand, want in ((0, 4, 3, None, OK), (5, 0, 3, None, INVALID), (0, 0, 3, None, INVALID), (5, 0, 65537, None, UNSUPPORTED),
                                   (5, 4, 65537, None, UNSUPPORTED), (5, 4, 3, falling, INVALID), (5, 4, 3, from_one, INVALID)):
        pn, cn, rd = fresh()
        assert call(n, dim, nc, pri, cand, (C.byref(pn), C.byref(cn), C.byref(rd))) == want, (n, dim, nc)
        assert not pn and not cn and not rd, (n, dim, nc)
    for cand, pairs in ((None, 15), (lists, 4)):
        for primary in (pri, None):
            for absent in (False, True):      # without primary, its two outs may be there (and come back null) or not
                if primary is not None and absent:
                    continue
                pn, cn, rd = fresh()
                outs = (None, C.byref(cn), None) if absent else (C.byref(pn), C.byref(cn), C.byref(rd))
                assert call(5, 4, 3, primary, cand, outs) == OK
                w_pn, w_cn, w_rd = acc.cluster_residuals(x, cen, primary, *(cand or (None, None)), form=1, host_entry=True)
                assert same(take(cn, np.float64, (pairs,)), w_cn)
                if primary is not None:
                    assert same(take(pn, np.float64, (5,)), w_pn) and same(take(rd, np.float64, (pairs,)), w_rd)
                    vt.free_residuals(None, pn, cn, rd)
                else:
                    assert absent or (not pn and not rd)
                    vt.free_residuals(None, None, cn, None)
    pn, cn, rd = fresh()      # no listed pair at all: the arrays are there all the same
    assert call(5, 4, 3, pri, empty, (C.byref(pn), C.byref(cn), C.byref(rd))) == OK and pn and cn and rd
    vt.free_residuals(None, pn, cn, rd)
    vt.free_residuals(None, None, None, None)


# ---- topology_quality_v1.persistence_h0 -------------------------------------------------------------------------------------
def h0_fields(res):
    return {k: getattr(res, k) for k, _ in _lib.PersistenceH0._fields_}


def test_persistence_door(door, acc):
    vt, x = door.topology_quality, rows_of(9, 5, 4)
    sel = np.array([3, 0, 4], np.uint32)

    def call(n, dim, select, n_select, out, dist, w):
        return vt.persistence_h0(None, ptr(x, vp), n, dim, None if select is None else ptr(select, vp), n_select, 0, out, dist, w)
    dist, w = sent(f64p), sent(f64p)
    assert call(5, 4, None, 0, None, C.byref(dist), C.byref(w)) == INVALID and addr(dist) == addr(w) == SENTINEL
    # a refusal writes nothing at all: not the result, not the two optional outs
    for n, dim, select, n_select, want in ((5, 0, None, 0, INVALID), (5, 4, sel, 16385, UNSUPPORTED), (5, 4097, None, 0, UNSUPPORTED),
                                           (5, 4, np.array([5], np.uint32), 1, INVALID)):
        res, dist, w = _lib.PersistenceH0(), sent(f64p), sent(f64p)
        C.memset(C.byref(res), 0x5A, C.sizeof(res))
        assert call(n, dim, select, n_select, C.byref(res), C.byref(dist), C.byref(w)) == want, (n, dim, n_select)
        assert addr(dist) == addr(w) == SENTINEL and bytes(res) == b"\x5a" * C.sizeof(res), (n, dim, n_select)
    for select, m in ((None, 5), (sel, 3), (sel[:1], 1), (None, 0)):      # m == 1: no merge weights; m == 0: no array at all
        n = 0 if m == 0 else 5
        want = acc.persistence_h0(x[:n], select, host_entry=True, want_distances=True, want_weights=True)
        for want_dist in (True, False):
            for want_w in (True, False):
                res, dist, w = _lib.PersistenceH0(), sent(f64p), sent(f64p)
                assert call(n, 4, select, m if select is not None else 0, C.byref(res), C.byref(dist) if want_dist else None,
                            C.byref(w) if want_w else None) == OK
                got = h0_fields(res)
                assert all(np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes() for k in got), (m, got, want)
                if not want_dist:
                    assert addr(dist) == SENTINEL
                elif m == 0:
                    assert not dist
                else:
                    assert same(take(dist, np.float64, (m, m)), want["distances"])
                if not want_w:
                    assert addr(w) == SENTINEL
                elif m < 2:
                    assert not w
                else:
                    assert same(take(w, np.float64, (m - 1,)), want["weights"])
                vt.free_persistence_h0(None, dist if want_dist else None, w if want_w else None)
    vt.free_persistence_h0(None, None, None)


# ---- the two handle families ------------------------------------------------------------------------------------------------
def hexes(rows):
    return b"".join(r.tobytes().hex().encode() + b"\0" for r in rows)


class Dedup:
    """content_hash_v1.dedup_* of one plugin: every entry takes an id."""
    def __init__(self, door):
        self.vt = door.content_hash

    def create(self):
        ident = C.c_uint64(0)
        assert self.vt.dedup_create(None, 0, C.byref(ident)) == OK
        return ident.value

    def insert(self, ident, digests):
        out = np.full(len(digests), 0xAA, np.uint8)
        return self.vt.dedup_insert(None, ident, hexes(digests), len(digests), ptr(out, u8p)), out.tolist()

    def contains(self, ident, digests):
        out = np.full(len(digests), 0xAA, np.uint8)
        return self.vt.dedup_contains(None, ident, hexes(digests), len(digests), ptr(out, u8p)), out.tolist()

    def size(self, ident):
        v = C.c_uint64(77)
        return self.vt.dedup_size(None, ident, C.byref(v)), v.value

    def destroy(self, ident):
        return self.vt.dedup_destroy(None, ident)

    def gone(self, ident, digests):
        """every entry answers NOT_FOUND and writes nothing (an empty call included: the id is judged first)"""
        untouched = [0xAA] * len(digests)
        return (self.insert(ident, digests) == (NOT_FOUND, untouched) and self.contains(ident, digests) == (NOT_FOUND, untouched) and
                self.insert(ident, digests[:0])[0] == NOT_FOUND and self.size(ident) == (NOT_FOUND, 77) and self.destroy(ident) == NOT_FOUND)


VECTORS = rows_of(10, 4, 4)      # 2 clusters x (centroid, one representative), dim 4
ROUTE_OFF, ROUTE_HAS, ROUTE_POS = np.array([0, 2, 4], np.uint32), np.ones(2, np.uint8), np.array([0xFFFF, 0, 0xFFFF, 0], np.uint16)
QUERY = rows_of(11, 1, 4)


class Route:
    """topology_route_v1 of one plugin."""
    def __init__(self, door):
        self.vt = door.topology_route

    def create(self, vectors):
        ident, norms = C.c_uint64(0), np.zeros(4, np.float32)
        assert self.vt.index_create(None, ptr(vectors, vp), 4, 4, ptr(ROUTE_OFF, vp), ptr(ROUTE_HAS, vp), ptr(ROUTE_POS, vp), 2, C.byref(ident),
                                    ptr(norms, vp)) == OK
        return ident.value, norms

    def info(self, ident):
        inf = _lib.RouteIndexInfo()
        C.memset(C.byref(inf), 0x5A, C.sizeof(inf))
        return self.vt.index_info(None, ident, C.byref(inf)), bytes(inf)

    def dense(self, ident):
        dense, obs, ev = np.full(2, 7.0, np.float32), np.full(2, 7, np.uint8), np.full(1, 7, np.uint32)
        st = self.vt.dense(None, ident, ptr(QUERY, vp), 1, 0, None, ptr(dense, vp), ptr(obs, vp), ptr(ev, vp), None)
        return st, dense, obs, ev

    def destroy(self, ident):
        return self.vt.index_destroy(None, ident)

    def gone(self, ident):
        st, dense, obs, ev = self.dense(ident)
        return (st == NOT_FOUND and (dense == 7.0).all() and (obs == 7).all() and ev[0] == 7 and
                self.info(ident) == (NOT_FOUND, b"\x5a" * C.sizeof(_lib.RouteIndexInfo)) and self.destroy(ident) == NOT_FOUND)


def test_dedup_handles(door):
    d = Dedup(door)
    digests = np.random.default_rng(12).integers(0, 256, (4, 32), dtype=np.uint8)
    assert d.gone(0, digests) and d.gone(1 << 40, digests)      # ids never handed out
    a, b = d.create(), d.create()
    assert a != b and a >= 1 and b >= 1
    assert d.insert(a, digests) == (OK, [1, 1, 1, 1]) and d.insert(a, digests[:2]) == (OK, [0, 0]) and d.size(a) == (OK, 4)
    assert d.contains(b, digests) == (OK, [0, 0, 0, 0]) and d.size(b) == (OK, 0)      # two live sets share nothing
    assert d.insert(b, digests[1:3]) == (OK, [1, 1]) and d.size(b) == (OK, 2) and d.size(a) == (OK, 4)
    assert d.destroy(a) == OK
    assert d.gone(a, digests)                                    # ... and the second destroy is NOT_FOUND
    assert d.contains(b, digests) == (OK, [0, 1, 1, 0])         # the other set lives on
    assert d.destroy(b) == OK and d.gone(b, digests)


def test_route_handles(door, acc):
    r = Route(door)
    assert r.gone(0) and r.gone(1 << 40)
    other = np.ascontiguousarray(VECTORS[::-1])
    (a, norms_a), (b, norms_b) = r.create(VECTORS), r.create(other)
    assert a != b and a >= 1 and b >= 1
    for ident, vectors, norms in ((a, VECTORS, norms_a), (b, other, norms_b)):      # each equals the flat entries on its own table
        flat = acc.route_index(vectors, ROUTE_OFF, ROUTE_HAS, ROUTE_POS, host_entry=True)
        w_dense, w_obs, w_ev, _ = acc.route_dense(flat, QUERY, host_entry=True)
        st, dense, obs, ev = r.dense(ident)
        assert st == OK and same(dense, w_dense[0]) and obs.astype(bool).tolist() == w_obs[0].tolist() and ev[0] == w_ev[0]
        assert same(norms, flat.norms)
        st, raw = r.info(ident)
        inf = _lib.RouteIndexInfo.from_buffer_copy(raw)
        assert st == OK and (inf.n_vectors, inf.n_clusters, inf.dim, inf.bytes) == tuple(flat.info()[k] for k in ("n_vectors", "n_clusters", "dim", "bytes"))
        flat.close()
    assert not same(r.dense(a)[1], r.dense(b)[1])               # two live indexes share nothing
    assert r.destroy(a) == OK and r.gone(a)
    assert r.dense(b)[0] == OK
    assert r.destroy(b) == OK and r.gone(b)


def test_handles_do_not_outlive_a_shutdown(door):
    """Everything is destroyed at yams_plugin_shutdown; after a fresh init the old ids name nothing, and the ids handed out
    next continue the sequence: an old id is never given to a new object."""
    d, r = Dedup(door), Route(door)
    digests = np.random.default_rng(13).integers(0, 256, (4, 32), dtype=np.uint8)
    old_set, (old_index, _) = d.create(), r.create(VECTORS)
    assert d.insert(old_set, digests)[0] == OK
    door.L.yams_plugin_shutdown()
    assert d.size(old_set)[0] == UNSUPPORTED and r.dense(old_index)[0] == UNSUPPORTED      # not initialised: every entry refuses
    assert door.L.yams_plugin_init(b'{"device":0}', None) == 0
    assert d.gone(old_set, digests) and r.gone(old_index)
    new_set, (new_index, _) = d.create(), r.create(VECTORS)
    assert new_set > old_set and new_index > old_index
    assert d.contains(new_set, digests) == (OK, [0, 0, 0, 0])
    assert d.destroy(new_set) == OK and r.destroy(new_index) == OK


# ---- the entries that lease a work context and forward ----------------------------------------------------------------------
def test_forwarded_entries_equal_the_flat_entries(door, acc):
    x, q = rows_of(14, 5, 4), rows_of(15, 2, 4)
    off = np.array([0, 2, 5], np.uint64)
    rec = np.array([4, 0, 1, 3, 2], np.uint32)
    out, cnt = np.zeros((2, 4), np.float32), np.zeros(2, np.uint32)
    assert door.topology_features.aggregate(None, ptr(x, vp), 5, 4, ptr(off, vp), ptr(rec, vp), 2, ptr(out, vp), ptr(cnt, vp)) == OK
    assert all(same(g, w) for g, w in zip((out, cnt), acc.features_aggregate(x, off, rec, host_entry=True)))
    mean, var = np.zeros(4, np.float64), np.zeros(4, np.float64)
    assert door.topology_features.variance(None, ptr(x, vp), 5, 4, None, 5, 0, ptr(mean, vp), ptr(var, vp)) == OK
    assert all(same(g, w) for g, w in zip((mean, var), acc.features_variance(x, host_entry=True)))
    out, dims = np.zeros((5, 4), np.float32), np.zeros(5, np.uint32)
    assert door.topology_features.compose(None, ptr(x, vp), 5, 4, None, None, 0, None, None, 0, None, 0, 0.0, 0.0, ptr(out, vp), 4, ptr(dims, vp)) == OK
    assert all(same(g, w) for g, w in zip((out, dims), acc.features_compose(x, host_entry=True)))
    sc = np.zeros(2, np.float32)
    assert door.late_interaction_rerank.maxsim(None, ptr(q, vp), 2, 4, ptr(x, vp), ptr(off, vp), 2, 0, ptr(sc, vp), None, None, None) == OK
    assert same(sc, acc.rerank_maxsim(q, x, off, host_entry=True)[0])
    out = np.zeros((2, 4), np.float32)
    assert door.late_interaction_rerank.maxpool(None, ptr(x, vp), 4, ptr(off, vp), 2, ptr(out, vp)) == OK
    assert same(out, acc.rerank_maxpool(x, off, host_entry=True))
    hidden, out = rows_of(16, 6, 4).reshape(2, 3, 4), np.zeros((2, 4), np.float32)
    assert door.embedding_pool.pool(None, ptr(hidden, vp), 2, 3, 4, None, 0, _lib.EMBED_POOL_MEAN, _lib.EMBED_NORMALIZE, ptr(out, vp), None) == OK
    assert same(out, acc.embed_pool(hidden, host_entry=True)[0])
    out = np.zeros((5, 4), np.float32)
    assert door.embedding_pool.normalize(None, ptr(x, vp), 5, 4, ptr(out, vp)) == OK
    assert same(out, acc.embed_normalize(x, host_entry=True))
    msgs = [np.frombuffer(b"abc", np.uint8), np.frombuffer(b"hello, world", np.uint8)]
    ptrs, lens, crc = (vp * 2)(*[m.ctypes.data for m in msgs]), (C.c_size_t * 2)(3, 12), np.zeros(2, np.uint32)
    assert door.content_checksum.crc32_many(None, ptrs, lens, 2, ptr(crc, u32p)) == OK
    assert same(crc, acc.crc32_many(msgs))
    text = vp()
    assert door.vector_scan.get_runtime_info_json(None, C.byref(text)) == OK
    info = json.loads(C.string_at(text).decode())
    door.vector_scan.free_string(None, text)
    # the description of the device is the same from any context; what a context adds about its own past (its last host
    # ingest, its sweep's deal) and the free memory of the moment are not the door's to equal
    flat = acc.device_info()
    device = ("backend", "arch", "name", "compute_units", "clock_khz", "memory_clock_khz", "memory_bus_bits", "hbm_bytes",
              "lds_per_block", "wavefront", "l2_bytes", "version")
    assert "hbm_free_bytes" in info and [info[k] for k in device] == [flat[k] for k in device]
    edges, cols, weights = np.arange(6, dtype=np.uint64), np.array([1, 0, 3, 2, 0], np.uint32), np.ones(5, np.float32)
    out, diag = np.zeros((5, 4), np.float32), _lib.SgcDiag()
    C.memset(C.byref(diag), 0x5A, C.sizeof(diag))
    assert door.topology_smooth.smooth(None, ptr(x, f32p), 5, 4, ptr(edges, u64p), ptr(cols, u32p), ptr(weights, f32p), 1, ptr(out, f32p), C.byref(diag)) == OK
    w_out, w_diag = acc.sgc_smooth(x, edges, cols, weights, 1, host_entry=True)
    assert same(out, w_out) and diag.as_dict() == w_diag and diag.reserved == 0
    C.memset(C.byref(diag), 0x5A, C.sizeof(diag))      # a refusal still zeroes the diagnostics
    assert door.topology_smooth.smooth(None, ptr(x, f32p), 5, 0, ptr(edges, u64p), ptr(cols, u32p), ptr(weights, f32p), 1, ptr(out, f32p), C.byref(diag)) == INVALID
    assert bytes(diag) == b"\0" * C.sizeof(diag)
