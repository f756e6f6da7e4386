"""The device k-means on the GPU against the restatement of tests/_kmeans_oracle.py, bit for bit: membership, centroid bits,
effective k and iterations run, for every golden case and for larger seeded cases; the induced partition equals the one the
reference's own engine produced (tests/golden/kmeans.json); yams_cluster_assign_device against the oracle's nearest centroid
(skipped centroids, all-NaN distances, the fp64 distance bits); the host twin and the plugin path return the same arrays;
non-finite rows are refused; and the edges: more than 256 block partials with ties between different rows, k_eff above 256, dim
at YAMS_CLUSTER_MAX_DIM, float-aligned device bases, the staged host upload, every pair's distance, signed zeros, workspace reuse,
concurrent plugin callers.  Nothing is compared within a tolerance (a NaN equals a NaN: _kmeans_oracle.same_f32)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _kmeans_oracle as ko
from test_kmeans_cpu import CASES, build_kmeans_test

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE = [n for n in sorted(ko.CASES) if n not in ("ragged_shell", "one_usable_row")]


def device_shell(acc, **kw):
    return lambda rows, k, it: acc.cluster_kmeans(rows, k, it, **kw)


def check(acc, rows, k, it, **kw):
    mem, cent, ke, ran = ko.kmeans(rows, k, it)
    gm, gc, gk, gr = acc.cluster_kmeans(rows, k, it, **kw)
    assert (gk, gr) == (ke, ran)
    assert np.array_equal(gm, mem), int((gm != mem).sum())
    assert ko.same_f32(gc, cent)
    return gm, gc


@pytest.mark.parametrize("name", DENSE)
def test_golden_cases_equal_the_oracle_and_the_reference_partition(acc, name):
    c = CASES[name]
    rows = np.array(ko.case_rows(name), np.float32)
    gm, _ = check(acc, rows, c["k"], c["max_iterations"])
    assert ko.partition(gm) == c["partition"]


@pytest.mark.parametrize("name", ["ragged_shell", "one_usable_row", "duplicates"])
def test_shell_over_the_device_equals_the_reference_partition(acc, name):
    c = CASES[name]
    a = ko.run_shell(ko.case_rows(name), c["k"], c["max_iterations"], core=device_shell(acc))
    assert ko.partition(a) == c["partition"]


@pytest.mark.parametrize("n,dim,k,it,groups", [(3000, 96, 0, 0, 40), (5000, 33, 130, 4, 25), (1500, 384, 0, 3, 12), (20000, 64, 0, 2, 200),
                                               (700, 768, 70, 0, 9), (129, 5, 129, 0, 3)])
def test_larger_seeded_cases_equal_the_oracle(acc, n, dim, k, it, groups):
    rows = ko.clustered_rows(1000 + n, n, dim, groups)
    rows[n // 2] = 0.0
    rows[n // 3] = rows[n // 5]                              # a duplicate pair
    check(acc, rows, k, it)


def test_duplicate_heavy_rows_run_the_repair_path(acc):
    base = ko.uniform_rows(77, 9, 24)
    rows = base[(np.arange(500) * 7) % 9].copy()
    rows[::50] = ko.uniform_rows(78, 10, 24)
    before = ko.REPAIRS[0]
    check(acc, rows, 40, 0)
    assert ko.REPAIRS[0] > before


def test_denormal_and_huge_rows_are_served_as_the_cpu_computes_them(acc):
    for name in ("denormal_rows", "flt_max_quarter", "zero_rows"):
        rows = np.array(ko.case_rows(name), np.float32)
        for k, it in ((0, 0), (5, 1), (len(rows), 2)):
            check(acc, rows, k, it)


def test_host_twin_and_plugin_path_return_the_same_arrays(acc):
    from yams_amd import _lib
    rows = ko.clustered_rows(5, 900, 50, 11)
    mem, cent = check(acc, rows, 0, 0)
    hm, hc = check(acc, rows, 0, 0, host_entry=True)
    assert np.array_equal(hm, mem) and ko.same_f32(hc, cent)
    L = _lib.load()
    assert L.yams_plugin_init(b'{"device":0}', None) == 0
    try:
        p = C.c_void_p()
        assert L.yams_plugin_get_interface(b"topology_cluster_v1", 1, C.byref(p)) == 0
        vt = C.cast(p, C.POINTER(_lib.TopologyClusterV1)).contents
        pm = _lib.u32p(); pc = _lib.f32p(); ke = C.c_uint32(); it = C.c_uint32()
        assert vt.kmeans(None, rows.ctypes.data_as(_lib.f32p), 900, 50, 0, 0, C.byref(pm), C.byref(pc), C.byref(ke), C.byref(it)) == 0
        assert ke.value == cent.shape[0]
        assert np.array_equal(np.ctypeslib.as_array(pm, (900,)), mem)
        assert ko.same_f32(np.ctypeslib.as_array(pc, (ke.value, 50)), cent)
        vt.free_clusters(None, pm, pc)
        empty = np.zeros(ke.value, np.uint8); empty[::3] = 1
        wa, wd = ko.nearest(rows, cent, empty)
        pa = _lib.u32p(); pd = C.POINTER(C.c_double)()
        assert vt.assign(None, rows.ctypes.data_as(_lib.f32p), 900, 50, cent.ctypes.data_as(_lib.f32p), ke.value,
                         empty.ctypes.data_as(_lib.u8p), C.byref(pa), C.byref(pd)) == 0
        assert np.array_equal(np.ctypeslib.as_array(pa, (900,)), wa) and ko.same_f64(np.ctypeslib.as_array(pd, (900,)), wd)
        vt.free_assignment(None, pa, pd)
        bad = rows.copy(); bad[17, 3] = np.nan
        assert vt.kmeans(None, bad.ctypes.data_as(_lib.f32p), 900, 50, 0, 0, C.byref(pm), None, None, None) == _lib.YAMS_ERR_INVALID_ARG
        assert not pm
    finally:
        L.yams_plugin_shutdown()


@pytest.mark.parametrize("n,dim,nc", [(1000, 64, 141), (257, 3, 5), (128, 50, 64), (2000, 384, 65), (77, 1, 2)])
def test_assign_equals_the_oracle(acc, n, dim, nc):
    rng = np.random.default_rng(n + dim)
    rows = ko.clustered_rows(n, n, dim, 7)
    rows[1] = 0.0
    cents = rng.standard_normal((nc, dim)).astype(np.float32)
    cents[nc // 2] = cents[0]                               # a tie: the lower index wins
    if nc > 4:
        cents[3] = 0.0                                       # a zero centroid: distance 2.0
        cents[4, 0] = np.nan                                 # NaN distances never win
    for empty in (None, (rng.random(nc) < 0.4).astype(np.uint8), np.ones(nc, np.uint8)):
        wa, wd = ko.nearest(rows, cents, empty)
        ga, gd = acc.cluster_assign(rows, cents, empty)
        assert np.array_equal(ga, wa) and ko.same_f64(gd, wd)
    ga, _ = acc.cluster_assign(rows, cents, None, with_distance=False)
    assert np.array_equal(ga, ko.nearest(rows, cents)[0])


def test_assign_with_all_nan_distances_and_without_centroids(acc):
    rows = ko.uniform_rows(3, 300, 12)
    cents = np.full((5, 12), np.inf, np.float32); cents[2] = np.nan
    ga, gd = acc.cluster_assign(rows, cents)
    assert (ga == 0).all() and (gd == ko.DBL_MAX).all()
    ga, gd = acc.cluster_assign(rows, np.zeros((0, 12), np.float32))
    assert (ga == 0).all() and (gd == ko.DBL_MAX).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_rows_are_refused(acc, bad):
    from yams_amd import _lib
    rows = ko.uniform_rows(9, 400, 20)
    rows[399, 19] = bad
    with pytest.raises(_lib.AccelError) as e:
        acc.cluster_kmeans(rows, 0, 0)
    assert e.value.status == _lib.YAMS_ERR_INVALID_ARG
    with pytest.raises(_lib.AccelError) as e:
        acc.cluster_kmeans(rows, 0, 0, host_entry=True)
    assert e.value.status == _lib.YAMS_ERR_INVALID_ARG
    with pytest.raises(_lib.AccelError) as e:
        acc.cluster_assign(rows, rows[:4])
    assert e.value.status == _lib.YAMS_ERR_INVALID_ARG


def test_kmeans_adapter_against_the_host_loop():
    """tests/cpp/kmeans_test.cpp: AccelKMeans::run (the usable-row shell over topology_cluster_v1) against a scalar host loop."""
    from yams_amd import build as b
    r = subprocess.run([build_kmeans_test(), b.LIB], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_stress_harness_on_the_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_kmeans.py"), "--cases", "60", "--seed", "1"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mode"] == "device" and res["cases"] == 60


# ---- the edges: strided partials, far ties, k_eff above 256, the dimension limit, unaligned bases, signed zeros, threads -------
FAR_TIES = (70, 300, 700, 65791, 66000, 131000, 139999)        # 65791: the last row of partial 256, a thread's second stride


def far_tie_rows():
    """Row 0 = e0, fillers e0 + 1e-3 N(0, 1), and seven rows 2.5 e_a (a = 1..7): at distance exactly 1.0 from every centroid
    picked before them, so minDist ties between DIFFERENT rows in different waves, blocks and partials more than 256 apart."""
    n, dim = 140000, 8
    rows = (np.random.default_rng(140000).standard_normal((n, dim)) * 1e-3).astype(np.float32)
    rows[:, 0] += np.float32(1.0)
    rows[0] = 0.0; rows[0, 0] = 1.0
    for a, u in enumerate(FAR_TIES, start=1):
        rows[u] = 0.0; rows[u, a] = 2.5
    return rows


def test_far_ties_across_strided_partials_pick_the_lowest_row(acc):
    rows = far_tie_rows()
    mem, cent, ke, ran = ko.kmeans(rows, 8, 2)
    assert ke == 8 and {u: int(mem[u]) for u in FAR_TIES} == {u: a for a, u in enumerate(FAR_TIES, start=1)}   # the oracle reaches the ties
    gm, gc, gk, gr = acc.cluster_kmeans(rows, 8, 2)
    assert (gk, gr) == (ke, ran) and np.array_equal(gm, mem) and ko.same_f32(gc, cent), {u: int(gm[u]) for u in FAR_TIES}


def test_duplicates_at_scale_repair_above_the_partial_stride(acc):
    base = ko.uniform_rows(81, 37, 8)
    rows = base[(np.arange(70001) * 11) % 37].copy()
    before = ko.REPAIRS[0]
    check(acc, rows, 45, 2)
    assert ko.REPAIRS[0] > before                              # more clusters than distinct rows: the repair path ran


@pytest.mark.parametrize("n,dim,k,it", [(66000, 4, 7, 2), (131073, 3, 5, 1)])
def test_more_than_256_partials_equal_the_oracle(acc, n, dim, k, it):
    check(acc, ko.clustered_rows(1000 + n, n, dim, 9), k, it)


@pytest.mark.parametrize("n,dim,k,it", [(1200, 8, 257, 2), (1500, 12, 513, 2), (2100, 6, 1025, 1), (900, 5, 900, 1)])
def test_effective_k_above_256_equals_the_oracle(acc, n, dim, k, it):
    """kmeans_scan_kernel with more than one cluster per thread; group / centroid grids above 256 workgroups."""
    rows = ko.clustered_rows(n + k, n, dim, 20)
    rows[::13] = rows[1]
    before = ko.REPAIRS[0]
    _, gc = check(acc, rows, k, it)
    assert gc.shape[0] == k
    if k == n:
        assert ko.REPAIRS[0] > before                          # duplicate rows and k == n: clusters come up empty


@pytest.mark.parametrize("dim", [4095, 4096])
def test_dim_at_the_limit_equals_the_oracle(acc, dim):
    """YAMS_CLUSTER_MAX_DIM: one centroid fills the 16 KiB stage of kmeans_pick_kernel / kmeans_centroid_kernel exactly."""
    from yams_amd import _lib
    assert _lib.CLUSTER_MAX_DIM == 4096
    rows = ko.clustered_rows(dim, 300, dim, 4)
    _, cent = check(acc, rows, 6, 2)
    if dim == _lib.CLUSTER_MAX_DIM:
        wa, wd = ko.nearest(rows, cent[:5])
        ga, gd = acc.cluster_assign(rows, cent[:5])
        assert np.array_equal(ga, wa) and ko.same_f64(gd, wd)


SENTINEL = 0xA5


def _host_image(arr, shift, tail=64):
    raw = np.full(shift + arr.nbytes + tail, SENTINEL, np.uint8)
    raw[shift:shift + arr.nbytes] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    return raw


def _shifted(acc, arr, shift, tail=64):
    """arr uploaded `shift` bytes into a sentinel-filled allocation; returns (buffer, device address of the data)."""
    buf = acc.to_device(_host_image(arr, shift, tail))
    return buf, buf.ptr + shift


def _out(acc, nbytes, shift, tail=64):
    buf = acc.to_device(np.full(shift + nbytes + tail, SENTINEL, np.uint8))
    return buf, buf.ptr + shift


def _read(buf, nbytes, shift, dtype):
    """The output range of a buffer made by _out; the bytes before and after it must still hold the sentinel."""
    raw = buf.download(np.uint8, buf.nbytes)
    assert (raw[:shift] == SENTINEL).all() and (raw[shift + nbytes:] == SENTINEL).all(), "wrote outside the output range"
    return raw[shift:shift + nbytes].copy().view(dtype)


@pytest.mark.parametrize("dim", [8, 64])
@pytest.mark.parametrize("row_shift", [4, 8])
def test_kmeans_on_unaligned_device_bases(acc, dim, row_shift):
    """The header promises float alignment only: rows 4 / 8 bytes into an allocation take the scalar assignment kernel although
    dim % 4 == 0; membership and centroids land 4 bytes into theirs."""
    n, k, it = 513, 70, 3
    rows = ko.clustered_rows(dim + row_shift, n, dim, 9)
    rows[7] = rows[400]
    am, ac = check(acc, rows, k, it)                           # the aligned call, held to the oracle
    bufs = []
    try:
        bx, px = _shifted(acc, rows, row_shift); bufs.append(bx)
        bm, pm = _out(acc, n * 4, 4); bufs.append(bm)
        bc, pc = _out(acc, k * dim * 4, 4); bufs.append(bc)
        assert px % 16 != 0
        ke, ran = acc.cluster_kmeans_device(px, n, dim, k, it, pm, pc)
        gm = _read(bm, n * 4, 4, np.uint32); gc = _read(bc, k * dim * 4, 4, np.float32).reshape(k, dim)
        assert bx.download(np.uint8, bx.nbytes).tobytes() == _host_image(rows, row_shift).tobytes()      # the input is left alone
    finally:
        for b in bufs:
            b.free()
    assert ke == k and np.array_equal(gm, am) and ko.same_f32(gc, ac)


@pytest.mark.parametrize("dim", [8, 64])
@pytest.mark.parametrize("row_shift,cent_shift", [(4, 4), (8, 8), (0, 4), (16, 8)])
def test_assign_on_unaligned_device_bases(acc, dim, row_shift, cent_shift):
    """(0, 4): only the centroid base is off (not 8-byte aligned); (16, 8): shifted but aligned enough for the vector kernel."""
    n, nc = 513, 65
    rows = ko.clustered_rows(3 * dim + row_shift, n, dim, 7)
    cents = ko.uniform_rows(dim + cent_shift, nc, dim)
    cents[40] = cents[2]; cents[5] = 0.0
    empty = np.zeros(nc, np.uint8); empty[::6] = 1
    wa, wd = ko.nearest(rows, cents, empty)
    aa, ad = acc.cluster_assign(rows, cents, empty)            # the aligned call
    assert np.array_equal(aa, wa) and ko.same_f64(ad, wd)
    bufs = []
    try:
        bx, px = _shifted(acc, rows, row_shift); bufs.append(bx)
        bc, pc = _shifted(acc, cents, cent_shift); bufs.append(bc)
        be, pe = _shifted(acc, empty, 1); bufs.append(be)
        ba, pa = _out(acc, n * 4, 4); bufs.append(ba)
        bd, pd = _out(acc, n * 8, 8); bufs.append(bd)           # (a double* is 8-byte aligned by its type)
        acc._check(acc.L.yams_cluster_assign_device(acc.ctx, px, n, dim, pc, nc, pe, pa, pd))
        ga = _read(ba, n * 4, 4, np.uint32); gd = _read(bd, n * 8, 8, np.float64)
    finally:
        for b in bufs:
            b.free()
    assert np.array_equal(ga, wa) and ko.same_f64(gd, wd)


def test_host_entry_above_the_staging_threshold(acc):
    rows = ko.clustered_rows(9, 33000, 64, 6)
    assert rows.nbytes == 8448000 > 8 << 20                     # the pinned staging ring and its copy crew
    hm, hc = check(acc, rows, 4, 1, host_entry=True)
    dm, dc, _, _ = acc.cluster_kmeans(rows, 4, 1)
    assert np.array_equal(hm, dm) and ko.same_f32(hc, dc)


def test_every_distance_of_4096_rows_to_32_centroids(acc):
    """One centroid per call, so out_distance holds that centroid's distance to every row: the fp64 sqrt, the fp64 divide and
    the clamp of km_distance, 131072 values bit for bit."""
    rows = ko.uniform_rows(4, 4096, 24)
    cents = [rows[c] for c in range(28)] + [np.zeros(24, np.float32), (np.float32(3.0) * rows[5]).astype(np.float32),
                                            (np.float32(2.0) * rows[14]).astype(np.float32), -rows[7]]
    assert len(cents) == 32
    na = ko.sumsq(rows)
    seen = 0
    for c in cents:
        c = np.ascontiguousarray(c[None, :], np.float32)
        wa, wd = ko.nearest(rows, c, na=na)
        ga, gd = acc.cluster_assign(rows, c)
        assert (ga == 0).all() and ko.same_f64(gd, wd), int((gd.view(np.uint64) != wd.view(np.uint64)).sum())
        seen += gd.size
    assert seen == 131072
    one = lambda u, c: float(ko.nearest(rows[u:u + 1], cents[c][None, :])[1][0])
    assert (ko.nearest(rows, cents[28][None, :])[1] == 2.0).all()                                  # the zero centroid
    assert 0.0 < one(5, 29) <= 2.0 ** -50                       # 3 x row 5 (rounded to fp32): a cosine one step under 1
    cos = ko._dots(rows[14:15], cents[30][None, :])[0, 0] / (np.sqrt(na[14]) * np.sqrt(ko.sumsq(cents[30][None, :])[0]))
    assert cos > 1.0 and one(14, 30) == 0.0                     # 2 x row 14 (exact): the cosine rounds above 1, the clamp cuts it
    assert one(7, 31) == 2.0                                    # the opposite row: -1 exactly


def test_assign_over_many_centroid_tiles(acc):
    n, dim, nc = 130, 3, 4097                                  # 65 tiles of 64 centroids; the last holds one
    rows = ko.uniform_rows(31, n, dim)
    cents = ko.uniform_rows(32, nc, dim)
    rows[:9] = (np.float32(0.5) * cents[3]).astype(np.float32)
    cents[67] = cents[3]; cents[4096] = cents[3]
    rng = np.random.default_rng(4097)
    for skipped, winner in (((), 3), ((3,), 67), ((3, 67), 4096)):
        for empty in (None, (rng.random(nc) < 0.3).astype(np.uint8)):
            if empty is None and skipped:
                empty = np.zeros(nc, np.uint8)
            if empty is not None:
                empty[[3, 67, 4096]] = 0; empty[list(skipped)] = 1
            wa, wd = ko.nearest(rows, cents, empty)
            assert (wa[:9] == winner).all()                     # the oracle reaches the tie across tiles
            ga, gd = acc.cluster_assign(rows, cents, empty)
            assert np.array_equal(ga, wa) and ko.same_f64(gd, wd)


def signed_zero_rows(dim):
    n = 240
    rows = ko.clustered_rows(50 + dim, n, dim, 4, spread=0.05)
    pick = (ko.uniform_rows(52 + dim, n, 1)[:, 0].astype(np.float64) * 0.5 + 0.5) * 4      # clustered_rows' own group of a row
    group = np.minimum(pick.astype(np.int64), 3)
    rows[ko.uniform_rows(60 + dim, n, dim) < -0.8] = -0.0      # scattered
    rows[group == 2, 1] = -0.0                                  # one cluster holds nothing but -0.0 in a dimension
    rows[group == 1, dim - 1] = -0.0                            # ... and one in the last dimension, next to the chunk's zero fill
    rows[3] = -0.0                                              # a row of nothing else
    rows[100:140] = rows[5]                                     # duplicates: with k = 60 the repair path copies rows into centroids
    return rows


@pytest.mark.parametrize("dim", [5, 17])
def test_negative_zeros_keep_their_sign_where_the_cpu_keeps_it(acc, dim):
    assert not ko.same_f32(np.float32([-0.0]), np.float32([0.0]))      # the comparison tells the two zeros apart
    rows = signed_zero_rows(dim)
    assert np.signbit(rows[rows == 0]).all() and (rows == 0).sum() > 100
    _, cent = check(acc, rows, 6, 0)
    assert ((cent == 0) & ~np.signbit(cent)).any()             # a mean of -0.0 alone is +0.0 (the chain starts at +0.0f)
    assert ((cent == 0) & np.signbit(cent)).all(axis=1).any()   # the -0.0 row, repaired into a cluster of its own, stays -0.0
    before = ko.REPAIRS[0]
    _, cent = check(acc, rows, 60, 1)
    assert ko.REPAIRS[0] > before and ((cent == 0) & np.signbit(cent)).any()       # a copied row keeps its -0.0
    empty = np.zeros(60, np.uint8); empty[::4] = 1
    wa, wd = ko.nearest(rows, cent, empty)
    ga, gd = acc.cluster_assign(rows, cent, empty)
    assert np.array_equal(ga, wa) and ko.same_f64(gd, wd)


def test_workspace_reuse_large_small_large_is_deterministic(acc):
    large = ko.clustered_rows(71, 30000, 16, 12)
    small = ko.clustered_rows(72, 50, 3, 2)
    m1, c1 = check(acc, large, 24, 2)
    check(acc, small, 0, 0)
    m3, c3, k3, r3 = acc.cluster_kmeans(large, 24, 2)
    assert m3.tobytes() == m1.tobytes() and c3.tobytes() == c1.tobytes() and (k3, r3) == (c1.shape[0], 2)


def test_concurrent_plugin_callers_each_equal_the_oracle(acc):
    """Four host threads in topology_cluster_v1 at once: every call leases a work context with its own workspaces and pinned
    buffer, so no thread may see another's rows, counts or flags."""
    import threading
    from yams_amd import _lib
    shapes = [(600, 8, 0, 3), (1100, 33, 40, 2), (1700, 64, 0, 2), (2500, 5, 70, 3)]
    inputs = []
    for t, (n, dim, k, it) in enumerate(shapes):
        rows = ko.clustered_rows(200 + t, n, dim, 6 + t)
        rows[n // 2] = rows[1]
        mem, cent, ke, ran = ko.kmeans(rows, k, it)
        empty = np.zeros(ke, np.uint8); empty[t::5] = 1
        inputs.append((rows, k, it, mem, cent, ke, ran, empty) + ko.nearest(rows, cent, empty))
    L = _lib.load()
    assert L.yams_plugin_init(b'{"device":0}', None) == 0
    failures = []
    try:
        p = C.c_void_p()
        assert L.yams_plugin_get_interface(b"topology_cluster_v1", 1, C.byref(p)) == 0
        vt = C.cast(p, C.POINTER(_lib.TopologyClusterV1)).contents
        start = threading.Barrier(len(shapes))

        def worker(t):
            rows, k, it, mem, cent, ke, ran, empty, wa, wd = inputs[t]
            n, dim = rows.shape
            try:
                start.wait(timeout=60)
                for rnd in range(3):
                    pm = _lib.u32p(); pc = _lib.f32p(); gk = C.c_uint32(); gr = C.c_uint32()
                    st = vt.kmeans(None, rows.ctypes.data_as(_lib.f32p), n, dim, k, it, C.byref(pm), C.byref(pc), C.byref(gk), C.byref(gr))
                    if st != 0:
                        failures.append((t, rnd, "kmeans status", st)); return
                    ok = (gk.value, gr.value) == (ke, ran) and np.array_equal(np.ctypeslib.as_array(pm, (n,)), mem) and \
                        ko.same_f32(np.ctypeslib.as_array(pc, (gk.value, dim)), cent)
                    vt.free_clusters(None, pm, pc)
                    if not ok:
                        failures.append((t, rnd, "kmeans differs")); return
                    pa = _lib.u32p(); pd = C.POINTER(C.c_double)()
                    st = vt.assign(None, rows.ctypes.data_as(_lib.f32p), n, dim, cent.ctypes.data_as(_lib.f32p), ke,
                                   empty.ctypes.data_as(_lib.u8p), C.byref(pa), C.byref(pd))
                    if st != 0:
                        failures.append((t, rnd, "assign status", st)); return
                    ok = np.array_equal(np.ctypeslib.as_array(pa, (n,)), wa) and ko.same_f64(np.ctypeslib.as_array(pd, (n,)), wd)
                    vt.free_assignment(None, pa, pd)
                    if not ok:
                        failures.append((t, rnd, "assign differs")); return
            except Exception as e:                              # (a thread's exception must reach the test)
                failures.append((t, repr(e)))

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(len(shapes))]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    finally:
        L.yams_plugin_shutdown()
    assert not failures, failures
