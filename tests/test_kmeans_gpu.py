"""The device k-means on the GPU against the restatement of tests/_kmeans_oracle.py, bit for bit: membership, centroid bits,
effective k and iterations run, for every golden case and for larger seeded cases; the induced partition equals the one the
reference's own engine produced (tests/golden/kmeans.json); yams_cluster_assign_device against the oracle's nearest centroid
(skipped centroids, all-NaN distances, the fp64 distance bits); the host twin and the plugin path return the same arrays;
non-finite rows are refused.  Nothing is compared within a tolerance (a NaN equals a NaN: _kmeans_oracle.same_f32)."""
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
