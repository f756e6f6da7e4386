"""The cluster artifacts on the GPU (yams_cluster_centroids / _representatives / _residuals, _device and _host, and
topology_artifacts_v1) against the restatement of tests/_artifacts_oracle.py.  Every comparison is on bits; the only tolerance
is that a NaN matches any NaN.  Every device output is followed by guard bytes that the wrapper checks."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import _artifacts_oracle as ao

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 63, 64, 65]


def statuses():
    from yams_amd import _lib
    return _lib.YAMS_ERR_INVALID_ARG, _lib.YAMS_ERR_UNSUPPORTED


def refused(call):
    from yams_amd._lib import AccelError
    with pytest.raises(AccelError) as e:
        call()
    return e.value.status


# ---- centroids ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 3, 4, 37, 64, 1024, 4096])
def test_centroids_sizes_and_dims(acc, dim):
    x, off, mem = ao.clustered_case(100 + dim, SIZES, dim)
    want = ao.centroids(x, off, mem)
    for host in (False, True):
        cent, cnt = acc.cluster_centroids(x, off, mem, host_entry=host)
        assert ao.same_bits(cent, want[0]) and cnt.tolist() == want[1].tolist() == SIZES
    cent, _ = acc.cluster_centroids(x, off, mem, misalign=4)      # float-aligned bases
    assert ao.same_bits(cent, want[0])


@pytest.mark.parametrize("dim", [37, 64])
def test_centroids_one_giant_cluster_beside_singletons(acc, dim):
    x, off, mem = ao.clustered_case(7, [4000] + [1] * 1000, dim)
    want = ao.centroids(x, off, mem)
    cent, cnt = acc.cluster_centroids(x, off, mem)
    assert ao.same_bits(cent, want[0]) and cnt[0] == 4000 and (cnt[1:] == 1).all()
    assert ao.same_bits(cent[1:], x[mem[4000:].astype(np.int64)])      # s / 1.0f: the row itself


def test_centroids_keep_the_order_of_the_member_list(acc):
    x, off, desc = ao.clustered_case(11, [300, 65], 37, order="descending")
    asc = np.concatenate([np.sort(desc[:300]), np.sort(desc[300:])]).astype(np.uint32)
    want_d, want_a = ao.centroids(x, off, desc)[0], ao.centroids(x, off, asc)[0]
    assert (ao.bits(want_d) != ao.bits(want_a)).any()      # on the oracle the order matters
    assert ao.same_bits(acc.cluster_centroids(x, off, desc)[0], want_d)
    assert ao.same_bits(acc.cluster_centroids(x, off, asc)[0], want_a)


def test_centroids_signed_zeros_denormals_and_overflow(acc):
    big = np.float32(ao.F32_MAX / 4)
    x = np.zeros((12, 5), np.float32)
    x[0] = -0.0; x[1] = -0.0                                  # 0.0f + -0.0f = +0.0f: the sum starts at +0.0f
    x[2] = ao.f32(np.array([1, 2, 3, 0x007fffff, 0x80000001], np.uint32)); x[3] = x[2]; x[4] = x[2]      # denormals, / 3.0f
    x[5:10] = big; x[7, 1] = -big                             # five rows of FLT_MAX / 4: the sum overflows to inf
    x[10] = [np.inf, -np.inf, np.nan, 1.0, -1.0]; x[11] = [-np.inf, -np.inf, 1.0, 2.0, -0.0]
    off = np.array([0, 2, 5, 10, 12], np.uint64)
    mem = np.arange(12, dtype=np.uint32)
    want = ao.centroids(x, off, mem)[0]
    assert np.isinf(want[2, 0]) and ao.bits(want[0])[0] == 0 and np.isnan(want[3, 0]) and np.isnan(want[3, 2])
    for host in (False, True):
        assert ao.same_bits(acc.cluster_centroids(x, off, mem, host_entry=host)[0], want)


# ---- representatives ----------------------------------------------------------------------------------------------------------
def rep_case(seed, sizes, dim):
    x, off, cand = ao.clustered_case(seed, sizes, dim)
    cents = ao.centroids(x, off, cand)[0]
    return x, off, cand, cents


@pytest.mark.parametrize("n_extra", [1, 2, 4, 64])
@pytest.mark.parametrize("dim", [3, 37, 64])
def test_representatives_sizes_and_counts(acc, dim, n_extra):
    x, off, cand, cents = rep_case(200 + dim, SIZES, dim)
    want = ao.representatives(x, off, cand, cents, n_extra)
    assert want[1].tolist() == [min(s, n_extra) for s in SIZES]      # n_extra > candidates: everything is selected
    for host in (False, True):
        sel, cnt = acc.cluster_representatives(x, off, cand, cents, n_extra, host_entry=host)
        assert sel.tolist() == want[0].tolist() and cnt.tolist() == want[1].tolist()
    sel, _ = acc.cluster_representatives(x, off, cand, cents, n_extra, misalign=4)
    assert sel.tolist() == want[0].tolist()


@pytest.mark.parametrize("dim,n_extra", [(1024, 3), (4096, 2), (1, 4)])
def test_representatives_wide_and_narrow_rows(acc, dim, n_extra):
    x, off, cand, cents = rep_case(300 + dim, [5, 70, 0, 3], dim)
    want = ao.representatives(x, off, cand, cents, n_extra)
    sel, cnt = acc.cluster_representatives(x, off, cand, cents, n_extra)
    assert sel.tolist() == want[0].tolist() and cnt.tolist() == want[1].tolist()


def test_representatives_one_giant_cluster_beside_singletons(acc):
    x, off, cand, cents = rep_case(9, [4000] + [1] * 1000, 16)
    want = ao.representatives(x, off, cand, cents, 4)
    sel, cnt = acc.cluster_representatives(x, off, cand, cents, 4)
    assert sel.tolist() == want[0].tolist() and cnt.tolist() == want[1].tolist()


def test_representatives_ties_zero_rows_and_special_centroids(acc):
    rng = np.random.default_rng(5)
    x = ao.random_rows(rng, 40, 6)
    x[10:20] = x[10]                      # ten exact duplicates: every tie goes to the first in list order
    x[25] = 0.0                           # a zero row: distance 2.0, the farthest
    off = np.array([0, 10, 20, 30, 35, 40], np.uint64)
    cand = np.arange(40, dtype=np.uint32)
    cents = ao.centroids(x, off, cand)[0]
    cents[3] = 0.0                        # a zero centroid: every distance is 2.0, the first candidate wins the first pass
    cents[4] = np.inf                     # an inf centroid: NaN distances, minDist stays, the first candidate wins the first pass
    want = ao.representatives(x, off, cand, cents, 4)
    assert want[0][1].tolist() == [0, 1, 2, 3] and want[0][2][0] == 5 and want[0][3][0] == 0 and want[0][4][0] == 0
    for host in (False, True):
        sel, cnt = acc.cluster_representatives(x, off, cand, cents, 4, host_entry=host)
        assert sel.tolist() == want[0].tolist() and cnt.tolist() == want[1].tolist()
    empty = np.array([0, 1, 0, 1, 0], np.uint8)
    want = ao.representatives(x, off, cand, cents, 4, empty)
    sel, cnt = acc.cluster_representatives(x, off, cand, cents, 4, centroid_empty=empty)
    assert sel.tolist() == want[0].tolist() and cnt.tolist() == [4, 0, 4, 0, 4] and (sel[1] == ao.NONE).all()


def test_representatives_candidates_in_any_order_and_repeated_rows(acc):
    # the candidate lists need not partition the rows: a row may serve two clusters, a list may be a subset
    x = ao.random_rows(np.random.default_rng(6), 50, 9)
    off = np.array([0, 20, 45], np.uint64)
    cand = np.concatenate([np.arange(19, -1, -1), np.arange(10, 35)]).astype(np.uint32)
    cents = ao.centroids(x, off, cand)[0]
    want = ao.representatives(x, off, cand, cents, 5)
    sel, cnt = acc.cluster_representatives(x, off, cand, cents, 5)
    assert sel.tolist() == want[0].tolist() and cnt.tolist() == want[1].tolist()


# ---- residuals ----------------------------------------------------------------------------------------------------------------
def check_residuals(acc, x, cents, pri, off, cand, wants=None, **kw):
    wants = wants or {form: ao.residuals(x, cents, pri, off, cand, form) for form in (ao.SEPARATE, ao.FUSED)}
    # the case tells the forms apart: on the oracle alone, some chain differs between them
    assert any(w0 is not None and (ao.bits(w0) != ao.bits(w1)).any() for w0, w1 in zip(wants[ao.SEPARATE], wants[ao.FUSED]))
    for form, want in wants.items():
        got = acc.cluster_residuals(x, cents, pri, off, cand, form=form, **kw)
        for name, g, w in zip(("primary_norm_sq", "cand_norm_sq", "residual_dot"), got, want):
            assert (g is None) == (w is None), name
            if w is None:
                continue
            if name == "residual_dot" and pri is not None:      # undefined for a document without a primary
                doc = np.repeat(np.arange(len(x)), len(cents)) if off is None else np.repeat(np.arange(len(x)), np.diff(off.astype(np.int64)))
                keep = np.asarray(pri)[doc] != ao.NONE
                g, w = g[keep], w[keep]
            assert ao.same_bits(g, w), (name, form, np.argwhere(ao.bits(g) != ao.bits(w))[:4].tolist())
    return wants


@pytest.mark.parametrize("c,n,dim", [(2, 130, 19), (3, 129, 8), (33, 70, 37), (40, 66, 37), (70, 66, 24), (3, 5, 1030)])
def test_residuals_dense(acc, c, n, dim):
    x, cents, pri, _, _ = ao.residual_case(400 + c, n, c, dim)
    wants = check_residuals(acc, x, cents, pri, None, None)
    check_residuals(acc, x, cents, pri, None, None, wants=wants, misalign=4)


@pytest.mark.parametrize("c,n,dim", [(2, 40, 19), (3, 40, 8), (33, 40, 37), (40, 30, 37)])
def test_residuals_lists(acc, c, n, dim):
    x, cents, pri, off, cand = ao.residual_case(500 + c, n, c, dim, list_len=32)
    assert int(off[-1]) > 256 and len(set(np.diff(off.astype(np.int64)).tolist())) > 1
    wants = check_residuals(acc, x, cents, pri, off, cand)
    check_residuals(acc, x, cents, pri, off, cand, wants=wants, misalign=4)


@pytest.mark.parametrize("c", [3, 40])
def test_residuals_without_a_primary(acc, c):
    x, cents, _, off, cand = ao.residual_case(600 + c, 50, c, 21, list_len=32)
    check_residuals(acc, x, cents, None, None, None)      # dense: only the candidate norms
    check_residuals(acc, x, cents, None, off, cand)       # the radius pass: lists, no primary


def test_residuals_non_finite_inputs_are_served(acc):
    x, cents, pri, off, cand = ao.residual_case(700, 70, 5, 11, list_len=32)
    x[3, 2] = np.nan; x[9, 0] = np.inf; x[12] = ao.F32_MAX; cents[1, 4] = -np.inf; cents[2, 1] = np.nan; cents[4] = -ao.F32_MAX
    wants = check_residuals(acc, x, cents, pri, None, None)
    assert np.isnan(wants[ao.SEPARATE][1]).any() and np.isinf(wants[ao.SEPARATE][1]).any()
    check_residuals(acc, x, cents, pri, off, cand)


def test_residuals_host_entry_in_slices(acc):
    x, cents, pri, off, cand = ao.residual_case(800, 70, 33, 12, list_len=32)
    check_residuals(acc, x, cents, pri, None, None, host_entry=True)
    check_residuals(acc, x, cents, pri, off, cand, host_entry=True)
    check_residuals(acc, x, cents, None, off, cand, host_entry=True)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal(acc):
    inv, unsup = statuses()
    x, off, mem = ao.clustered_case(1, [3, 4], 5, specials=False)
    cents = ao.centroids(x, off, mem)[0]
    bad_off = np.array([0, 5, 4], np.uint64); late_off = np.array([1, 3, 7], np.uint64)
    bad_mem = mem.copy(); bad_mem[2] = 7
    for host in (False, True):
        for o, m in ((bad_off, mem), (late_off, mem), (off, bad_mem)):
            assert refused(lambda: acc.cluster_centroids(x, o, m, host_entry=host)) == inv
            assert refused(lambda: acc.cluster_representatives(x, o, m, cents, 2, host_entry=host)) == inv
        assert refused(lambda: acc.cluster_representatives(x, off, mem, cents, 65, host_entry=host)) == unsup
        nf = x.copy(); nf[6, 1] = np.inf
        assert refused(lambda: acc.cluster_representatives(nf, off, mem, cents, 2, host_entry=host)) == inv
        wide = np.zeros((2, 4097), np.float32)
        assert refused(lambda: acc.cluster_centroids(wide, [0, 2], [0, 1], host_entry=host)) == unsup
        assert refused(lambda: acc.cluster_residuals(wide, wide, host_entry=host)) == unsup
        pri = np.array([0, 1, 2, 0, 1, ao.NONE, 1], np.uint32)      # 2 is not a cluster
        assert refused(lambda: acc.cluster_residuals(x, cents, pri, host_entry=host)) == inv
        pri[2] = 0
        assert refused(lambda: acc.cluster_residuals(x, cents, pri, form=2, host_entry=host)) == inv
        lo = np.array([0, 1, 2, 3, 4, 5, 6, 7], np.uint64)
        assert refused(lambda: acc.cluster_residuals(x, cents, pri, lo, np.array([0, 1, 0, 1, 2, 0, 1], np.uint32), host_entry=host)) == inv
        down = lo.copy(); down[3] = 9
        assert refused(lambda: acc.cluster_residuals(x, cents, pri, down, np.zeros(7, np.uint32), host_entry=host)) == inv
    L, ctx = acc.L, acc.ctx
    assert L.yams_cluster_centroids_device(ctx, None, 1 << 31, 4, None, None, 1, None, None) == unsup
    assert L.yams_cluster_centroids_device(ctx, None, 0, 0, None, None, 1, None, None) == inv
    assert L.yams_cluster_centroids_device(ctx, None, 0, 4, None, None, 65537, None, None) == unsup
    assert L.yams_cluster_centroids_device(ctx, None, 0, 4, None, None, 1, None, None) == inv      # null offsets / outputs
    assert L.yams_cluster_centroids_device(ctx, None, 0, 4, None, None, 0, None, None) == 0        # no clusters: nothing to do
    assert L.yams_cluster_residuals_device(ctx, None, 0, 4, None, 0, None, None, None, 0, None, None, None) == 0
    assert L.yams_cluster_residuals_device(None, None, 0, 4, None, 0, None, None, None, 0, None, None, None) == inv
    # the context still serves after the refusals
    assert ao.same_bits(acc.cluster_centroids(x, off, mem)[0], cents)


# ---- whole entry points -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vtable():
    from yams_amd import _lib
    L = _lib.load()
    assert L.yams_plugin_init(b'{"device":0}', None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"topology_artifacts_v1", 1, C.byref(p)) == 0
    yield C.cast(p, C.POINTER(_lib.TopologyArtifactsV1)).contents
    L.yams_plugin_shutdown()


def through_vtable(vt, x, off, mem, n_extra, pri, form):
    """centroids -> representatives -> dense residuals through topology_artifacts_v1; everything the plugin allocated is freed."""
    from yams_amd import _lib
    n, dim = x.shape
    c = len(off) - 1
    fp, u32, u64 = _lib.f32p, _lib.u32p, _lib.u64p
    cent_p, cnt_p = fp(), u32()
    assert vt.centroids(None, x.ctypes.data_as(fp), n, dim, off.ctypes.data_as(u64), mem.ctypes.data_as(u32), c, C.byref(cent_p), C.byref(cnt_p)) == 0
    cent = np.ctypeslib.as_array(cent_p, (c, dim)).copy()
    cnt = np.ctypeslib.as_array(cnt_p, (c,)).copy()
    vt.free_centroids(None, cent_p, cnt_p)
    sel_p, scnt_p = u32(), u32()
    assert vt.representatives(None, x.ctypes.data_as(fp), n, dim, off.ctypes.data_as(u64), mem.ctypes.data_as(u32), cent.ctypes.data_as(fp), None,
                              c, n_extra, C.byref(sel_p), C.byref(scnt_p)) == 0
    sel = np.ctypeslib.as_array(sel_p, (c, n_extra)).copy()
    scnt = np.ctypeslib.as_array(scnt_p, (c,)).copy()
    vt.free_representatives(None, sel_p, scnt_p)
    pn_p, cn_p, rd_p = _lib.f64p(), _lib.f64p(), _lib.f64p()
    assert vt.residuals(None, x.ctypes.data_as(fp), n, dim, cent.ctypes.data_as(fp), c, pri.ctypes.data_as(u32), None, None, form,
                        C.byref(pn_p), C.byref(cn_p), C.byref(rd_p)) == 0
    res = tuple(np.ctypeslib.as_array(p, (m,)).copy() for p, m in ((pn_p, n), (cn_p, n * c), (rd_p, n * c)))
    vt.free_residuals(None, pn_p, cn_p, rd_p)
    return cent, cnt, sel, scnt, res


def vtable_case(seed):
    x, off, mem = ao.clustered_case(seed, [40, 1, 64, 25], 13)
    pri = np.zeros(len(x), np.uint32)
    for k in range(4):
        pri[mem[int(off[k]):int(off[k + 1])].astype(np.int64)] = k
    want_c = ao.centroids(x, off, mem)
    want_s = ao.representatives(x, off, mem, want_c[0], 3)
    want_r = ao.residuals(x, want_c[0], pri, None, None, ao.FUSED)
    return (x, off, mem, pri), (want_c, want_s, want_r)


def vtable_differs(got, want):
    cent, cnt, sel, scnt, res = got
    (wc, wcnt), (ws, wscnt), wr = want
    return [name for name, ok in (("centroids", ao.same_bits(cent, wc) and cnt.tolist() == wcnt.tolist()),
                                  ("representatives", sel.tolist() == ws.tolist() and scnt.tolist() == wscnt.tolist()),
                                  ("residuals", all(ao.same_bits(g, w) for g, w in zip(res, wr)))) if not ok]


def test_vtable_serves_the_three_entries(vtable):
    from yams_amd import _lib
    assert vtable.abi_version == 1
    (x, off, mem, pri), want = vtable_case(31)
    assert vtable_differs(through_vtable(vtable, x, off, mem, 3, pri, ao.FUSED), want) == []
    p1, p2 = _lib.f32p(), _lib.u32p()
    assert vtable.centroids(None, x.ctypes.data_as(_lib.f32p), len(x), 13, np.array([0, 3, 2], np.uint64).ctypes.data_as(_lib.u64p),
                            mem.ctypes.data_as(_lib.u32p), 2, C.byref(p1), C.byref(p2)) == _lib.YAMS_ERR_INVALID_ARG
    assert not p1 and not p2


def test_four_concurrent_callers(vtable):
    cases = [vtable_case(40 + i) for i in range(4)]
    bad = [None] * 4

    def run(i):
        (x, off, mem, pri), want = cases[i]
        try:
            bad[i] = [vtable_differs(through_vtable(vtable, x, off, mem, 3, pri, ao.FUSED), want) for _ in range(3)]
        except Exception as e:      # noqa: BLE001
            bad[i] = repr(e)
    threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert bad == [[[], [], []]] * 4, bad


def test_residuals_host_entry_of_more_than_one_slice(acc):
    """The _host entry serves the documents in slices of 256 MiB of outputs: 70 000 x 256 pairs x 16 bytes is two slices of the
    dense mode, 540 000 x 32 listed pairs two of the list mode.  Narrow rows keep the case quick; SEPARATE, whose restatement
    is vectorised."""
    rng = np.random.default_rng(21)
    n, c, dim = 70000, 256, 2
    cents = ao.random_rows(rng, c, dim)
    x = ao.random_rows(rng, n, dim)
    pri = rng.integers(0, c, n).astype(np.uint32)
    want = ao.residuals(x, cents, pri, None, None, ao.SEPARATE)
    got = acc.cluster_residuals(x, cents, pri, form=ao.SEPARATE, host_entry=True)
    assert n * c * 16 > 256 << 20 and all(ao.same_bits(g, w) for g, w in zip(got, want))
    n, per, c = 540000, 32, 5
    x = ao.random_rows(rng, n, dim)
    pri = rng.integers(0, c, n).astype(np.uint32)
    off = (np.arange(n + 1, dtype=np.uint64) * per)
    off[n // 2:] -= 7                      # one shorter list, so that the slices' local offsets matter
    cand = rng.integers(0, c, int(off[-1])).astype(np.uint32)
    want = ao.residuals(x, cents[:c], pri, off, cand, ao.SEPARATE)
    got = acc.cluster_residuals(x, cents[:c], pri, off, cand, form=ao.SEPARATE, host_entry=True)
    assert int(off[-1]) * 16 > 256 << 20 and all(ao.same_bits(g, w) for g, w in zip(got, want))


def test_stress_harness():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_artifacts.py"), "--cases", "60"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "60 cases, 0 failures OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("form", ["separate", "fused"])
def test_shell_through_the_real_plugin_equals_the_golden_file(form):
    """include/yams_accel/topology_artifacts.hpp over the real topology_artifacts_v1 against what the reference's own functions
    returned (tests/golden/cluster_artifacts.json)."""
    import json
    import subprocess
    import tempfile
    from _artifacts_build import build_shell_test
    from yams_amd import _lib
    exe = build_shell_test()
    golden = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "cluster_artifacts.json")))["cases"]}
    for name in sorted(ao.GOLDEN_CASES):
        docs, clusters, memberships, cfg = ao.GOLDEN_CASES[name]()
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "case.bin")
            ao.write_case(path, docs, clusters, memberships, cfg)
            r = subprocess.run([exe, path, *(["--fused"] if form == "fused" else []), "--plugin", _lib.LIB_PATH], capture_output=True, text=True,
                               timeout=120)
        assert r.returncode == 0, (name, r.stdout[-1000:], r.stderr[-2000:])
        got = ao.parse_driver(r.stdout)
        for key in ("mean_bits", "selected", "assignments", "overlap", "members"):
            assert got[key] == golden[name][form][key], (name, form, key)
