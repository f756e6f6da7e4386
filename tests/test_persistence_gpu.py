"""computePersistenceH0 on the GPU (yams_quality_persistence_h0_device / _host, topology_quality_v1, the shell over the real
plugin) against the restatements of tests/_persistence_oracle.py and the golden file made from the reference's own translation
unit.  Every comparison is on bits, of EVERY output: all m * m distances (symmetry and the +0.0 diagonal included), the
percentile and its index, the m - 1 merge weights, the value — the value alone hides a wrong chain form.  Every device output is
followed by guard bytes that the wrapper checks.

Where both forms are served on one input, the oracle's two forms differ in at least one distance (asserted), so a form mix-up
cannot pass.  Two kinds of input cannot satisfy that and are exempt by arithmetic, not by choice: m == 1 has no distance, and
at dim == 1 the chain is the single step 0.0 + d * d, whose fused and unfused roundings are the same round(d * d)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _persistence_oracle as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "persistence_h0.json")
TILE_EDGES = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 193, 256, 257]      # (2, 3 | 4, 5 | ... 256 | 257: another round of the tree)
TREE_EDGES = [1023, 1024, 1025, 2049]
_CACHE = {}


def forms_differing_points(m, dim):
    """Mixed-exponent points whose two oracle forms differ in at least one distance (the first seed that does), with both
    oracle results.  Computed once per shape and left unchanged."""
    key = (m, dim)
    if key not in _CACHE:
        for seed in range(400):
            x = po.mixed_points(7000 + 1000 * dim + 13 * m + seed, m, dim)
            want = [po.persistence_cpp(x, f) for f in (po.SEPARATE, po.FUSED)]
            differ = bool((po.bits64(want[0]["distances"]) != po.bits64(want[1]["distances"])).any())
            if differ or m < 2 or dim == 1:
                break
        assert differ == (m >= 2 and dim > 1), (m, dim, "no seed whose forms differ")
        _CACHE[key] = (x, want)
    return _CACHE[key]


def check(acc, x, want, form, **kw):
    got = acc.persistence_h0(x, form=form, want_distances=True, want_weights=True, **kw)
    m = want["n_points"]
    assert got["distances"].shape == (m, m) and (po.bits64(got["distances"]) == po.bits64(want["distances"])).all(), "distances"
    assert (po.bits64(np.diagonal(got["distances"])) == 0).all() and (po.bits64(got["distances"]) == po.bits64(got["distances"].T)).all()
    assert po.same(got, want), {k: (got[k], want[k]) for k in ("norm", "norm_index", "value", "n_merges", "n_edges", "n_points")}
    return got


@pytest.mark.parametrize("dim", [1, 3, 7, 8, 9, 33, 768])
def test_every_output_at_the_tiles_edges(acc, dim):
    for m in TILE_EDGES:
        x, want = forms_differing_points(m, dim)
        for form in (po.SEPARATE, po.FUSED):
            check(acc, x, want[form], form)


@pytest.mark.parametrize("m", TREE_EDGES)
def test_every_output_where_the_trees_rounds_and_the_selects_grid_change(acc, m):
    x, want = forms_differing_points(m, 3)
    for form in (po.SEPARATE, po.FUSED):
        check(acc, x, want[form], form)


@pytest.mark.parametrize("dim", [8, 9, 768])
def test_float_aligned_bases_and_the_host_entry(acc, dim):
    for m in (65, 129):
        x, want = forms_differing_points(m, dim)
        for form in (po.SEPARATE, po.FUSED):
            check(acc, x, want[form], form, misalign=4)      # the scalar-load path at a dimension the vector path would take
            check(acc, x, want[form], form, host_entry=True)


def test_the_python_restatement_agrees_where_it_is_quick_enough(acc):
    x, want = forms_differing_points(65, 3)
    for form in (po.SEPARATE, po.FUSED):
        assert po.same(po.persistence_py(x, form), want[form])


def test_ties_plateaus_and_zero_distances(acc):
    cases = [po.lattice_points(1, 200, 2), po.lattice_points(2, 300, 3, side=3), po.GOLDEN_CASES["lattice_plateau_m30"](),
             po.duplicated_points(4, 150, 50, 5), po.GOLDEN_CASES["duplicates_norm_zero_m41"](), po.duplicated_points(6, 1500, 20, 3),
             np.repeat(po.mixed_points(7, 1, 9), 130, 0), po.cluster_points(8, 5, 60, 9)]
    assert po.plateau_is_strictly_inside(cases[2])
    for x in cases:
        for form in (po.SEPARATE, po.FUSED):
            want = po.persistence_cpp(x, form)
            got = check(acc, x, want, form)
            assert (po.bits64(got["weights"]) == po.bits64(po.prim_weights(want["distances"]))).all()
    zero = acc.persistence_h0(cases[4])
    assert zero["norm"] == 0.0 and zero["value"] == 0.0 and zero["n_merges"] == 0
    assert acc.persistence_h0(cases[6])["value"] == 0.0


def test_one_and_two_points(acc):
    x = po.mixed_points(3, 2, 5)
    for host in (False, True):
        one = acc.persistence_h0(x[:1], want_distances=True, want_weights=True, host_entry=host)
        assert (one["value"], one["norm"], one["n_edges"], one["n_points"], one["n_merges"]) == (0.0, 0.0, 0, 1, 0)
        assert po.bits64(one["distances"]).tolist() == [[0]] and one["weights"].size == 0
        none = acc.persistence_h0(x[:0], want_weights=True, host_entry=host)
        assert (none["value"], none["n_edges"], none["n_points"]) == (0.0, 0, 0)
        two = check(acc, x, po.persistence_cpp(x, po.SEPARATE), po.SEPARATE, host_entry=host)
        assert two["value"] == 0.0 and two["n_edges"] == 1 and two["norm"] > 0 and two["weights"][0] == two["norm"] == two["distances"][0, 1]


def test_select_reorders_repeats_and_drops_rows(acc):
    x, _ = forms_differing_points(129, 33)
    rng = np.random.default_rng(5)
    for sel in (rng.permutation(129)[:100], rng.integers(0, 129, 200), np.array([128, 0, 128, 5, 5, 64]), np.array([7]), np.array([], np.int64)):
        sel = sel.astype(np.uint32)
        for form in (po.SEPARATE, po.FUSED):
            want = po.persistence_cpp(x[sel.astype(np.int64)], form)
            for host in (False, True):
                got = acc.persistence_h0(x, select=sel, form=form, want_distances=True, want_weights=True, host_entry=host)
                assert po.same(got, want), (len(sel), form, host)


def test_centroids_go_from_the_centroid_entry_to_the_statistic_on_the_device(acc):
    """yams_cluster_centroids_device -> the clusters with at least two members as `select` -> persistence, no copy to the host
    in between (the counts come back to choose the rows, as TopologyManager's loop does)."""
    import _artifacts_oracle as ao
    from yams_amd import _lib
    sizes = [5, 1, 0, 9, 2, 1, 30, 4, 0, 12, 3, 2]
    x, off, mem = ao.clustered_case(77, sizes, 48, specials=False)
    c, dim = len(sizes), 48
    d_x, d_off, d_mem = acc.to_device(x), acc.to_device(off), acc.to_device(mem)
    d_cent, d_cnt = acc.alloc(c * dim * 4), acc.alloc(c * 4)
    acc._check(acc.L.yams_cluster_centroids_device(acc.ctx, d_x.ptr, len(x), dim, d_off.ptr, d_mem.ptr, c, d_cent.ptr, d_cnt.ptr))
    counts = d_cnt.download(np.uint32, c)
    sel = np.flatnonzero(counts >= 2).astype(np.uint32)
    assert sel.tolist() == [i for i, s in enumerate(sizes) if s >= 2]
    d_sel, d_dist, d_w = acc.to_device(sel), acc.alloc(len(sel) ** 2 * 8), acc.alloc(len(sel) * 8)
    cents = ao.centroids(x, off, mem)[0][sel.astype(np.int64)]
    for form in (po.SEPARATE, po.FUSED):
        res = _lib.PersistenceH0()
        acc._check(acc.L.yams_quality_persistence_h0_device(acc.ctx, d_cent.ptr, c, dim, d_sel.ptr, len(sel), form, C.byref(res),
                                                            d_dist.ptr, d_w.ptr, None))
        want = po.persistence_cpp(cents, form)
        got = {k: getattr(res, k) for k, _ in _lib.PersistenceH0._fields_}
        got["distances"] = d_dist.download(np.float64, len(sel) ** 2).reshape(len(sel), len(sel))
        got["weights"] = d_w.download(np.float64, len(sel) - 1)
        assert po.same(got, want) and got["value"] > 0
    for b in (d_x, d_off, d_mem, d_cent, d_cnt, d_sel, d_dist, d_w):
        b.free()


def refused(call):
    from yams_amd._lib import AccelError
    with pytest.raises(AccelError) as e:
        call()
    return e.value.status


def test_refusals_write_nothing(acc):
    """The wrapper fills every output with guard words and checks, after a refusal, that all of them are still there."""
    import torch
    from yams_amd import _lib
    inv, unsup = _lib.YAMS_ERR_INVALID_ARG, _lib.YAMS_ERR_UNSUPPORTED
    x, want = forms_differing_points(65, 7)
    kw = dict(want_distances=True, want_weights=True)
    for host in (False, True):
        assert refused(lambda: acc.persistence_h0(np.zeros((3, 0), np.float32), host_entry=host, **kw)) == inv                    # dim == 0
        assert refused(lambda: acc.persistence_h0(x, form=2, host_entry=host, **kw)) == inv                                        # unknown form
        assert refused(lambda: acc.persistence_h0(x, select=np.array([0, 65, 1], np.uint32), host_entry=host, **kw)) == inv        # entry >= n
        assert refused(lambda: acc.persistence_h0(x, select=np.array([65], np.uint32), host_entry=host, **kw)) == inv              # also at m == 1
        for bad in (np.nan, np.inf, -np.inf):
            y = x.copy()
            y[64, 6] = bad
            assert refused(lambda: acc.persistence_h0(y, host_entry=host, **kw)) == inv
            assert refused(lambda: acc.persistence_h0(y, select=np.array([3, 64], np.uint32), host_entry=host, **kw)) == inv
            sel = np.arange(64, dtype=np.uint32)                                                                                   # the row is not selected: served
            assert po.same(acc.persistence_h0(y, select=sel, host_entry=host, **kw), po.persistence_cpp(x[:64], po.SEPARATE))
        assert refused(lambda: acc.persistence_h0(np.zeros((2, 4097), np.float32), host_entry=host, **kw)) == unsup                # dim > YAMS_CLUSTER_MAX_DIM
    # the limit: decided before anything is allocated (the matrix would be 2 GiB and a bit)
    many = np.zeros((_lib.QUALITY_MAX_POINTS + 1, 1), np.float32)
    acc.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    for host in (False, True):
        assert refused(lambda: acc.persistence_h0(many, host_entry=host)) == unsup
        assert refused(lambda: acc.persistence_h0(x, select=np.zeros(_lib.QUALITY_MAX_POINTS + 1, np.uint32), host_entry=host)) == unsup
    assert free_before - torch.cuda.mem_get_info()[0] < 64 << 20
    L, ctx = acc.L, acc.ctx
    res = _lib.PersistenceH0()
    d = acc.to_device(x)
    assert L.yams_quality_persistence_h0_device(ctx, d.ptr, 65, 7, None, 0, 0, None, None, None, None) == inv                      # null out
    assert L.yams_quality_persistence_h0_device(ctx, None, 65, 7, None, 0, 0, C.byref(res), None, None, None) == inv               # null rows
    assert L.yams_quality_persistence_h0_device(None, d.ptr, 65, 7, None, 0, 0, C.byref(res), None, None, None) == inv             # null context
    assert L.yams_quality_persistence_h0_device(ctx, d.ptr, 1 << 31, 7, d.ptr, 2, 0, C.byref(res), None, None, None) == unsup      # n >= 2^31
    assert L.yams_quality_persistence_h0_host(ctx, x.ctypes.data, 1 << 31, 7, x.ctypes.data, 2, 0, C.byref(res), None, None, None) == unsup
    assert L.yams_quality_persistence_h0_device(ctx, None, 0, 7, None, 0, 0, C.byref(res), None, None, None) == 0 and res.value == 0.0
    d.free()
    # the context still serves after the refusals
    check(acc, x, want[po.FUSED], po.FUSED)


# ---- the golden file: what the reference's own function returned ---------------------------------------------------------------
def golden():
    return json.load(open(GOLDEN))["cases"]


@pytest.mark.parametrize("host", [False, True])
def test_the_entries_equal_the_golden_file(acc, host):
    for case in golden():
        x = po.GOLDEN_CASES[case["name"]]()
        assert po.digest(x) == case["sha256"]
        for form in ("separate", "fused"):
            got = acc.persistence_h0(x, form=po.FORMS[form], want_distances=True, want_weights=True, host_entry=host)
            assert po.hex64(got["value"]) == case[form]["returned"], (case["name"], form)
            assert po.golden_record(got) == case[form]["restatement"], (case["name"], form)


@pytest.fixture(scope="module")
def vtable():
    from yams_amd import _lib
    L = _lib.load()
    assert L.yams_plugin_init(b'{"device":0}', None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"topology_quality_v1", 1, C.byref(p)) == 0
    yield C.cast(p, C.POINTER(_lib.TopologyQualityV1)).contents
    L.yams_plugin_shutdown()


def test_the_plugin_interface_equals_the_golden_file(vtable):
    from yams_amd import _lib
    assert vtable.abi_version == 1
    for case in golden():
        x = po.GOLDEN_CASES[case["name"]]()
        m = len(x)
        for form in ("separate", "fused"):
            res, dp, wp = _lib.PersistenceH0(), _lib.f64p(), _lib.f64p()
            assert vtable.persistence_h0(None, x.ctypes.data, m, x.shape[1], None, 0, po.FORMS[form], C.byref(res), C.byref(dp), C.byref(wp)) == 0
            got = {k: getattr(res, k) for k, _ in _lib.PersistenceH0._fields_}
            got["distances"] = np.ctypeslib.as_array(dp, (m, m)).copy()
            got["weights"] = np.ctypeslib.as_array(wp, (m - 1,)).copy()
            vtable.free_persistence_h0(None, dp, wp)
            assert po.hex64(got["value"]) == case[form]["returned"] and po.golden_record(got) == case[form]["restatement"], (case["name"], form)
    # a refusal hands nothing out; the arrays are optional
    x = po.GOLDEN_CASES["clusters_4x6_d9"]()
    res, dp, wp = _lib.PersistenceH0(), _lib.f64p(), _lib.f64p()
    sel = np.array([0, 99], np.uint32)
    assert vtable.persistence_h0(None, x.ctypes.data, len(x), 9, sel.ctypes.data, 2, 0, C.byref(res), C.byref(dp), C.byref(wp)) == _lib.YAMS_ERR_INVALID_ARG
    assert not dp and not wp
    assert vtable.persistence_h0(None, x.ctypes.data, len(x), 9, None, 0, 0, C.byref(res), None, None) == 0
    assert po.hex64(res.value) == po.hex64(po.persistence_cpp(x, po.SEPARATE)["value"])


@pytest.mark.parametrize("form", ["separate", "fused"])
def test_shell_through_the_real_plugin_equals_the_golden_file(form):
    """include/yams_accel/topological_quality.hpp over the real topology_quality_v1 against what the reference's own function
    returned; the shell's probe, asked about the device, reports the form it was created with."""
    from _persistence_build import build_shell_test
    from yams_amd import _lib
    exe = build_shell_test()
    cases = golden()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, case in enumerate(cases):
            paths.append(os.path.join(tmp, "case_%03d.bin" % i))
            po.write_case(paths[-1], po.GOLDEN_CASES[case["name"]]())
        r = subprocess.run([exe, *(["--fused"] if form == "fused" else []), "--plugin", _lib.LIB_PATH, *paths], capture_output=True, text=True,
                           timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.split("\n")
    assert lines[0] == "probe " + form
    values = [l.split()[1:] for l in lines[1:] if l.startswith("value")]
    assert values == [[c[form]["returned"]] * 2 for c in cases]


def test_stress_harness():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_persistence.py"), "--cases", "60"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "60 cases, 0 failures OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
