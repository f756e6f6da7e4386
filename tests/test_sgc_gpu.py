"""SGC smoothing on the GPU (yams_graph_sgc_smooth_device / _host, topology_smooth_v1) against the restatement of
tests/_sgc_oracle.py and the reference's own applySGCSmoothing (tests/golden/sgc.json).  Every comparison is on bits; the only
tolerance is that a NaN matches any NaN.  The diagnostics (nnz, max_degree, edges_skipped_zero_scale, hub_rows) are compared
too: hub_rows is what shows that a case took the hub launch."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import _sgc_oracle as sg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "sgc.json")))["cases"]}
SENTINEL = 0xA5


def differs(got, want):
    out, diag = got
    y, wd = want
    bad = [] if sg.same_bits(out, y) else [("out", np.argwhere(~((sg.bits(out) == sg.bits(y)) | (np.isnan(out) & np.isnan(y))))[:4].tolist())]
    return bad + [(k, diag[k], wd[k]) for k in ("nnz", "max_degree", "edges_skipped_zero_scale", "hops", "hub_rows") if diag[k] != wd[k]]


def check(acc, x, off, cols, w, hops, host_entry=False, want=None):
    want = want or sg.smooth(x, off, cols, w, hops, with_diag=True)
    got = acc.sgc_smooth(x, off, cols, w, hops, host_entry=host_entry)
    bad = differs(got, want)
    assert not bad, bad
    return got, want


@pytest.fixture(scope="module")
def vtable():
    from yams_amd import _lib
    L = _lib.load()
    assert L.yams_plugin_init(b'{"device":0}', None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"topology_smooth_v1", 1, C.byref(p)) == 0
    yield C.cast(p, C.POINTER(_lib.TopologySmoothV1)).contents
    L.yams_plugin_shutdown()


def through_vtable(vt, x, off, cols, w, hops, fill=None):
    """One topology_smooth_v1.smooth call; returns (status, out, diag)."""
    from yams_amd import _lib
    x = np.ascontiguousarray(x, np.float32)
    off = np.ascontiguousarray(off, np.uint64); cols = np.ascontiguousarray(cols, np.uint32); w = np.ascontiguousarray(w, np.float32)
    out = np.zeros_like(x) if fill is None else np.full_like(x, fill)
    diag = _lib.SgcDiag()
    st = vt.smooth(None, x.ctypes.data_as(_lib.f32p), x.shape[0], x.shape[1], off.ctypes.data_as(_lib.u64p),
                   cols.ctypes.data_as(_lib.u32p) if cols.size else None, w.ctypes.data_as(_lib.f32p) if w.size else None, hops,
                   out.ctypes.data_as(_lib.f32p), C.byref(diag))
    return st, out, diag.as_dict()


# ---- the golden cases through the three doors -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sg.GOLDEN_CASES))
def test_golden_cases_equal_the_reference_function(acc, vtable, name):
    c = GOLDEN[name]
    docs = sg.GOLDEN_CASES[name][0]()
    off = np.array(c["row_offsets"], np.uint64); cols = np.array(c["cols"], np.uint32); w = sg.f32(np.array(c["weights_bits"], np.uint32))
    x, live = sg.feature_matrix(docs)
    hops = c["hops"]

    def written_back(y):      # what the shell leaves in the documents: the rows of the right size
        return [y[i].copy() if live[i] else d["emb"] for i, d in enumerate(docs)]

    for out in (acc.sgc_smooth(x, off, cols, w, hops)[0], acc.sgc_smooth(x, off, cols, w, hops, host_entry=True)[0],
                through_vtable(vtable, x, off, cols, w, hops)[1]):
        embs = written_back(out)
        assert sg.embeddings_digest(embs) == c["out_sha256"], name                     # the reference's own output
        if "out_bits" in c:
            assert [sg.bits(e).tolist() for e in embs] == c["out_bits"], name


# ---- shapes -----------------------------------------------------------------------------------------------------------------
# every dim class: one float, below a vector, exactly one, odd, a wave of vectors, several workgroups per row, the limit and its
# neighbours; n from 2 to 2000; the three hop counts (both parities of the ping-pong) spread over them
@pytest.mark.parametrize("dim,n,hops", [(1, 2000, 3), (3, 2, 1), (4, 257, 2), (37, 1000, 3), (64, 513, 1), (384, 300, 2), (1024, 130, 3),
                                        (1025, 65, 2), (4095, 33, 1), (4096, 40, 2)])
def test_dims_and_row_counts(acc, dim, n, hops):
    x, off, cols, w = sg.seeded_case(1000 + dim, n, dim, 8)
    (out, diag), (y, _) = check(acc, x, off, cols, w, hops)
    empty = np.nonzero(np.diff(off.astype(np.int64)) == 0)[0]
    if hops == 1 and len(empty):
        assert sg.same_bits(out[empty], x[empty])                                  # no edges: inv^2 == 1, bit-identical
    check(acc, x, off, cols, w, hops, host_entry=True, want=(y, _))


@pytest.mark.parametrize("dim", [8, 37])
@pytest.mark.parametrize("hops", [1, 2, 3, 4])
def test_hop_counts_land_in_out(acc, dim, hops):
    x, off, cols, w = sg.seeded_case(7, 300, dim, 6)
    check(acc, x, off, cols, w, hops)


def test_rows_without_edges_come_back_bit_identical(acc):
    x = sg.random_rows(np.random.default_rng(3), 500, 12)
    off = np.zeros(501, np.uint64)
    (out, diag), _ = check(acc, x, off, np.zeros(0, np.uint32), np.zeros(0, np.float32), 3)
    assert sg.same_bits(out, x) and diag["nnz"] == 0 and diag["max_degree"] == 0


@pytest.mark.parametrize("dim,degree", [(64, 5000), (37, 5000), (4, sg.HUB_DEGREE - 1), (4, sg.HUB_DEGREE), (5, sg.HUB_DEGREE + 1)])
def test_one_hub_row_among_short_rows(acc, dim, degree):
    x, off, cols, w = sg.seeded_case(50 + dim, 600, dim, 8, hub=(311, degree))
    (out, diag), _ = check(acc, x, off, cols, w, 2)
    assert diag["max_degree"] == degree and diag["hub_rows"] == (1 if degree >= sg.HUB_DEGREE else 0)


def test_several_hub_rows(acc):
    rng = np.random.default_rng(9)
    n, dim = 40, 20
    cnt = rng.integers(0, 4, n); cnt[[0, 17, 39]] = [600, 512, 1000]
    off = np.zeros(n + 1, np.uint64); off[1:] = np.cumsum(cnt)
    cols = rng.integers(0, n, int(off[n])).astype(np.uint32); w = rng.random(int(off[n])).astype(np.float32)
    (out, diag), _ = check(acc, sg.random_rows(rng, n, dim), off, cols, w, 3)
    assert diag["hub_rows"] == 3


def test_a_row_whose_edges_all_have_zero_scale(acc):
    x, off, cols, w = sg.seeded_case(77, 64, 6, 5, specials=False)
    r = int(np.argmax(np.diff(off.astype(np.int64))))                              # the longest row of the case
    a, b = int(off[r]), int(off[r + 1])
    assert b - a >= 2
    w[a:b] = 0.0
    x[r] = [-0.0, 1.0, -0.0, -2.0, 0.0, -0.0]
    (out, diag), _ = check(acc, x, off, cols, w, 1)
    assert sg.same_bits(out[r], x[r])                                              # deg 1, every edge skipped: -0.0f survives
    assert not sg.same_bits(sg.smooth(x, off, cols, w, 1, skip_zero_scale=False)[r], x[r])
    assert diag["edges_skipped_zero_scale"] >= b - a


def test_signed_zero_denormal_and_large_elements(acc):
    rng = np.random.default_rng(5)
    n, dim = 120, 9
    off, cols, w = sg.random_lists(rng, n, 6)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[:, 0] = -0.0; x[:, 1] = np.float32(1e-40); x[:, 2] = -np.float32(1.4e-45); x[::2, 3] = sg.FLT_MAX / 4; x[1::2, 3] = -sg.FLT_MAX / 4
    x[:, 4] = np.float32(1.1754944e-38); x[:, 5] *= np.float32(1e-38)
    (out, _), _ = check(acc, x, off, cols, w, 2)
    tiny = np.float32(1.1754944e-38)
    assert ((np.abs(out) > 0) & (np.abs(out) < tiny)).any() and (sg.bits(out) == 0x80000000).any()      # denormals and -0.0f kept


def test_overflow_inside_the_hops_is_served(acc):
    x = np.full((3, 4), sg.FLT_MAX, np.float32); x[2] = -sg.FLT_MAX
    off = np.array([0, 3, 3, 6], np.uint64); cols = np.array([1, 1, 1, 0, 1, 2], np.uint32); w = np.ones(6, np.float32)
    (out, _), _ = check(acc, x, off, cols, w, 1)
    assert np.isposinf(out[0]).all()
    (out2, _), _ = check(acc, x, off, cols, w, 3)                                  # inf - inf further on: a NaN matches any NaN
    assert not np.isfinite(out2[0]).all()


@pytest.mark.parametrize("dim,shift", [(8, 4), (64, 8), (37, 4)])
def test_float_aligned_device_bases(acc, dim, shift):
    """The header promises float alignment only: rows and out 4 / 8 bytes into their allocations take element loads although
    dim % 4 == 0; the bytes around out stay as they were."""
    n = 193
    x, off, cols, w = sg.seeded_case(31, n, dim, 8)
    want = sg.smooth(x, off, cols, w, 2, with_diag=True)
    nb = n * dim * 4
    d_x = acc.alloc(nb + 64); d_x.upload(x.view(np.uint8).reshape(-1), shift)
    d_out = acc.alloc(nb + 64); d_out.upload(np.full(nb + 64, SENTINEL, np.uint8))
    bufs = [acc.to_device(off), acc.to_device(cols), acc.to_device(w)]
    try:
        diag = acc.sgc_smooth_device(d_x.ptr + shift, n, dim, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 2, d_out.ptr + shift)
        raw = d_out.download(np.uint8, nb + 64)
    finally:
        for b in bufs + [d_x, d_out]:
            b.free()
    assert (raw[:shift] == SENTINEL).all() and (raw[shift + nb:] == SENTINEL).all()
    assert not differs((raw[shift:shift + nb].view(np.float32).reshape(n, dim), diag), want)


def test_workspace_reuse_across_shapes(acc):
    big = sg.seeded_case(41, 1500, 48, 8)
    small = sg.seeded_case(42, 5, 3, 2)
    hubby = sg.seeded_case(43, 300, 16, 4, hub=(7, 900))
    for case, hops in ((big, 2), (small, 3), (hubby, 2), (big, 1), (small, 1), (big, 3)):
        check(acc, *case, hops)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _bad_inputs():
    x, off, cols, w = sg.seeded_case(61, 50, 8, 5, specials=False)
    def variant(**kw):
        d = dict(x=x.copy(), off=off.copy(), cols=cols.copy(), w=w.copy());
        for k, f in kw.items():
            f(d[k])
        return d
    def set_(i, v):
        return lambda a: a.__setitem__(i, v)
    return {
        "column_at_n": variant(cols=set_(3, 50)),
        "column_max": variant(cols=set_(len(cols) - 1, 0xffffffff)),
        "offsets_start": variant(off=set_(0, 1)),
        "offset_decreases": variant(off=set_(20, 0)),
        "negative_weight": variant(w=set_(5, -0.5)),
        "nan_weight": variant(w=set_(0, np.nan)),
        "inf_weight": variant(w=set_(len(w) - 1, np.inf)),
        "nan_row": variant(x=set_((49, 7), np.nan)),
        "inf_row": variant(x=set_((0, 0), -np.inf)),
    }


@pytest.mark.parametrize("name", sorted(_bad_inputs()))
def test_every_refusal_leaves_out_untouched(acc, vtable, name):
    from yams_amd import _lib
    d = _bad_inputs()[name]
    x, off, cols, w = d["x"], d["off"], d["cols"], d["w"]
    with pytest.raises((sg.InvalidArg, sg.Unsupported)):
        sg.smooth(x, off, cols, w, 2)
    n, dim = x.shape
    nb = n * dim * 4
    bufs = [acc.to_device(a) for a in (x, off, cols, w)]
    d_out = acc.alloc(nb + 16); d_out.upload(np.full(nb + 16, SENTINEL, np.uint8))
    try:
        st = acc.L.yams_graph_sgc_smooth_device(acc.ctx, bufs[0].ptr, n, dim, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 2, d_out.ptr, None)
        raw = d_out.download(np.uint8, nb + 16)
    finally:
        for b in bufs + [d_out]:
            b.free()
    assert st == _lib.YAMS_ERR_INVALID_ARG and (raw == SENTINEL).all(), name
    out = np.full((n, dim), 7.0, np.float32)
    st = acc.L.yams_graph_sgc_smooth_host(acc.ctx, x.ctypes.data, n, dim, off.ctypes.data, cols.ctypes.data, w.ctypes.data, 2, out.ctypes.data, None)
    assert st == _lib.YAMS_ERR_INVALID_ARG and (out == 7.0).all(), name
    st, out, _ = through_vtable(vtable, x, off, cols, w, 2, fill=7.0)
    assert st == _lib.YAMS_ERR_INVALID_ARG and (out == 7.0).all(), name
    check(acc, *sg.seeded_case(62, 20, 4, 3), 1)                                   # the context serves the next call


def test_argument_statuses_and_hops_zero(acc, vtable):
    from yams_amd import _lib
    x, off, cols, w = sg.seeded_case(63, 30, 6, 4)
    out, diag = acc.sgc_smooth(x, off, cols, w, 0)
    assert sg.same_bits(out, x)                                                    # hops == 0 copies
    out, _ = acc.sgc_smooth(x, off, cols, w, 0, host_entry=True)
    assert sg.same_bits(out, x)
    st, out, _ = through_vtable(vtable, x, off, cols, w, 0)
    assert st == 0 and sg.same_bits(out, x)
    d_x = acc.to_device(x); d_off = acc.to_device(off)
    try:
        call = lambda rows, n, dim, o, dst: acc.L.yams_graph_sgc_smooth_device(acc.ctx, rows, n, dim, o, None, None, 1, dst, None)
        assert call(None, 0, 6, None, None) == _lib.YAMS_OK                        # n == 0: nothing written
        assert call(d_x.ptr, 30, 0, d_off.ptr, d_x.ptr) == _lib.YAMS_ERR_INVALID_ARG
        assert call(d_x.ptr, 30, 6, d_off.ptr, None) == _lib.YAMS_ERR_INVALID_ARG
        assert call(d_x.ptr, 30, 6, None, d_x.ptr + 4096) == _lib.YAMS_ERR_INVALID_ARG
        assert call(d_x.ptr, 30, 6, d_off.ptr, d_x.ptr + 8) == _lib.YAMS_ERR_INVALID_ARG      # out overlaps rows
        assert call(d_x.ptr, 30, 6, d_off.ptr, d_x.ptr) == _lib.YAMS_ERR_INVALID_ARG
        assert call(d_x.ptr, 30, _lib.SGC_MAX_DIM + 1, d_off.ptr, d_x.ptr) == _lib.YAMS_ERR_UNSUPPORTED
        assert call(d_x.ptr, 1 << 31, 6, d_off.ptr, d_x.ptr) == _lib.YAMS_ERR_UNSUPPORTED
        # edges announced but no cols / weights: refused on the device
        d_out = acc.alloc(30 * 6 * 4)
        assert call(d_x.ptr, 30, 6, d_off.ptr, d_out.ptr) == _lib.YAMS_ERR_INVALID_ARG
        d_out.free()
    finally:
        d_x.free(); d_off.free()


# ---- the plugin door ------------------------------------------------------------------------------------------------------------
def test_concurrent_callers_of_the_vtable(vtable):
    """Four host threads in topology_smooth_v1 at once: every call leases a work context with its own workspace."""
    shapes = [(300, 8, 8, 2), (700, 33, 4, 3), (150, 64, 12, 1), (1100, 5, 6, 2)]
    inputs = [sg.seeded_case(80 + i, n, dim, deg) + (hops,) for i, (n, dim, deg, hops) in enumerate(shapes)]
    wants = [sg.smooth(*inp, with_diag=True) for inp in inputs]
    results = [None] * 4

    def run(i):
        results[i] = [through_vtable(vtable, *inputs[i]) for _ in range(3)]

    threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i in range(4):
        for st, out, diag in results[i]:
            assert st == 0 and not differs((out, diag), wants[i]), (i, differs((out, diag), wants[i]))


def test_shell_through_the_real_plugin_equals_the_scalar_loop():
    """tests/cpp/sgc_test.cpp --plugin: AccelSGC::apply over the real topology_smooth_v1 against the stand-in loop."""
    from _sgc_build import build_sgc_test
    from yams_amd import build as b
    r = subprocess.run([build_sgc_test(), "--plugin", b.LIB], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "3 cases" in r.stdout and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_stress_harness_on_the_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_sgc.py"), "--cases", "60", "--seed", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mode"] == "device" and res["cases"] == 60 and res["skipped"] == 0
    assert all(v > 0 for v in res["paths"].values()), res["paths"]
