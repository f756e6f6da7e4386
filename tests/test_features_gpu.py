"""The topology build's input features on the GPU (yams_features_aggregate / _variance / _compose, _device and _host,
topology_features_v1, the shell over the real plugin) against the restatements of tests/_features_oracle.py and the golden file
made from the reference's own translation unit.  Every output element is compared on bits (fo.equal: where the restatement
has a NaN that arithmetic made, some NaN); every device output is followed by guard bytes that the wrapper checks; every
refusal is made behind guard words that must come back untouched.

The references are computed once per shape by the C++ restatement and left unchanged."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _features_oracle as fo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "features.json")
DIMS = [1, 3, 4, 5, 63, 64, 65, 257, 1024, 4096]
_CACHE = {}


def rows_of(n, dim, seed=0):
    key = ("rows", n, dim, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(9000 + 31 * n + dim + seed)
        x = fo.mixed(rng, (n, dim), -8, 8)
        x.reshape(-1)[rng.integers(0, x.size, max(1, x.size // 50))] = rng.choice(np.array([0.0, -0.0], np.float32), max(1, x.size // 50))
        _CACHE[key] = x
    return _CACHE[key]


# ---- aggregate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_aggregate_list_lengths_at_every_dimension(acc, dim):
    n = 64 if dim >= 1024 else 300
    x = rows_of(n, dim)
    rng = np.random.default_rng(dim)
    lengths = [0, 1, 2, 17, 1000, 0, 1, 3] if dim <= 257 else [0, 1, 2, 17, 1000]
    off = fo.csr(lengths)
    rec = rng.integers(0, n, int(off[-1])).astype(np.uint32)
    want = fo.aggregate_cpp(x, off, rec)
    assert want[1].tolist() == lengths
    for kw in (dict(), dict(misalign=4), dict(host_entry=True)):
        got = acc.features_aggregate(x, off, rec, **kw)
        assert fo.equal(got[0], want[0]) and fo.equal(got[1], want[1]), (dim, kw)
        assert not got[0][0].any() and not got[0][5 if dim <= 257 else 0].any()      # an empty list: zeros


@pytest.mark.parametrize("n_docs", [1, 255, 256, 257, 1000])
def test_aggregate_document_counts(acc, n_docs):
    x = rows_of(500, 65)
    rng = np.random.default_rng(n_docs)
    off = fo.csr(rng.choice([0, 1, 2, 5], n_docs))
    rec = rng.integers(0, 500, int(off[-1])).astype(np.uint32)
    want = fo.aggregate_cpp(x, off, rec)
    for host in (False, True):
        got = acc.features_aggregate(x, off, rec, host_entry=host)
        assert fo.equal(got[0], want[0]) and fo.equal(got[1], want[1])


def test_aggregate_assigns_the_first_record(acc):
    """A lone record keeps its bits (-0.0f, a NaN's payload); -0.0f + -0.0f stays -0.0f where a `0.0f +` start gives +0.0f."""
    nz = np.float32(-0.0)
    payload = np.array([0x7fc12345, 0xffc00001, 0x7f800001], np.uint32).view(np.float32)      # two quiet NaNs and a signalling one
    x = np.array([[nz, 1, payload[0]], [nz, 2, payload[1]], [0, nz, payload[2]]], np.float32)
    off, rec = fo.csr([1, 1, 1, 2, 2]), np.array([0, 1, 2, 0, 1, 0, 2], np.uint32)
    want = fo.aggregate_py(x, off, rec)
    for host in (False, True):
        got, cnt = acc.features_aggregate(x, off, rec, host_entry=host)
        assert fo.same_bits(got[:3], x) and cnt.tolist() == [1, 1, 1, 2, 2]      # assigned: bit for bit, payloads included
        assert fo.equal(got, want[0])
        assert np.signbit(got[3, 0]) and got[3, 1] == 1.5 and not np.signbit(got[4, 0])


# ---- variance ----------------------------------------------------------------------------------------------------------------
def forms_differing_sample(m, dim):
    """Rows whose two oracle forms differ in at least one variance (the first seed that does), with both oracle results.  Below
    three rows no input can: at m == 1 every residual is 0, at m == 2 it is half a difference of two floats, whose square is
    exact in fp64."""
    key = ("var", m, dim)
    if key not in _CACHE:
        for seed in range(400):
            x = fo.mixed(np.random.default_rng(7000 + 1000 * dim + 13 * m + seed), (m, dim), -2, 2)
            want = [fo.variance_cpp(x, None, f) for f in (fo.SEPARATE, fo.FUSED)]
            differ = not fo.same_bits(want[0][1], want[1][1])
            if differ or m < 3:
                break
        assert differ == (m >= 3), (m, dim, "no seed whose forms differ")
        _CACHE[key] = (x, want)
    return _CACHE[key]


@pytest.mark.parametrize("dim", DIMS)
def test_variance_both_forms_at_every_dimension(acc, dim):
    for m in (1, 2, 4096 if dim in (64, 65) else 37):
        x, want = forms_differing_sample(m, dim)
        for form in (fo.SEPARATE, fo.FUSED):
            got = acc.features_variance(x, form=form)
            assert fo.equal(got[0], want[form][0]) and fo.equal(got[1], want[form][1]), (dim, m, form)
    x, want = forms_differing_sample(37, dim)
    for form in (fo.SEPARATE, fo.FUSED):
        for kw in (dict(misalign=4), dict(host_entry=True)):
            got = acc.features_variance(x, form=form, **kw)
            assert fo.equal(got[0], want[form][0]) and fo.equal(got[1], want[form][1]), (dim, form, kw)


def test_variance_select_reorders_repeats_and_drops_rows(acc):
    x = rows_of(300, 257, seed=5)
    rng = np.random.default_rng(3)
    for sel in (rng.permutation(300)[:100], rng.integers(0, 300, 4096), np.array([299, 0, 299, 5, 5]), np.array([7]), np.array([], np.int64)):
        sel = sel.astype(np.uint32)
        for form in (fo.SEPARATE, fo.FUSED):
            for host in (False, True):
                got = acc.features_variance(x, select=sel, form=form, host_entry=host)
                if len(sel) == 0:
                    assert got == (None, None)      # m == 0: YAMS_OK, nothing written (the wrapper checked the guard words)
                    continue
                want = fo.variance_cpp(x, sel, form)
                assert fo.equal(got[0], want[0]) and fo.equal(got[1], want[1]), (len(sel), form, host)


def test_variance_serves_what_ieee_gives(acc):
    x = rows_of(9, 5, seed=5).copy()
    x[3, 1], x[4, 2], x[5, 3] = np.inf, np.nan, -0.0
    for form in (fo.SEPARATE, fo.FUSED):
        want = fo.variance_cpp(x, None, form)
        got = acc.features_variance(x, form=form)
        assert fo.equal(got[0], want[0]) and fo.equal(got[1], want[1]) and np.isnan(got[1][1]) and np.isnan(got[1][2])


def test_the_python_restatement_agrees_where_it_is_quick_enough(acc):
    x, want = forms_differing_sample(37, 5)
    for form in (fo.SEPARATE, fo.FUSED):
        py = fo.variance_py(x, None, form)
        assert fo.same_bits(py[0], want[form][0]) and fo.same_bits(py[1], want[form][1])


# ---- compose -----------------------------------------------------------------------------------------------------------------
def compose_case(n, dim, k, sig_len, sketch_dim, weights, seed=0):
    key = ("compose", n, dim, k, sig_len, sketch_dim, weights, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(4000 + n + 7 * dim + sig_len + sketch_dim + seed)
        x = rows_of(n, dim, seed=11).copy()
        x[0] = 0.0                                                       # sumSq == 0
        if n > 2:
            x[1] = fo.HUGE                                               # the norm rounds to inf (dim > 1) or is the element
            x[2] = 0.0
            x[2, dim // 2] = fo.TINY                                     # the smallest norm there is
        w = None
        if weights:
            w = np.abs(fo.mixed(rng, dim, -3, 3))
            w[rng.random(dim) < 0.5] = 0.0
            if dim > 4:
                w[1], w[3] = np.nan, -1.0
        ent = fo.mixed(rng, (n, k), -2, 2) if k else None
        sig = rng.integers(0, 1 << 32, (n, sig_len), dtype=np.uint64).astype(np.uint32) if sig_len else None
        if sig is not None and n > 3:
            sig[3] = 5                                                   # every element in one bucket
        eon = (np.arange(n) & 1).astype(np.uint8)
        son = ((np.arange(n) >> 1) & 1).astype(np.uint8)                 # the four combinations, row after row
        args = (x, w, ent, eon, sig, son, sketch_dim, 0.25, 0.125)
        _CACHE[key] = (args, fo.compose_cpp(*args))
    return _CACHE[key]


def check_compose(acc, args, want, **kw):
    got = acc.features_compose(*args, **kw)
    assert fo.equal(got[1], want[1]), "out_dims"
    assert fo.equal(got[0], want[0]), "out"


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("dim", DIMS)
def test_compose_at_every_dimension(acc, dim, weights):
    args, want = compose_case(257, dim, 16, 256, 64, weights)
    assert len(set(want[1].tolist())) == 4      # the four (entityOn, minhashOn) combinations have four lengths
    check_compose(acc, args, want)
    check_compose(acc, args, want, misalign=4)
    if dim in (5, 64, 1024):
        check_compose(acc, args, want, host_entry=True)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_compose_row_counts(acc, n):
    for weights in (False, True):
        args, want = compose_case(n, 65, 3, 7, 7, weights)
        check_compose(acc, args, want)
        check_compose(acc, args, want, host_entry=True)


@pytest.mark.parametrize("sketch_dim", [1, 7, 64, 4096])
def test_compose_sketch_shapes(acc, sketch_dim):
    for sig_len in (1, 256, 65536):
        n = 6 if sig_len == 65536 else 40
        args, want = compose_case(n, 5, 0, sig_len, sketch_dim, False)
        check_compose(acc, args, want)
    args, want = compose_case(6, 5, 4096, 256, sketch_dim, True)      # K at its limit
    check_compose(acc, args, want, host_entry=True)


def test_compose_parts_switched_off_and_a_wider_stride(acc):
    args, want = compose_case(40, 63, 3, 11, 7, True)
    x, w, ent, eon, sig, son, sd, ae, am = args
    for a in ((x, w, None, None, sig, son, sd, ae, am), (x, w, ent, eon, None, None, 0, ae, am), (x, None, None, None, None, None, 0, ae, am),
              (x, w, ent, eon, sig, son, 0, ae, am), (x, np.zeros(63, np.float32), ent, eon, sig, son, sd, ae, am),
              (x, w, ent, eon, sig, son, sd, float("nan"), am), (x, w, ent, eon, sig, son, sd, 0.75, 0.5)):
        exp = fo.compose_cpp(*a)
        for host in (False, True):
            check_compose(acc, a, exp, host_entry=host)
    wide = fo.compose_cpp(*args, out_stride=want[0].shape[1] + 9)
    assert not wide[0][:, -9:].any()
    check_compose(acc, args, wide, out_stride=want[0].shape[1] + 9)
    # both parts off on every row: the dense part alone, no multiply
    off = acc.features_compose(x, None, ent, np.zeros(40, np.uint8), sig, np.zeros(40, np.uint8), sd, ae, am)
    plain = fo.compose_cpp(x, None, None, None, None, None, 0, ae, am)
    assert fo.equal(off[0][:, :63], plain[0]) and (off[1] == 63).all() and not off[0][:, 63:].any()


def test_the_python_restatement_of_compose_agrees(acc):
    args, want = compose_case(40, 63, 3, 11, 7, True)
    py = fo.compose_py(*args)
    assert fo.same_bits(py[0], want[0]) and fo.same_bits(py[1], want[1])


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def refused(call):
    from yams_amd._lib import AccelError
    with pytest.raises(AccelError) as e:
        call()
    return e.value.status


def test_refusals_write_nothing(acc):
    """The wrapper fills every output with guard words and checks, after a refusal, that all of them are still there."""
    from yams_amd import _lib
    inv, unsup = _lib.YAMS_ERR_INVALID_ARG, _lib.YAMS_ERR_UNSUPPORTED
    x = rows_of(40, 5)
    off, rec = fo.csr([2, 0, 3]), np.array([0, 1, 5, 6, 39], np.uint32)
    args, want = compose_case(40, 63, 3, 11, 7, True)
    cx, w, ent, eon, sig, son, sd, ae, am = args
    for host in (False, True):
        kw = dict(host_entry=host)
        # aggregate
        assert refused(lambda: acc.features_aggregate(np.zeros((3, 0), np.float32), off, rec[:0], **kw)) == inv                  # dim == 0
        assert refused(lambda: acc.features_aggregate(x, np.array([1, 2, 5, 5], np.uint64), rec, **kw)) == inv                   # offsets do not start at 0
        assert refused(lambda: acc.features_aggregate(x, np.array([0, 3, 2, 5], np.uint64), rec, **kw)) == inv                   # offsets decrease
        assert refused(lambda: acc.features_aggregate(x, off, np.array([0, 1, 5, 40, 39], np.uint32), **kw)) == inv              # index out of range
        assert refused(lambda: acc.features_aggregate(np.zeros((2, 4097), np.float32), fo.csr([1]), rec[:1], **kw)) == unsup     # dim > 4096
        # variance
        assert refused(lambda: acc.features_variance(np.zeros((3, 0), np.float32), **kw)) == inv
        assert refused(lambda: acc.features_variance(x, form=2, **kw)) == inv                                                    # unknown form
        assert refused(lambda: acc.features_variance(x, select=np.array([0, 40, 1], np.uint32), **kw)) == inv
        assert refused(lambda: acc.features_variance(np.zeros((2, 4097), np.float32), **kw)) == unsup
        # compose
        assert refused(lambda: acc.features_compose(np.zeros((3, 0), np.float32), **kw)) == inv
        assert refused(lambda: acc.features_compose(*args, out_stride=want[0].shape[1] - 1, **kw)) == inv                        # out_stride too small
        assert refused(lambda: acc.features_compose(cx, w, ent, None, sig, son, sd, ae, am, **kw)) == inv                        # a part without its switch
        assert refused(lambda: acc.features_compose(cx, w, ent, eon, sig, None, sd, ae, am, **kw)) == inv
        assert refused(lambda: acc.features_compose(np.zeros((2, 4097), np.float32), **kw)) == unsup
        assert refused(lambda: acc.features_compose(cx, w, np.zeros((40, 4097), np.float32), eon, sig, son, sd, ae, am, **kw)) == unsup   # K
        assert refused(lambda: acc.features_compose(cx, w, ent, eon, sig, son, 4097, ae, am, **kw)) == unsup                     # sketch_dim
        assert refused(lambda: acc.features_compose(cx[:2], w, ent[:2], eon[:2], np.zeros((2, 65537), np.uint32), son[:2], sd, ae, am, **kw)) == unsup
    L, ctx = acc.L, acc.ctx
    d = acc.to_device(x)
    d_off, d_rec = acc.to_device(off), acc.to_device(rec)
    o = acc.alloc(1 << 16)
    f = C.c_float
    # null arrays, a null context, the 2^31 limits, outputs that overlap an input
    assert L.yams_features_aggregate_device(None, d.ptr, 40, 5, d_off.ptr, d_rec.ptr, 3, o.ptr, o.ptr + 4096) == inv
    assert L.yams_features_aggregate_device(ctx, d.ptr, 40, 5, None, d_rec.ptr, 3, o.ptr, o.ptr + 4096) == inv
    assert L.yams_features_aggregate_device(ctx, d.ptr, 40, 5, d_off.ptr, d_rec.ptr, 3, None, o.ptr + 4096) == inv
    assert L.yams_features_aggregate_device(ctx, None, 40, 5, d_off.ptr, d_rec.ptr, 3, o.ptr, o.ptr + 4096) == inv
    assert L.yams_features_aggregate_device(ctx, d.ptr, 40, 5, d_off.ptr, d_rec.ptr, 3, d.ptr + 8, o.ptr) == inv                 # out overlaps rows
    assert L.yams_features_aggregate_device(ctx, d.ptr, 1 << 31, 5, d_off.ptr, d_rec.ptr, 3, o.ptr, o.ptr + 4096) == unsup
    assert L.yams_features_aggregate_device(ctx, d.ptr, 40, 5, d_off.ptr, d_rec.ptr, 1 << 31, o.ptr, o.ptr + 4096) == unsup
    assert L.yams_features_aggregate_device(ctx, d.ptr, 40, 5, None, None, 0, None, None) == 0                                   # n_docs == 0
    assert L.yams_features_variance_device(ctx, None, 40, 5, None, 0, 0, o.ptr, o.ptr + 4096) == inv
    assert L.yams_features_variance_device(ctx, d.ptr, 40, 5, None, 0, 0, None, o.ptr) == inv
    assert L.yams_features_variance_device(ctx, d.ptr, 40, 5, None, 0, 0, d.ptr, o.ptr) == inv                                   # out_mean overlaps rows
    assert L.yams_features_variance_device(ctx, d.ptr, 40, 5, None, 0, 0, o.ptr, o.ptr + 8) == inv                               # the outputs overlap
    assert L.yams_features_variance_device(ctx, d.ptr, 1 << 31, 5, None, 0, 0, o.ptr, o.ptr + 4096) == unsup
    assert L.yams_features_variance_device(ctx, d.ptr, 40, 5, d_rec.ptr, 1 << 32, 0, o.ptr, o.ptr + 4096) == unsup
    assert L.yams_features_variance_device(ctx, None, 0, 5, None, 0, 0, None, None) == 0                                         # m == 0
    assert L.yams_features_variance_device(ctx, None, 0, 5, None, 0, 7, None, None) == inv                                       # ... after the form
    z = f(0.0)
    assert L.yams_features_compose_device(ctx, None, 40, 5, None, None, 0, None, None, 0, None, 0, z, z, o.ptr, 5, o.ptr + 4096) == inv
    assert L.yams_features_compose_device(ctx, d.ptr, 40, 5, None, None, 0, None, None, 0, None, 0, z, z, None, 5, o.ptr + 4096) == inv
    assert L.yams_features_compose_device(ctx, d.ptr, 40, 5, None, None, 0, None, None, 0, None, 0, z, z, d.ptr + 400, 5, o.ptr) == inv   # overlap
    assert L.yams_features_compose_device(ctx, d.ptr, 1 << 31, 5, None, None, 0, None, None, 0, None, 0, z, z, o.ptr, 5, o.ptr + 4096) == unsup
    assert L.yams_features_compose_device(ctx, None, 0, 5, None, None, 0, None, None, 0, None, 0, z, z, None, 0, None) == 0      # n == 0
    assert L.yams_features_compose_host(None, x.ctypes.data, 40, 5, None, None, 0, None, None, 0, None, 0, z, z, None, 5, None) == inv
    for b in (d, d_off, d_rec, o):
        b.free()
    # the context still serves after the refusals
    check_compose(acc, args, want)


# ---- the golden file: what the reference's own functions returned -----------------------------------------------------------
def golden():
    return json.load(open(GOLDEN))["cases"]


def accel_restated(acc, form, host):
    return fo.restated(form,
                       lambda rows, off, rec: acc.features_aggregate(rows, off, rec, host_entry=host),
                       lambda rows, sel, f: acc.features_variance(rows, select=sel, form=f, host_entry=host),
                       fo.weights_cpp,
                       lambda *a: acc.features_compose(*a, host_entry=host))


def nan_blind(cases):
    """The cases' vectors with every NaN replaced by one pattern (a NaN that arithmetic made is some NaN)."""
    out = []
    for vectors in cases:
        row = []
        for v in vectors:
            a = np.frombuffer(bytes.fromhex(v), np.float32).copy()
            a[np.isnan(a)] = np.float32(np.nan)
            row.append(fo.hexbits(a))
        out.append(row)
    return out


@pytest.mark.parametrize("host", [False, True])
def test_the_entries_equal_the_golden_file(acc, host):
    cases = golden()
    assert [c["name"] for c in cases] == fo.case_names()
    for form in ("separate", "fused"):
        got = accel_restated(acc, fo.FORMS[form], host)
        assert nan_blind(got) == nan_blind([c[form] for c in cases]), form
    assert sum(c["forms_differ"] for c in cases) >= 4


@pytest.fixture(scope="module")
def vtable():
    from yams_amd import _lib
    L = _lib.load()
    assert L.yams_plugin_init(b'{"device":0}', None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"topology_features_v1", 1, C.byref(p)) == 0
    yield C.cast(p, C.POINTER(_lib.TopologyFeaturesV1)).contents
    L.yams_plugin_shutdown()


def test_the_plugin_interface_equals_the_golden_file(vtable):
    from yams_amd import _lib
    assert vtable.abi_version == 1
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731

    def aggregate(rows, off, rec):
        rows, off, rec = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(rec, np.uint32)
        d, dim = len(off) - 1, rows.shape[1]
        out, cnt = np.empty((d, dim), np.float32), np.empty(d, np.uint32)
        assert vtable.aggregate(None, p(rows), len(rows), dim, p(off), p(rec), d, p(out), p(cnt)) == 0
        return out, cnt

    def variance(rows, sel, form):
        rows = np.ascontiguousarray(rows, np.float32)
        mean, var = np.empty(rows.shape[1]), np.empty(rows.shape[1])
        assert vtable.variance(None, p(rows), len(rows), rows.shape[1], None, 0, form, p(mean), p(var)) == 0
        return mean, var

    def compose(dense, w, ent, eon, sig, son, sd, ae, am):
        dense = np.ascontiguousarray(dense, np.float32)
        n, dim = dense.shape
        k, sl = 0 if ent is None else ent.shape[1], 0 if sig is None else sig.shape[1]
        stride = fo.longest_row(dim, w, ent, k, sig, sl, sd)
        out, dims = np.empty((n, stride), np.float32), np.empty(n, np.uint32)
        arrs = [None if a is None else np.ascontiguousarray(a) for a in (w, ent, eon, sig, son)]
        assert vtable.compose(None, p(dense), n, dim, p(arrs[0]), p(arrs[1]), k, p(arrs[2]), p(arrs[3]), sl, p(arrs[4]), sd, ae, am, p(out), stride, p(dims)) == 0
        return out, dims

    cases = golden()
    for form in ("separate", "fused"):
        got = fo.restated(fo.FORMS[form], aggregate, variance, fo.weights_cpp, compose)
        assert nan_blind(got) == nan_blind([c[form] for c in cases]), form
    # a refusal comes back as its status
    x = np.zeros((2, 3), np.float32)
    out = np.zeros(3)
    assert vtable.variance(None, p(x), 2, 3, None, 0, 9, p(out), p(out.copy())) == _lib.YAMS_ERR_INVALID_ARG


@pytest.mark.parametrize("form", ["separate", "fused"])
def test_shell_through_the_real_plugin_equals_the_golden_file(form):
    """include/yams_accel/topology_features.hpp over the real topology_features_v1 against what the reference's own functions
    returned; the shell's probe, asked about the device, reports the form it was created with."""
    from _features_build import build_shell_test
    from yams_amd import _lib
    exe = build_shell_test()
    cases = golden()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.bin")
        fo.write_cases(path)
        r = subprocess.run([exe, *(["--fused"] if form == "fused" else []), "--plugin", _lib.LIB_PATH, path], capture_output=True, text=True,
                           timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    probe, got = fo.parse_driver_output(r.stdout)
    assert probe == form
    assert nan_blind(got) == nan_blind([c[form] for c in cases])


def test_stress_harness():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_features.py"), "--cases", "60"], capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0 and "60 cases, 0 failures OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
