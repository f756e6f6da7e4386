"""The late-interaction rerank on the GPU (yams_rerank_maxsim / _maxpool, _device and _host, late_interaction_rerank_v1, the
shell over the real plugin) against the C++ restatement (tests/cpp/rerank_oracle.cpp) and the golden file made from the
reference's own member functions.  Scores, row maxima and winning tokens are compared on bits (ro.equal: a NaN matches any NaN);
every device output is followed by guard bytes that the wrapper checks; every refusal is made behind guard words that must come
back untouched.

The lattice sits at the kernel's tiles: 32 query tokens per workgroup, 256 document tokens per pass (four waves x two MFMA
accumulators of 32), 32 dimensions per stage, an MFMA k step of 2.  The references are computed once per shape and left
unchanged."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _rerank_oracle as ro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "colbert_maxsim.json")
DIMS = [1, 3, 4, 47, 48, 49, 64, 127, 128]
QT, DT = 32, 256
TQS = [0, 1, QT - 1, QT, QT + 1, 2 * QT + 1]
LENS = [0, 1, DT - 1, DT, DT + 1, 2 * DT + 1]
FORMS = [ro.SEPARATE, ro.FUSED]
_CACHE = {}


def golden():
    return json.load(open(GOLDEN))["cases"]


def window(dim, tq, lengths, seed=0):
    """(query, rows, off, {form: (scores, rowmax, rowarg)}) — drawn and restated once."""
    key = (dim, tq, tuple(lengths), seed)
    if key not in _CACHE:
        rng = np.random.default_rng(4000 + 97 * dim + 13 * tq + len(lengths) + seed)
        off = ro.csr(lengths)
        q, x = ro.mixed(rng, (tq, dim), -3, 3), ro.mixed(rng, (int(off[-1]), dim), -3, 3)
        _CACHE[key] = (q, x, off, {f: ro.maxsim_cpp(q, x, off, f) for f in FORMS})
    return _CACHE[key]


def check(acc, q, x, off, form, want, **kw):
    from yams_amd import _lib
    sc, mx, arg, diag = acc.rerank_maxsim(q, x, off, form=form, want_rowmax=True, **kw)
    assert ro.equal(sc, want[0]) and ro.equal(mx, want[1]) and ro.equal(arg, want[2]), (q.shape, len(off) - 1, form, kw)
    assert diag["form"] == form and diag["docs"] == len(off) - 1 and diag["rows"] == int(off[-1]) and diag["query_tokens"] == len(q)
    assert diag["path"] == (_lib.RERANK_PATH_MFMA if form == ro.FUSED else _lib.RERANK_PATH_VALU), diag
    sc2, _ = acc.rerank_maxsim(q, x, off, form=form, **kw)      # without the row maxima: the same scores
    assert ro.equal(sc2, want[0])


# ---- the golden file ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
def test_the_flat_entries_equal_the_golden_file(acc, host):
    cases = golden()
    for form in ("separate", "fused"):
        got = ro.restated(ro.FORMS[form], lambda q, x, off, f: acc.rerank_maxsim(q, x, off, form=f, host_entry=host)[0],
                          lambda x, off: acc.rerank_maxpool(x, off, host_entry=host))
        want = [c[form] for c in cases]
        assert ro.nan_blind(got) == ro.nan_blind(want), [c["name"] for c, g, w in zip(cases, ro.nan_blind(got), ro.nan_blind(want)) if g != w]
    assert sum(c["forms_differ"] for c in cases) >= 4


@pytest.fixture(scope="module")
def vtable():
    from yams_amd import _lib
    L = _lib.load()
    assert L.yams_plugin_init(b'{"device":0}', None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"late_interaction_rerank_v1", 1, C.byref(p)) == 0
    yield C.cast(p, C.POINTER(_lib.LateInteractionRerankV1)).contents
    L.yams_plugin_shutdown()


def test_the_plugin_interface_equals_the_golden_file(vtable):
    from yams_amd import _lib
    assert vtable.abi_version == 1
    p = lambda a: a.ctypes.data if a.size else None      # noqa: E731

    def maxsim(q, x, off, form):
        q, x, off = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(x, np.float32), np.ascontiguousarray(off, np.uint64)
        d = len(off) - 1
        out, dg = np.empty(d, np.float32), _lib.RerankDiag()
        assert vtable.maxsim(None, p(q), q.shape[0], q.shape[1], p(x), p(off), d, form, p(out), None, None, C.byref(dg)) == 0
        assert dg.form == form and dg.docs == d
        return out

    def maxpool(x, off):
        x, off = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(off, np.uint64)
        out = np.empty((len(off) - 1, x.shape[1]), np.float32)
        assert vtable.maxpool(None, p(x), x.shape[1], p(off), len(off) - 1, p(out)) == 0
        return out

    cases = golden()
    for form in ("separate", "fused"):
        assert ro.nan_blind(ro.restated(ro.FORMS[form], maxsim, maxpool)) == ro.nan_blind([c[form] for c in cases]), form
    # a refusal comes back as its status, the outputs untouched
    q, out = np.zeros((1, 2), np.float32), np.full(1, 7.0, np.float32)
    off = np.array([0, 1], np.uint64)
    assert vtable.maxsim(None, p(q), 1, 2, p(q), p(off), 1, 9, p(out), None, None, None) == _lib.YAMS_ERR_INVALID_ARG and out[0] == 7.0


@pytest.mark.parametrize("form", ["separate", "fused"])
def test_shell_through_the_real_plugin_equals_the_golden_file(form):
    """include/yams_accel/colbert_rerank.hpp over the real late_interaction_rerank_v1, with a host function of the form: the
    probe finds it, the device serves every case (the driver fails if the host function had to), the bits are the reference's."""
    from _rerank_build import build_shell_test
    from yams_amd import _lib
    exe = build_shell_test()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.bin")
        ro.write_cases(path)
        r = subprocess.run([exe, *(["--fused"] if form == "fused" else []), "--plugin", _lib.LIB_PATH, path], capture_output=True, text=True,
                           timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    probe, got = ro.parse_driver_output(r.stdout)
    assert probe == form
    assert ro.nan_blind(got) == ro.nan_blind([c[form] for c in golden()])


# ---- the lattice -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_every_dimension_over_the_length_lattice(acc, dim):
    """Documents of every lattice length in one window, a query of two tiles plus one."""
    q, x, off, want = window(dim, 2 * QT + 1, LENS)
    for form in FORMS:
        check(acc, q, x, off, form, want[form])
    check(acc, q, x, off, ro.FUSED, want[ro.FUSED], misalign=4)
    check(acc, q, x, off, ro.SEPARATE, want[ro.SEPARATE], host_entry=True)


@pytest.mark.parametrize("tq", TQS)
def test_every_query_length(acc, tq):
    for dim in (47, 64):
        q, x, off, want = window(dim, tq, [DT + 1, 0, 1, QT - 1])
        for form in FORMS:
            check(acc, q, x, off, form, want[form])
            if tq == 0:
                assert not want[form][0].view(np.uint32).any()      # an empty query: +0.0f


@pytest.mark.parametrize("length", LENS)
def test_one_document_of_every_length(acc, length):
    q, x, off, want = window(48, QT + 1, [length])
    for form in FORMS:
        check(acc, q, x, off, form, want[form])
        check(acc, q, x, off, form, want[form], host_entry=True)
        if length == 0:
            assert (want[form][0] == -np.inf).all() and (want[form][2] == ro.NONE).all()


def test_300_documents_of_mixed_lengths(acc):
    rng = np.random.default_rng(300)
    lengths = rng.choice([0, 0, 1, 2, 17, 31, 32, 33, 64, 100], 300)
    q, x, off, want = window(48, QT, lengths.tolist())
    assert (lengths == 0).sum() >= 20
    for form in FORMS:
        check(acc, q, x, off, form, want[form])
    check(acc, q, x, off, ro.FUSED, want[ro.FUSED], host_entry=True)


PLANTS = [0, 1, 31, 32, 63, 64, DT - 1, DT, DT + 1, 2 * DT - 1, 2 * DT]      # first, last, every tile, wave and accumulator edge


@pytest.mark.parametrize("dim", [3, 48])
def test_the_winner_planted_at_every_edge(acc, dim):
    """One document per plant: 2 * DT + 1 small tokens, and at the planted position the second query token itself, scaled: its
    sim with that token is a sum of squares no other token reaches.  out_rowarg names the position; the bits are the oracle's."""
    key = ("plant", dim)
    if key not in _CACHE:
        rng = np.random.default_rng(50 + dim)
        n = 2 * DT + 1
        q = ro.mixed(rng, (3, dim), -1, 1)
        x = ro.mixed(rng, (n * len(PLANTS), dim), -6, -4)
        for d, p in enumerate(PLANTS):
            x[d * n + p] = q[1] * np.float32(8.0)
        off = ro.csr([n] * len(PLANTS))
        _CACHE[key] = (q, x, off, {f: ro.maxsim_cpp(q, x, off, f) for f in FORMS})
    q, x, off, want = _CACHE[key]
    for form in FORMS:
        assert want[form][2][:, 1].tolist() == PLANTS      # the oracle itself finds the plants
        check(acc, q, x, off, form, want[form])
    check(acc, q, x, off, ro.FUSED, want[ro.FUSED], host_entry=True)


def test_equal_zeros_of_both_signs_keep_the_first(acc):
    for q, rows, off, bits in ro.zero_tie_cases():
        for form in FORMS:
            want = ro.maxsim_cpp(q, rows, off, form)
            assert want[1].view(np.uint32)[:, 0].tolist() == bits[form] and not want[2].any()
            check(acc, q, rows, off, form, want)
    # the same tie across a pass boundary and across waves: zeros everywhere, the first token stays
    for form in FORMS:
        q, x = np.zeros((2, 5), np.float32), np.zeros((2 * DT + 1, 5), np.float32)
        x[1::2] = -0.0
        q[1] = -1.0
        want = ro.maxsim_cpp(q, x, ro.csr([2 * DT + 1]), form)
        assert not want[2].any()
        check(acc, q, x, ro.csr([2 * DT + 1]), form, want)


def test_special_values_flow_as_the_chain_carries_them(acc):
    rng = np.random.default_rng(77)
    q, x = ro.mixed(rng, (QT + 1, 49), -3, 3), ro.mixed(rng, (DT + 40, 49), -3, 3)
    for a in (q, x):
        flat = a.reshape(-1)
        k = flat.size // 40
        flat[rng.integers(0, flat.size, k)] = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-42, -1e-42, 3e38], np.float32), k)
    x[7] = np.nan      # a row of NaNs never wins
    off = ro.csr([DT + 1, 0, 39])
    for form in FORMS:
        want = ro.maxsim_cpp(q, x, off, form)
        assert np.isnan(want[0]).any() or np.isinf(want[0]).any()
        check(acc, q, x, off, form, want)
    # subnormals are kept: products and sums below 2^-126
    q, x = ro.mixed(rng, (3, 48), -70, -66), ro.mixed(rng, (9, 48), -75, -70)      # products in 2^-145 .. 2^-134: 48 of them stay below 2^-126
    for form in FORMS:
        want = ro.maxsim_cpp(q, x, ro.csr([9]), form)
        assert want[0][0] != 0 and abs(want[0][0]) < 1.2e-38
        check(acc, q, x, ro.csr([9]), form, want)


# ---- pooling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 3, 48, 127, 128, 257, 1024])
def test_maxpool_at_every_dimension(acc, dim):
    rng = np.random.default_rng(dim)
    lengths = [0, 1, 2, 17, 300] if dim <= 128 else [0, 1, 9]
    off = ro.csr(lengths)
    x = ro.mixed(rng, (int(off[-1]), dim), -6, 6)
    flat = x.reshape(-1)
    k = max(1, flat.size // 30)
    flat[rng.integers(0, flat.size, k)] = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-42], np.float32), k)
    want = ro.maxpool_cpp(x, off)
    assert ro.equal(want, ro.maxpool_py(x, off)) and not want[0].any()
    for kw in (dict(), dict(misalign=4), dict(host_entry=True)):
        assert ro.equal(acc.rerank_maxpool(x, off, **kw), want), (dim, kw)


def test_maxpool_small_norms(acc):
    x = np.array([[1e-9, -1e-9, 3e-9], [2e-9, 0, 0], [1e-8, 2e-9, 0], [1e-30, 1e-25, -1], [1e-42, 1e-40, 0]], np.float32)
    off = ro.csr([2, 1, 1, 1])
    want = ro.maxpool_cpp(x, off)
    assert not want[0].any() and want[1][0] > 0.9 and want[2][2] == -1.0 and not want[3].any()      # subnormals: a norm below 1e-8
    for host in (False, True):
        assert ro.equal(acc.rerank_maxpool(x, off, host_entry=host), want)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def refused(acc, host, status, q, x, off, form=0, tq=None, dim=None, n_docs=None, outs=(True, True, True)):
    """The call with every output behind guard words (the wrapper's _artifact_call asserts that a refusal left them as they
    were); arrays may be None: a null pointer."""
    from yams_amd import _lib
    tq = q.shape[0] if tq is None else tq
    dim = q.shape[1] if dim is None else dim
    d = len(off) - 1 if n_docs is None else n_docs
    dg = _lib.RerankDiag(path=77)
    specs = [(np.float32, max(d, 1)) if outs[0] else None, (np.float32, max(d * tq, 1)) if outs[1] else None,
             (np.uint32, max(d * tq, 1)) if outs[2] else None]
    with pytest.raises(_lib.AccelError) as e:
        acc._artifact_call(acc.L.yams_rerank_maxsim_device, acc.L.yams_rerank_maxsim_host, host, [q, x, off], specs,
                           lambda i, o: (i[0], tq, dim, i[1], i[2], d, form, o[0], o[1], o[2], C.byref(dg)))
    assert e.value.status == status, (e.value, status)
    assert dg.path == 77      # the diag is an output too


@pytest.mark.parametrize("host", [False, True])
def test_refusals_leave_every_output_untouched(acc, host):
    from yams_amd import _lib
    inv, uns = _lib.YAMS_ERR_INVALID_ARG, _lib.YAMS_ERR_UNSUPPORTED
    q, x = np.ones((2, 4), np.float32), np.ones((5, 4), np.float32)
    off = np.array([0, 2, 5], np.uint64)
    refused(acc, host, inv, q, x, off, form=2)                                                  # an unknown form
    refused(acc, host, inv, q, x, off, dim=0)                                                   # dim == 0
    refused(acc, host, uns, q, x, off, dim=_lib.RERANK_MAX_DIM + 1)                             # above the limit
    refused(acc, host, uns, q, x, off, tq=_lib.RERANK_MAX_QUERY_TOKENS + 1, outs=(True, False, False))
    refused(acc, host, uns, q, x, off, n_docs=_lib.RERANK_MAX_DOCS + 1, outs=(True, False, False))
    refused(acc, host, uns, q, x, np.zeros((1 << 16) + 1, np.uint64), tq=(1 << 11) + 1, outs=(True, False, False))      # n_docs * tq
    refused(acc, host, inv, q, x, np.array([0, 3, 2], np.uint64))                               # decreasing
    refused(acc, host, inv, q, x, np.array([1, 2, 5], np.uint64))                               # not from 0
    refused(acc, host, inv, None, x, off, tq=2, dim=4)                                                    # null query
    refused(acc, host, inv, q, None, off)                                                       # null rows
    refused(acc, host, inv, q, x, None, n_docs=2)                                               # null offsets
    refused(acc, host, inv, q, x, off, outs=(False, True, True))                                # null out_scores
    long = np.array([0, _lib.RERANK_MAX_DOC_TOKENS + 1], np.uint64)
    refused(acc, host, uns, q, x, long)                                                         # a document too long (nothing is read)
    # maxpool
    for args, status in (((x, np.array([0, 3, 2], np.uint64)), inv), ((x, np.array([2, 3, 5], np.uint64)), inv)):
        with pytest.raises(_lib.AccelError) as e:
            acc.rerank_maxpool(*args, host_entry=host)
        assert e.value.status == status
    for dim, status in ((0, inv), (_lib.RERANK_MAX_DIM + 1, uns)):
        with pytest.raises(_lib.AccelError) as e:
            acc._artifact_call(acc.L.yams_rerank_maxpool_device, acc.L.yams_rerank_maxpool_host, host, [x, off], [(np.float32, 64)],
                               lambda i, o: (i[0], dim, i[1], 2, o[0]))
        assert e.value.status == status
    # n_docs == 0 is YAMS_OK and writes nothing
    out, = acc._artifact_call(acc.L.yams_rerank_maxsim_device, acc.L.yams_rerank_maxsim_host, host, [q, x, off], [(np.uint8, 16)],
                              lambda i, o: (i[0], 2, 4, i[1], i[2], 0, 0, o[0], None, None, None))
    assert (out == acc._GUARD).all()
    out, = acc._artifact_call(acc.L.yams_rerank_maxpool_device, acc.L.yams_rerank_maxpool_host, host, [x, off], [(np.uint8, 16)],
                              lambda i, o: (i[0], 4, i[1], 0, o[0]))
    assert (out == acc._GUARD).all()


# ---- the other fused path, and the stress ------------------------------------------------------------------------------------
def test_the_fused_form_on_the_vector_alu_gives_the_same_bits():
    """The measurement build serves the fused form on the VALU tile when asked (its own process: the library is chosen at
    import): the golden cases, the zero ties and two lattice windows, against the same oracle."""
    from yams_amd import build as _build
    assert os.path.exists(_build.MEASURE_LIB), "the measurement build is not in the tree (python -m yams_amd.build --measure)"
    env = dict(os.environ, YAMS_ACCEL_MEASURE_LIB="1", YAMS_ACCEL_RERANK_FUSED_PATH="valu")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_rerank_fused_valu.py")], capture_output=True, text=True, timeout=200, env=env)
    assert r.returncode == 0 and "fused on the VALU: OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_stress_harness():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_rerank.py"), "--cases", "60"], capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0 and "60 cases, 0 failures OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
