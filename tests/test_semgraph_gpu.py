"""The semantic-neighbour graph on the GPU (yams_graph_semantic_neighbors_device / _host, semantic_graph_v1) against the
restatement of tests/_semgraph_oracle.py and the reference's own loop (tests/golden/semantic_neighbors.json).  Every
comparison is on bits — neighbour rows, similarity bits, counts, inverse-norm bits, pairs_scored, pairs_admitted — and nothing
is compared within a tolerance.  pairs_scored is the check that catches a pair scored twice or not at all at a tile edge: the
top-K alone would not."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import _semgraph_oracle as so

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "semantic_neighbors.json")))["cases"]}
CASES = so.golden_cases()
SENTINEL = 0xA5


def same(got, want):
    """(rows, sims, counts, inv, diag) of the wrapper against the oracle's dict, bit for bit; returns what differs."""
    g_rows, g_sims, g_counts, g_inv, diag = got
    bad = []
    if not np.array_equal(g_counts, want["counts"]):
        bad.append(("counts", int((g_counts != want["counts"]).sum())))
    if not np.array_equal(g_rows, want["rows"]):
        bad.append(("rows", np.argwhere(g_rows != want["rows"])[:4].tolist()))
    if not np.array_equal(so.bits(g_sims), so.bits(want["sims"])):
        bad.append(("sims", np.argwhere(so.bits(g_sims) != so.bits(want["sims"]))[:4].tolist()))
    if not np.array_equal(so.bits(g_inv), so.bits(want["inv"])):
        bad.append(("inv", int((so.bits(g_inv) != so.bits(want["inv"])).sum())))
    if (diag["pairs_scored"], diag["pairs_admitted"]) != (want["pairs_scored"], want["pairs_admitted"]):
        bad.append(("pairs", diag["pairs_scored"], want["pairs_scored"], diag["pairs_admitted"], want["pairs_admitted"]))
    return bad


def check(acc, x, k, tie_rank=None, source_rows=None, threshold=None, host_entry=False, want=None):
    want = want or so.neighbors(x, k, tie_rank, source_rows, threshold)
    got = acc.semantic_neighbors(x, k, tie_rank=tie_rank, source_rows=source_rows, threshold=threshold, host_entry=host_entry)
    bad = same(got, want)
    assert not bad, bad
    return got[4], want


@pytest.fixture(scope="module")
def vtable():
    from yams_amd import _lib
    L = _lib.load()
    assert L.yams_plugin_init(b'{"device":0}', None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"semantic_graph_v1", 1, C.byref(p)) == 0
    yield C.cast(p, C.POINTER(_lib.SemanticGraphV1)).contents
    L.yams_plugin_shutdown()


def through_vtable(vt, x, k, tie_rank=None, source_rows=None, threshold=None):
    """One semantic_graph_v1.neighbors call; returns (status, (rows, sims, counts, inv, diag) or None)."""
    from yams_amd import _lib
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    tr = None if tie_rank is None else np.ascontiguousarray(tie_rank, np.uint32)
    sr = None if source_rows is None else np.ascontiguousarray(source_rows, np.uint32)
    S = n if sr is None else len(sr)
    pr = _lib.u32p(); ps = _lib.f32p(); pc = _lib.u32p(); pi = _lib.f32p(); diag = _lib.GraphDiag()
    st = vt.neighbors(None, x.ctypes.data_as(_lib.f32p), n, dim, tr.ctypes.data_as(_lib.u32p) if tr is not None else None,
                      sr.ctypes.data_as(_lib.u32p) if sr is not None else None, S, k, 0 if threshold is None else 1,
                      0.0 if threshold is None else threshold, C.byref(pr), C.byref(ps), C.byref(pc), C.byref(pi), C.byref(diag))
    if st != 0:
        assert not pr and not ps and not pc and not pi
        return st, None
    out = (np.ctypeslib.as_array(pr, (S, k)).copy(), np.ctypeslib.as_array(ps, (S, k)).copy(), np.ctypeslib.as_array(pc, (S,)).copy(),
           np.ctypeslib.as_array(pi, (n,)).copy(), diag.as_dict())
    vt.free_neighbors(None, pr, ps, pc, pi)
    return 0, out


def golden_want(name):
    """The golden record of a case in the oracle's shape: what the reference's own loop produced."""
    c, v = GOLDEN[name], CASES[name]
    n = len(v["rows"])
    src = list(range(n)) if v["sources"] is None else v["sources"]
    rows = np.full((len(src), v["k"]), so.EMPTY_ROW, np.uint32)
    sims = np.full((len(src), v["k"]), -np.inf, np.float32)
    counts = np.zeros(len(src), np.uint32)
    for i, s in enumerate(src):
        lst = c["neighbors"].get(str(s), [])
        counts[i] = len(lst)
        for j, (r, b) in enumerate(lst):
            rows[i, j] = r
            sims[i, j] = so.f32([b])[0]
    return dict(rows=rows, sims=sims, counts=counts, inv=so.f32(c["inv_bits"]), pairs_scored=c["pairs_scored"], pairs_admitted=c["pairs_admitted"])


# ---- the golden cases through the three doors -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases_equal_the_reference_loop(acc, vtable, name):
    v = CASES[name]
    want = golden_want(name)
    rank = so.rank_of_hashes(v["hashes"])
    check(acc, v["rows"], v["k"], rank, v["sources"], v["threshold"], want=want)
    check(acc, v["rows"], v["k"], rank, v["sources"], v["threshold"], host_entry=True, want=want)
    st, got = through_vtable(vtable, v["rows"], v["k"], rank, v["sources"], v["threshold"])
    assert st == 0 and not same(got, want), same(got, want)


# ---- tile edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 127, 128, 129, 191, 193])
def test_row_counts_around_the_tile_edges(acc, n):
    x = so.uniform_rows(n, n, 7)
    if n > 100:
        x[n - 1] = x[0]; x[64] = 0.0
    diag, want = check(acc, x, 8)
    assert want["pairs_scored"] == (n - (n > 100)) * (n - (n > 100) - 1) and diag["stripes"] == 1


@pytest.mark.parametrize("n_sources", [1, 127, 129])
def test_source_lists_unordered_and_repeated(acc, n_sources):
    n = 150
    x = so.clustered_rows(n_sources, n, 9)
    x[77] = 0.0
    rng = np.random.default_rng(n_sources)
    src = rng.integers(0, n, n_sources).astype(np.uint32)        # unordered, with repeats
    src[0] = n - 1
    if n_sources > 1:
        src[1] = 77; src[-1] = src[2]
        assert len(set(src.tolist())) < n_sources
    check(acc, x, 8, so.shuffled_rank(5, n), src)
    check(acc, x, 8, None, src, host_entry=True)


@pytest.mark.parametrize("dim", [1, 5, 7, 8, 9, 33, 383, 384, 4095, 4096])
def test_dimensions_around_the_chunk_and_the_limit(acc, dim):
    n = 130 if dim >= 4095 else 70
    x = so.uniform_rows(dim, n, dim)
    x[3] = x[n - 1]
    diag, want = check(acc, x, 8)
    assert want["pairs_scored"] == n * (n - 1)


# ---- best-K -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8, 63, 64])
def test_list_sizes(acc, k):
    x = so.clustered_rows(k, 200, 6)
    _, want = check(acc, x, k, so.shuffled_rank(k, 200), threshold=-1.0)
    assert (want["counts"] == k).all()                            # threshold -1: every pair admitted, every list full


def test_k_above_the_number_of_candidates(acc):
    x = so.uniform_rows(20, 20, 5)
    _, want = check(acc, x, 30, threshold=-1.0)
    assert (want["counts"] == 19).all()


@pytest.mark.parametrize("with_rank", [True, False])
def test_the_cut_at_k_goes_through_a_plateau(acc, with_rank):
    base = so.uniform_rows(40, 5, 12)
    x = np.tile(base, (40, 1))                                     # 40 copies of 5 distinct rows
    rank = so.shuffled_rank(41, 200) if with_rank else None
    deeper = so.neighbors(x, 9, rank)
    assert (so.bits(deeper["sims"][:, 7]) == so.bits(deeper["sims"][:, 8])).all()      # the 8th and the 9th best tie: the rank cuts
    if with_rank:
        assert not np.array_equal(deeper["rows"], so.neighbors(x, 9)["rows"])          # ... and not as row order would
    check(acc, x, 8, rank)


# ---- stripes ----------------------------------------------------------------------------------------------------------------
def test_a_shape_the_stripe_rule_splits(acc):
    n, dim = 6000, 32
    x = so.uniform_rows(6000, n, dim)
    src = np.arange(100, 164, dtype=np.uint32)
    x[5] = (np.float32(2.0) * x[100]).astype(np.float32)          # a best row in the first candidate stripe ...
    x[n - 1] = (np.float32(4.0) * x[100]).astype(np.float32)      # ... and in the last
    diag, want = check(acc, x, 8, so.shuffled_rank(6, n), src)
    assert diag["stripes"] > 1 and diag["source_tiles"] == 1
    assert set(want["rows"][0, :2].tolist()) == {5, n - 1}
    diag, _ = check(acc, x, 64, None, src, threshold=-1.0)
    assert diag["stripes"] > 1


def test_a_shape_the_stripe_rule_does_not_split(acc):
    x = so.uniform_rows(300, 300, 32)
    diag, _ = check(acc, x, 8)
    assert diag["stripes"] == 1 and diag["source_tiles"] == 3


# ---- admission --------------------------------------------------------------------------------------------------------------
def admission_rows():
    """140 rows of dim 2 around the special rows of the golden cases, so that they meet across tile borders."""
    x = so.uniform_rows(140, 140, 2)
    x[::9] = [1, 0]; x[1::9] = [0, 1]; x[2::9] = [-1, 0]                         # exactly-zero and negative cosines
    x[3::9] = [np.float32(1e-40), 1e10]; x[4::9] = [np.float32(-1e-40), 1e10]    # +0.0 and -0.0 from underflow
    x[5::18] = [np.float32(1e-40), 1]                                            # a positive denormal cosine against (1, 0)
    q = so.FLT_MAX / np.float32(4)
    x[6::18] = [q, -q]                                                           # a denormal inverse norm
    x[139] = 0.0
    return x


@pytest.mark.parametrize("threshold", [None, 0.0, 0.5, 1.0])
def test_admission_modes(acc, threshold):
    x = admission_rows()
    _, want = check(acc, x, 64, so.shuffled_rank(3, 140), threshold=threshold)
    kept = want["sims"][want["rows"] != so.EMPTY_ROW]
    if threshold is None:
        assert (kept > 0).all() and ((kept > 0) & (kept < np.float32(1.2e-38))).any()          # a denormal cosine is kept
    elif threshold == 0.0:
        assert ((kept == 0) & np.signbit(kept)).any() and ((kept == 0) & ~np.signbit(kept)).any()   # both zeros stay, each with its sign
    inv = want["inv"]
    assert ((inv > 0) & (inv < np.float32(1.2e-38))).any() and (inv == 0).any()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _out(acc, nbytes, shift=4, tail=64):
    buf = acc.to_device(np.full(shift + nbytes + tail, SENTINEL, np.uint8))
    return buf, buf.ptr + shift


def raw_call(acc, x, k, src=None, rank=None, shift=0):
    """The device entry over sentinel-filled outputs that start 4 bytes into their allocations (rows `shift` bytes into theirs).
    Returns (status, every output allocation's bytes, diag)."""
    from yams_amd import _lib
    n, dim = x.shape
    S = n if src is None else len(src)
    img = np.full(shift + x.nbytes + 64, SENTINEL, np.uint8)
    img[shift:shift + x.nbytes] = x.view(np.uint8).reshape(-1)
    bufs = [acc.to_device(img)]
    try:
        d_src = d_rank = None
        if src is not None:
            d_src = acc.to_device(np.ascontiguousarray(src, np.uint32)); bufs.append(d_src)
        if rank is not None:
            d_rank = acc.to_device(np.ascontiguousarray(rank, np.uint32)); bufs.append(d_rank)
        sizes = [S * k * 4, S * k * 4, S * 4, n * 4]
        outs = [_out(acc, sz) for sz in sizes]
        bufs += [b for b, _ in outs]
        diag = _lib.GraphDiag()
        st = acc.L.yams_graph_semantic_neighbors_device(acc.ctx, bufs[0].ptr + shift, n, dim, d_rank.ptr if d_rank else None,
                                                        d_src.ptr if d_src else None, S, k, 0, 0.0, outs[0][1], outs[1][1], outs[2][1],
                                                        outs[3][1], C.byref(diag))
        raws = [b.download(np.uint8, b.nbytes) for b, _ in outs]
    finally:
        for b in bufs:
            b.free()
    return st, raws, sizes, diag.as_dict()


@pytest.mark.parametrize("what", ["nan", "inf", "all_denormal", "source_index", "tie_rank_repeats", "tie_rank_range"])
def test_refusals_write_nothing(acc, what):
    from yams_amd import _lib
    n = 300
    x = so.uniform_rows(300, n, 6)
    src = rank = None
    if what == "nan":
        x[299, 5] = np.nan
    elif what == "inf":
        x[128, 0] = -np.inf
    elif what == "all_denormal":
        x[200] = np.float32(1e-40)                                  # norm = 6e-80: its float inverse is +inf
        with pytest.raises(so.InvalidArg):
            so.inverse_norms(x)
    elif what == "source_index":
        src = np.array([0, 5, n, 7], np.uint32)
    elif what == "tie_rank_repeats":
        rank = so.shuffled_rank(1, n); rank[17] = rank[250]
    else:
        rank = so.shuffled_rank(1, n); rank[17] = n
    st, raws, _, diag = raw_call(acc, x, 8, src, rank)
    assert st == _lib.YAMS_ERR_INVALID_ARG
    for raw in raws:
        assert (raw == SENTINEL).all()                              # nothing written: not the outputs, not the bytes around them
    assert diag == dict(stripes=0, source_tiles=0, pairs_scored=0, pairs_admitted=0)
    if what in ("nan", "inf", "all_denormal"):
        with pytest.raises(_lib.AccelError) as e:
            acc.semantic_neighbors(x, 8, host_entry=True)
        assert e.value.status == _lib.YAMS_ERR_INVALID_ARG


def test_limits_and_empty_results(acc):
    from yams_amd import _lib
    x = so.uniform_rows(1, 10, 4)
    with pytest.raises(_lib.AccelError) as e:
        acc.semantic_neighbors(x, 65)
    assert e.value.status == _lib.YAMS_ERR_UNSUPPORTED
    with pytest.raises(_lib.AccelError) as e:
        acc.semantic_neighbors(x, 8, threshold=float("nan"))
    assert e.value.status == _lib.YAMS_ERR_INVALID_ARG
    r = acc.semantic_neighbors(x, 0)
    assert r[0].shape == (10, 0) and r[4]["pairs_scored"] == 0
    r = acc.semantic_neighbors(x[:1], 8)
    assert r[2].tolist() == [0] and (r[0] == so.EMPTY_ROW).all()


# ---- bases and reuse --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [8, 64])
@pytest.mark.parametrize("shift", [4, 8])
def test_float_aligned_device_bases(acc, dim, shift):
    """The header promises float alignment only: rows 4 / 8 bytes into an allocation take the scalar staging although
    dim % 4 == 0; every output lands 4 bytes into its allocation and the bytes around it stay as they were."""
    n, k = 193, 8
    x = so.clustered_rows(dim + shift, n, dim)
    want = so.neighbors(x, k)
    st, raws, sizes, diag = raw_call(acc, x, k, shift=shift)
    assert st == 0
    outs = []
    for raw, sz in zip(raws, sizes):
        assert (raw[:4] == SENTINEL).all() and (raw[4 + sz:] == SENTINEL).all(), "wrote outside the output range"
        outs.append(raw[4:4 + sz].copy())
    got = (outs[0].view(np.uint32).reshape(n, k), outs[1].view(np.float32).reshape(n, k), outs[2].view(np.uint32), outs[3].view(np.float32), diag)
    assert not same(got, want), same(got, want)


def test_workspace_reuse_large_small_large(acc):
    large = so.clustered_rows(71, 1500, 24)
    small = so.uniform_rows(72, 9, 3)
    rank = so.shuffled_rank(7, 1500)
    check(acc, large, 16, rank)
    check(acc, small, 2)
    check(acc, large, 16, rank)
    check(acc, large[:700], 64, None, np.arange(699, -1, -7, dtype=np.uint32), threshold=0.25)


def test_concurrent_callers_of_the_vtable(vtable):
    """Four host threads in semantic_graph_v1 at once: every call leases a work context with its own workspace."""
    shapes = [(300, 8, 8, None), (700, 33, 4, 0.2), (150, 64, 64, -1.0), (1100, 5, 1, None)]
    inputs = []
    for t, (n, dim, k, thr) in enumerate(shapes):
        x = so.clustered_rows(200 + t, n, dim)
        x[n // 2] = x[1]
        rank = so.shuffled_rank(t, n)
        inputs.append((x, k, rank, thr, so.neighbors(x, k, rank, None, thr)))
    failures = []
    start = threading.Barrier(len(shapes))

    def worker(t):
        x, k, rank, thr, want = inputs[t]
        try:
            start.wait(timeout=60)
            for rnd in range(3):
                st, got = through_vtable(vtable, x, k, rank, None, thr)
                if st != 0 or same(got, want):
                    failures.append((t, rnd, st, same(got, want) if got else None)); return
        except Exception as e:                                      # (a thread's exception must reach the test)
            failures.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(len(shapes))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not failures, failures


def test_semantic_graph_adapter_against_the_reference_loop():
    """tests/cpp/semgraph_test.cpp: AccelSemanticGraph::build (the shell over semantic_graph_v1) on the golden cases."""
    from test_semgraph_cpu import build_semgraph_test, write_adapter_cases
    from yams_amd import build as b
    r = subprocess.run([build_semgraph_test(), write_adapter_cases(), b.LIB], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_stress_harness_on_the_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_semgraph.py"), "--cases", "150", "--seed", "1"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mode"] == "device" and res["cases"] == 150 and res["skipped"] == 0
