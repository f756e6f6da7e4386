"""SGC smoothing on the device (yams_graph_sgc_smooth_device / _host, topology_smooth_v1) without a GPU: the numpy restatement
equals, bit for bit, what the reference's own applySGCSmoothing produced on every golden case (tests/golden/sgc.json); the
edge cases reach the path they are there for; the seeded cases are sensitive to the order of a row's list; header, exports and
the index agree; the interface table is served and absent from the manifest; the argument checks that need no device answer as
documented; the stress harness draws its cases and its comparison tells a flipped bit.  The only tolerance anywhere: a NaN
matches any NaN."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _sgc_oracle as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "sgc.json")
GOLDEN = {c["name"]: c for c in json.load(open(GOLDEN_PATH))["cases"]}
SEEDED = [(21, 400, 37, 8), (22, 257, 64, 12), (23, 300, 1, 6)]


def golden_lists(c):
    return np.array(c["row_offsets"], np.uint64), np.array(c["cols"], np.uint32), sg.f32(np.array(c["weights_bits"], np.uint32))


def lists_of(name):
    return golden_lists(GOLDEN[name])


# ---- the restatement against the reference's own function ------------------------------------------------------------------------
def test_the_golden_file_covers_the_cases_and_stays_small():
    assert set(GOLDEN) == set(sg.GOLDEN_CASES) and len(GOLDEN) >= 12
    assert os.path.getsize(GOLDEN_PATH) < 256 * 1024
    for name, (make, min_edge, reciprocal_only, hops) in sg.GOLDEN_CASES.items():
        c, docs = GOLDEN[name], make()
        assert c["sha256"] == sg.docs_digest(docs), name                     # the recipe still gives the recorded bits
        assert (c["min_edge_score"], c["reciprocal_only"], c["hops"], c["n"]) == (min_edge, reciprocal_only, hops, len(docs))
        if "docs" in c:
            assert [d["emb_bits"] for d in c["docs"]] == [sg.bits(d["emb"]).tolist() for d in docs], name
            assert [d["hash"] for d in c["docs"]] == [d["hash"] for d in docs]


@pytest.mark.parametrize("name", sorted(sg.GOLDEN_CASES))
def test_oracle_equals_the_reference_function_bit_for_bit(name):
    c = GOLDEN[name]
    docs = sg.GOLDEN_CASES[name][0]()
    off, cols, w = golden_lists(c)
    embs = sg.apply_to_docs(docs, off, cols, w, c["hops"])
    assert sg.embeddings_digest(embs) == c["out_sha256"], name
    if "out_bits" in c:
        assert [sg.bits(e).tolist() for e in embs] == c["out_bits"], name


def test_the_cases_reach_the_edges_they_are_there_for():
    # hops == 0 changes nothing; ragged: rows of another size keep their bits and their size
    c = GOLDEN["two_clusters_hops0"]
    assert c["out_bits"] == [d["emb_bits"] for d in c["docs"]]
    c = GOLDEN["ragged_hops3"]
    assert [len(o) for o in c["out_bits"]] == [3, 0, 2, 3, 3, 3, 1]
    assert c["out_bits"][2] == c["docs"][2]["emb_bits"] and c["out_bits"][6] == c["docs"][6]["emb_bits"]
    assert c["out_bits"][0] != c["docs"][0]["emb_bits"]
    # ... and the row of another size stays in the matrix as zeros: rows 0's list still names 1 and 2
    off, cols, _ = golden_lists(c)
    assert sorted(cols[int(off[0]):int(off[1])].tolist()) == [1, 2]
    # duplicate hashes: the later document (2) takes the edges meant for "a"; document 0 keeps only what it sends itself
    off, cols, _ = lists_of("duplicate_hashes")
    assert 2 in cols[int(off[1]):int(off[2])].tolist() and 2 in cols[int(off[3]):int(off[4])].tolist()
    # reciprocalOnly: fewer edges with it than without
    assert len(GOLDEN["reciprocal_only"]["cols"]) < len(GOLDEN["reciprocal_off"]["cols"])
    # minEdgeScore at a score's exact value: the 0.5 pair (p, s) stays, the 0.49999997 pair (r, s) goes
    off, cols, w = lists_of("min_edge_at_a_score")
    row = lambda i: dict(zip(cols[int(off[i]):int(off[i + 1])].tolist(), w[int(off[i]):int(off[i + 1])].tolist()))
    assert row(3) == {0: 0.5} and 3 not in row(2)
    assert 0.5 in lists_of("reciprocal_off")[2] and np.float32(0.49999997) in lists_of("reciprocal_off")[2]
    # a NaN score becomes weight 0 (and the pair is there)
    off, cols, w = lists_of("nan_score")
    assert sorted(zip(cols[:int(off[1])].tolist(), w[:int(off[1])].tolist())) == [(1, 0.0), (2, 0.5)]
    # a pair seen from both sides: the larger weight, on both rows
    off, cols, w = lists_of("two_sided_scores")
    assert dict(zip(cols[:int(off[1])].tolist(), w[:int(off[1])].tolist())) == {1: 0.75}
    assert dict(zip(cols[int(off[1]):int(off[2])].tolist(), w[int(off[1]):int(off[2])].tolist())) == {0: 0.75, 2: np.float32(0.6)}


@pytest.mark.parametrize("name", ["zero_weight_beside_negative_zero", "nan_score"])
def test_the_zero_scale_skip_is_reached_and_changes_a_sign_bit(name):
    c = GOLDEN[name]
    docs = sg.GOLDEN_CASES[name][0]()
    off, cols, w = golden_lists(c)
    x, _ = sg.feature_matrix(docs)
    y, diag = sg.smooth(x, off, cols, w, c["hops"], with_diag=True)
    assert diag["edges_skipped_zero_scale"] > 0
    wrong = sg.smooth(x, off, cols, w, c["hops"], skip_zero_scale=False)
    differ = sg.bits(y) != sg.bits(wrong)
    assert differ.any() and (sg.bits(y)[differ] == 0x80000000).all() and (sg.bits(wrong)[differ] == 0).all()
    assert [sg.bits(e).tolist() for e in sg.apply_to_docs(docs, off, cols, w, c["hops"])] == c["out_bits"]      # the reference skips


@pytest.mark.parametrize("seed,n,dim,deg", SEEDED)
def test_sorting_a_rows_list_changes_output_bits(seed, n, dim, deg):
    x, off, cols, w = sg.seeded_case(seed, n, dim, deg, specials=False)
    y = sg.smooth(x, off, cols, w, 2)
    cs, ws = sg.sort_rows(off, cols, w)
    assert not np.array_equal(cs, cols)
    assert (sg.bits(sg.smooth(x, off, cs, ws, 2)) != sg.bits(y)).any()      # the cases are sensitive to the order


def test_golden_lists_are_order_sensitive_too():
    for name in ("seeded_300x37", "seeded_200x64_all_edges"):
        c = GOLDEN[name]
        docs = sg.GOLDEN_CASES[name][0]()
        off, cols, w = golden_lists(c)
        cs, ws = sg.sort_rows(off, cols, w)
        assert sg.embeddings_digest(sg.apply_to_docs(docs, off, cs, ws, c["hops"])) != c["out_sha256"], name


def test_properties_of_the_restatement():
    x, off, cols, w = sg.seeded_case(5, 50, 7, 5)
    assert sg.same_bits(sg.smooth(x, off, cols, w, 0), x)
    y = sg.smooth(x, off, cols, w, 1)
    empty = np.nonzero(np.diff(off.astype(np.int64)) == 0)[0]
    assert len(empty) and sg.same_bits(y[empty], x[empty])                 # no edges: inv^2 == 1, the row keeps its bits
    assert sg.same_bits(sg.smooth(y, off, cols, w, 1), sg.smooth(x, off, cols, w, 2))
    big = np.full((2, 1), sg.FLT_MAX, np.float32)
    with np.errstate(all="ignore"):
        o = sg.smooth(big, np.array([0, 3, 3], np.uint64), np.array([1, 1, 1], np.uint32), np.ones(3, np.float32), 1)
    assert np.isposinf(o[0, 0]) and o[1, 0] == sg.FLT_MAX                  # an overflow inside the hops is served, not refused
    for bad in (np.nan, np.inf, -np.inf):
        z = x.copy(); z[3, 2] = bad
        with pytest.raises(sg.InvalidArg):
            sg.smooth(z, off, cols, w, 1)
    for bad_w in (-1.0, np.nan, np.inf):
        ww = w.copy(); ww[0] = bad_w
        with pytest.raises(sg.InvalidArg):
            sg.smooth(x, off, cols, ww, 1)
    cc = cols.copy(); cc[0] = 50
    with pytest.raises(sg.InvalidArg):
        sg.smooth(x, off, cc, w, 1)
    oo = off.copy(); oo[3] = oo[4] + 1
    with pytest.raises(sg.InvalidArg):
        sg.smooth(x, oo, cols, w, 1)


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_indexed(accel_lib):
    from yams_amd import _lib
    header = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    index = doc[doc.index("## 8. Index of the flat C ABI"):]
    for s in ("yams_graph_sgc_smooth_device", "yams_graph_sgc_smooth_host"):
        assert hasattr(accel_lib, s) and s in _lib.EXPORTS and re.search(r"YAMS_ACCEL_API yams_status_t %s\(" % s, header), s
    assert "yams_graph_sgc_smooth_device / _host" in index
    assert "#define YAMS_SGC_MAX_DIM %du" % _lib.SGC_MAX_DIM in header and "#define YAMS_SGC_HUB_DEGREE %du" % _lib.SGC_HUB_DEGREE in header
    assert (_lib.SGC_MAX_DIM, _lib.SGC_HUB_DEGREE) == (sg.MAX_DIM, sg.HUB_DEGREE)
    assert C.sizeof(_lib.SgcDiag) == 32
    for line in (":23-179", ":114-125", ":140-161", ":60-84", ":86-112", ":130-137", ":163-168"):      # the contract names its lines
        assert line in header, line
    shell = open(os.path.join(ROOT, "include", "yams_accel", "topology_sgc.hpp")).read()
    assert "PROPERTY OF THE HOST'S STANDARD LIBRARY" in shell and "std::unordered_map<std::uint64_t, float>" in shell and "reserve(n * 4)" in shell


def test_topology_smooth_interface_and_refusal_without_a_gpu(accel_lib):
    from yams_amd import _lib
    L = accel_lib
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"topology_smooth_v1", 1, C.byref(p)) == 0
    vt = C.cast(p, C.POINTER(_lib.TopologySmoothV1)).contents
    assert vt.abi_version == 1
    for fname, _ in _lib.TopologySmoothV1._fields_[2:]:
        assert getattr(vt, fname), f"topology_smooth_v1.{fname} is NULL"
    for ver in (0, 2):
        q = C.c_void_p()
        assert L.yams_plugin_get_interface(b"topology_smooth_v1", ver, C.byref(q)) == -2      # NOT_FOUND
        assert q.value is None
    m = json.loads(L.yams_plugin_get_manifest_json())                      # the manifest is unchanged
    assert {(i["id"], i["version"]) for i in m["interfaces"]} == {("vector_scan_v1", 1), ("content_hash_v1", 1), ("chunker_v1", 3)}
    if L.yams_accel_device_count() > 0:
        return                                                             # the refusal below is what a CPU-only host sees
    L.yams_plugin_shutdown()
    assert L.yams_plugin_init(b"{}", None) == -3
    x = np.ones((4, 3), np.float32); out = np.full((4, 3), 7.0, np.float32)
    off = np.zeros(5, np.uint64)
    st = vt.smooth(None, x.ctypes.data_as(_lib.f32p), 4, 3, off.ctypes.data_as(_lib.u64p), None, None, 1, out.ctypes.data_as(_lib.f32p), None)
    assert st == _lib.YAMS_ERR_UNSUPPORTED and (out == 7.0).all()          # it refuses, it does not fall back


def test_argument_validation_that_needs_no_device(accel_lib):
    """The checks in front of the first device call.  A context needs a device, so without one only the null-context refusals
    run."""
    from yams_amd import _lib
    L = accel_lib
    x = np.ones((4, 3), np.float32); out = np.zeros((4, 3), np.float32); off = np.zeros(5, np.uint64)
    for fn in (L.yams_graph_sgc_smooth_device, L.yams_graph_sgc_smooth_host):
        assert fn(None, x.ctypes.data, 4, 3, off.ctypes.data, None, None, 1, out.ctypes.data, None) == _lib.YAMS_ERR_INVALID_ARG
    if L.yams_accel_device_count() <= 0:
        return
    ctx = C.c_void_p()
    assert L.yams_accel_ctx_create(0, None, C.byref(ctx)) == 0
    try:
        for fn in (L.yams_graph_sgc_smooth_device, L.yams_graph_sgc_smooth_host):
            diag = _lib.SgcDiag(9, 9, 9, 9, 9, 9)
            call = lambda rows, n, dim, o=off.ctypes.data, dst=out.ctypes.data: fn(ctx, rows, n, dim, o, None, None, 1, dst, C.byref(diag))
            assert call(None, 0, 3) == _lib.YAMS_OK and diag.as_dict() == dict(nnz=0, edges_skipped_zero_scale=0, max_degree=0, hops=0, hub_rows=0)
            assert call(x.ctypes.data, 4, 0) == _lib.YAMS_ERR_INVALID_ARG     # dim == 0
            assert call(None, 4, 3) == _lib.YAMS_ERR_INVALID_ARG              # null rows
            assert call(x.ctypes.data, 4, 3, dst=None) == _lib.YAMS_ERR_INVALID_ARG
            assert call(x.ctypes.data, 4, 3, o=None) == _lib.YAMS_ERR_INVALID_ARG
            assert call(x.ctypes.data, 4, 3, dst=x.ctypes.data + 8) == _lib.YAMS_ERR_INVALID_ARG      # out overlaps rows
            assert call(x.ctypes.data, 4, _lib.SGC_MAX_DIM + 1) == _lib.YAMS_ERR_UNSUPPORTED
            assert call(x.ctypes.data, 1 << 31, 3) == _lib.YAMS_ERR_UNSUPPORTED
    finally:
        L.yams_accel_ctx_destroy(ctx)


# ---- the harness ---------------------------------------------------------------------------------------------------------------
def test_stress_harness_dry_run_and_self_test():
    script = os.path.join(ROOT, "tests", "stress_sgc.py")
    r = subprocess.run([sys.executable, script, "--dry-run", "--cases", "60", "--seed", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mode"] == "dry-run" and res["cases"] == 60
    assert all(v > 0 for v in res["paths"].values()), res["paths"]          # every path the harness names is drawn
    r = subprocess.run([sys.executable, script, "--self-test"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1]) == {"mode": "self-test", "ok": True}, r.stdout + r.stderr
