"""The cluster router's dense signal (yams_route_index_* / yams_route_dense_*, topology_route_v1) without a GPU: the header,
the exports and the bindings agree; the restatement of tests/_route_oracle.py equals what the REFERENCE'S OWN buildRouteIndex
and route return (tests/golden/cluster_route.json, made by tests/golden/make_route_golden.py); the shell
include/yams_accel/topology_route.hpp over a stand-in table equals the same file, also as a stand-alone program under
AddressSanitizer and UBSan."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _route_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "cluster_route.json")
GOLDEN_FILE = json.load(open(GOLDEN_PATH))
GOLDEN = {c["name"]: c for c in GOLDEN_FILE["cases"]}
ENTRIES = ["yams_route_index_create_device", "yams_route_index_create_host", "yams_route_index_info", "yams_route_dense_device",
           "yams_route_dense_host"]
F32 = np.float32


def test_header_exports_and_bindings_agree(accel_lib):
    from yams_amd import _lib
    header = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    for name in ENTRIES:
        assert re.search(r"YAMS_ACCEL_API yams_status_t " + name + r"\(", header), name
        assert name in _lib.EXPORTS and hasattr(accel_lib, name), name
    assert "YAMS_ACCEL_API void yams_route_index_destroy(" in header and hasattr(accel_lib, "yams_route_index_destroy")
    for macro, value in (("YAMS_ROUTE_MAX_DIM", 4096), ("YAMS_ROUTE_MAX_CLUSTERS", 65536), ("YAMS_ROUTE_MAX_REPRESENTATIVES", 64),
                         ("YAMS_ROUTE_MAX_QUERIES", 1024)):
        assert re.search(r"#define %s %du\b" % (macro, value), header), macro
    assert '#define YAMS_IFACE_TOPOLOGY_ROUTE_V1 "topology_route_v1"' in header
    assert C.sizeof(_lib.RouteIndexInfo) == 24 and C.sizeof(_lib.RouteDiag) == 16


def test_interface_table_is_served_at_version_1_only(accel_lib):
    from yams_amd import _lib
    p = C.c_void_p()
    assert accel_lib.yams_plugin_get_interface(b"topology_route_v1", 1, C.byref(p)) == 0 and p.value
    vt = C.cast(p, C.POINTER(_lib.TopologyRouteV1)).contents
    assert vt.abi_version == 1
    for f in ("index_create", "index_info", "dense", "index_destroy"):
        assert getattr(vt, f), f
    for version in (0, 2):
        q = C.c_void_p()
        assert accel_lib.yams_plugin_get_interface(b"topology_route_v1", version, C.byref(q)) != 0 and not q.value
    assert b"topology_route_v1" not in accel_lib.yams_plugin_get_manifest_json()
    if accel_lib.yams_accel_device_count() == 0:      # without a device every door refuses
        out = C.c_uint64(0)
        assert vt.index_create(None, None, 0, 4, None, None, None, 0, C.byref(out), None) == _lib.YAMS_ERR_UNSUPPORTED
        assert vt.dense(None, 1, None, 0, 0, None, None, None, None, None) == _lib.YAMS_ERR_UNSUPPORTED


def test_a_null_handle_is_refused(accel_lib):
    from yams_amd import _lib
    h = C.c_void_p()
    for fn in (accel_lib.yams_route_index_create_device, accel_lib.yams_route_index_create_host):
        assert fn(None, None, 0, 4, None, None, None, 0, C.byref(h), None) == _lib.YAMS_ERR_INVALID_ARG and not h.value
    for fn in (accel_lib.yams_route_dense_device, accel_lib.yams_route_dense_host):
        assert fn(None, None, 0, 0, None, None, None, None, None) == _lib.YAMS_ERR_INVALID_ARG
    assert accel_lib.yams_route_index_info(None, None) == _lib.YAMS_ERR_INVALID_ARG
    accel_lib.yams_route_index_destroy(None)


def test_the_candidate_bitset_layout():
    from yams_amd.accel import pack_candidates
    m = np.zeros((2, 70), bool)
    m[0, [0, 31, 32, 69]] = True
    m[1, 33] = True
    assert pack_candidates(m).tolist() == [[0x80000001, 1, 1 << 5], [0, 2, 0]]
    assert pack_candidates(np.zeros((3, 0), bool)).shape == (3, 0)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_the_golden_file_covers_the_cases_and_stays_small():
    assert list(GOLDEN) == list(ro.GOLDEN_CASES) and len(GOLDEN) >= 25
    assert os.path.getsize(GOLDEN_PATH) < 64 * 1024
    assert GOLDEN_FILE["source"].startswith("SparseGuidedClusterRouter::buildRouteIndex / ::route")
    for name, case in ro.GOLDEN_CASES.items():
        assert GOLDEN[name]["sha256"] == ro.case_digest(case), name      # the file was made from these inputs
    # the cases reach what they are there for
    for name in ("inf_in_query", "inf_in_centroid", "norm_product_zero", "flt_max_quarter"):      # a NaN dense, observed
        assert GOLDEN[name]["routes"][0][1:3] == ["nan", "nan"], name
    only = {r[0]: r for r in GOLDEN["only_nan_representatives"]["routes"]}["c00"]
    assert only[2] == (1.0).hex()                                        # observed, dense 0.0: semanticCost 1.0
    assert GOLDEN["alpha_one_scores_nothing"]["work"]["evaluations"] == 0
    assert all(r[2] is None for r in GOLDEN["alpha_one_scores_nothing"]["routes"])
    z2, z3 = GOLDEN["zero_representative_first_max_2"], GOLDEN["zero_representative_first_max_3"]
    assert z2["work"]["evaluations"] == 3 and z3["work"]["evaluations"] == 6      # the zero-norm place used up the limit of 2
    assert all(r[2] == (0.0).hex() for r in z3["routes"]) and not any(r[2] == (0.0).hex() for r in z2["routes"])
    assert GOLDEN["candidate_mask_weighted_seeds"]["work"]["ann_used"] and GOLDEN["candidate_mask_weighted_seeds"]["work"]["exact_evaluations"] == 16
    tiny = ro.GOLDEN_CASES["norm_product_denormal"]["request"]["query"]
    n = ro.norms(tiny[None, :])[0]
    assert 0 < F32(n * n) < np.finfo(F32).tiny                          # the product of the norms is a denormal
    d = ro.GOLDEN_CASES["dot_denormal"]
    assert 0 < abs(F32(ro.chains(d["request"]["query"][None, :], d["clusters"][0]["centroid"][None, :])[0, 0])) < np.finfo(F32).tiny


@pytest.mark.parametrize("name", list(ro.GOLDEN_CASES))
def test_restatement_equals_the_reference_functions(name):
    case = ro.GOLDEN_CASES[name]
    got = ro.routes_hex(ro.route(case, ro.standin_ann(case)))
    want = GOLDEN[name]
    assert got["routes"] == want["routes"], name
    assert got["work"] == want["work"], name
    assert ro.same_result(got, want), name


@pytest.mark.parametrize("name", list(ro.GOLDEN_CASES))
def test_the_table_form_equals_the_route_loop(name):
    """dense_signal over table_of(...) — what the device serves — gives the dense, observed and count of the whole-route
    restatement (which the test above holds to the reference), the candidate mask included; the scalar form agrees."""
    case = ro.GOLDEN_CASES[name]
    rq = case["request"]
    table = ro.table_of(case["clusters"], rq["query"].size)
    whole = ro.route(case, ro.standin_ann(case))
    if F32(rq["alpha"]) >= 1:
        assert not whole["observed"].any()
        return
    cand = np.array(whole["candidates"], bool)
    dense, obs, ev = ro.dense_signal(table, rq["query"][None, :], rq["max_reps"], cand[None, :])
    assert ro.same_bits(dense[0], whole["dense"]) and (obs[0] == whole["observed"]).all()
    assert int(ev[0]) == whole["work"]["exact_evaluations"]
    d1, o1, e1 = ro.dense_signal_scalar(table, rq["query"], rq["max_reps"], cand)
    assert ro.same_bits(d1, dense[0]) and (o1 == obs[0]).all() and e1 == int(ev[0])


def test_vectorised_and_scalar_restatements_agree_on_seeded_tables():
    rng = np.random.default_rng(3)
    for dim, sizes in ((1, [1, 2, 3]), (33, [1, 0, 4, 65, 2, 64]), (7, [5] * 9)):
        t = ro.random_table(rng, dim, sizes, special=True)
        q = rng.standard_normal((4, dim)).astype(F32)
        q[1, 0] = np.nan
        q[2] = 0.0
        cand = rng.random((4, len(sizes))) < 0.6
        for limit in (0, 1, 2, 4):
            d, o, e = ro.dense_signal(t, q, limit, cand)
            for i in range(4):
                d1, o1, e1 = ro.dense_signal_scalar(t, q[i], limit, cand[i])
                assert ro.same_bits(d[i], d1) and (o[i] == o1).all() and e[i] == e1


def test_the_scans_fp64_cosine_is_not_the_routers():
    """Why the feature exists: the scan's similarity is dot / (|row| * |q|) taken in fp64 and rounded once; the router rounds
    the dot and each norm to float, multiplies the norms in float and divides in float.  On ordinary vectors the mapped
    values differ in their last bit for some pairs (15 of these 400), so a scan corpus of cluster vectors is no drop-in."""
    rng = np.random.default_rng(12)
    v = rng.standard_normal((400, 64)).astype(F32)
    q = rng.standard_normal((1, 64)).astype(F32)
    dot = ro.chains(q, v)
    router = ro.map_cosine(dot, ro.norms(q)[:, None], ro.norms(v)[None, :])
    scan = ro.scan_cosine(dot, ro.chains(q, q)[0, 0], np.array([ro.chains(v[i:i + 1], v[i:i + 1])[0, 0] for i in range(400)])[None, :])
    differ = int((ro.bits(router) != ro.bits(scan)).sum())
    assert differ >= 1, differ
    assert np.abs(router.astype(np.float64) - scan.astype(np.float64)).max() <= 2.0 ** -22      # ... by a few ulps of 0.5


def test_host_side_rules_of_the_table():
    cl = [{"centroid": np.ones(4, F32), "reps": [np.ones(3, F32), np.ones(4, F32), np.zeros(0, F32), 2 * np.ones(4, F32)]},
          {"centroid": np.zeros(0, F32), "reps": [np.ones(4, F32)]}]
    t = ro.table_of(cl, 4)
    assert t.offsets.tolist() == [0, 3, 4] and t.has_centroid.tolist() == [1, 0] and t.position.tolist() == [0, 1, 3, 0]
    cl[1]["centroid"] = np.ones(5, F32)
    assert ro.table_of(cl, 4) is None      # a non-empty centroid of another size: the host runs its own function


# ---- the shell -----------------------------------------------------------------------------------------------------------------
def run_driver(exe, name, *flags):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "case.bin")
        ro.write_case(path, ro.GOLDEN_CASES[name])
        r = subprocess.run([exe, path, *flags], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-1500:])
    return r.stdout


@pytest.mark.parametrize("sanitize", [False, True])
def test_shell_over_a_stand_in_equals_the_golden_file(sanitize):
    """sanitize=True: the stand-alone program under AddressSanitizer and UBSan, on the CPU."""
    from _route_build import build_shell_test
    exe = build_shell_test(sanitize=sanitize)
    for name in ro.GOLDEN_CASES:
        got = ro.parse_driver(run_driver(exe, name))
        assert "error" not in got and ro.same_result(got, GOLDEN[name]), (name, got, GOLDEN[name])


def test_shell_route_batch_equals_single_routes():
    from _route_build import build_shell_test
    exe = build_shell_test()
    for name in ("plain", "candidate_mask_weighted_seeds", "max_representatives_2", "nan_in_query"):
        parts = run_driver(exe, name, "--batch").split("request ")
        answers = [ro.parse_driver(parts[0] + p.split("\n", 1)[1]) for p in parts[1:]]
        assert len(answers) == 3
        assert ro.same_result(answers[0], GOLDEN[name]) and ro.same_result(answers[2], GOLDEN[name]), name
        case = dict(ro.GOLDEN_CASES[name], request=dict(ro.GOLDEN_CASES[name]["request"], max_reps=ro.GOLDEN_CASES[name]["request"]["max_reps"] + 1))
        want = ro.routes_hex(ro.route(case, ro.standin_ann(case)))
        assert ro.same_result(answers[1], want), name


def test_shell_refuses_what_it_cannot_serve_exactly():
    from _route_build import build_shell_test
    exe = build_shell_test()
    base = ro.GOLDEN_CASES["plain"]
    cases = {"centroid": dict(base, clusters=[dict(c) for c in base["clusters"]]), "query": dict(base, request=dict(base["request"]))}
    cases["centroid"]["clusters"][2]["centroid"] = np.ones(5, F32)
    cases["query"]["request"]["query"] = np.ones(9, F32)
    for what, case in cases.items():
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "case.bin")
            ro.write_case(path, case)
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "error" in r.stdout and "another size" in r.stdout, (what, r.stdout)
        assert not any(line.startswith(("route ", "work ")) for line in r.stdout.splitlines()), (what, r.stdout)


def test_stress_dry_run_and_self_test():
    for flag in ("--dry-run", "--self-test"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_route.py"), flag], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
