"""The cluster artifacts (yams_cluster_centroids / _representatives / _residuals, topology_artifacts_v1) without a GPU: the
symbols and the interface table exist, versions 0 and 2 are NOT_FOUND, the argument checks that need no device answer as
documented, and the restatement of tests/_artifacts_oracle.py holds its own properties: its fma is exact, its two residual
forms differ, its centroid keeps the order of the member list, its selection breaks ties towards the first candidate; the
restatement equals what the reference's own functions returned (tests/golden/cluster_artifacts.json), and so does the shell
include/yams_accel/topology_artifacts.hpp over a stand-in table, also as a stand-alone program under ASan and UBSan; the stress
harness draws its cases and its comparison tells a flipped bit."""
import ctypes as C
import math
import os
import random
import re
import struct
from fractions import Fraction

import numpy as np

import _artifacts_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["yams_cluster_centroids_device", "yams_cluster_centroids_host", "yams_cluster_representatives_device",
           "yams_cluster_representatives_host", "yams_cluster_residuals_device", "yams_cluster_residuals_host"]


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_bindings_agree(accel_lib):
    from yams_amd import _lib
    header = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    for name in ENTRIES:
        assert re.search(r"YAMS_ACCEL_API yams_status_t " + name + r"\(", header), name
        assert name in _lib.EXPORTS and hasattr(accel_lib, name), name
    for macro, value in (("YAMS_CLUSTER_MAX_REPRESENTATIVES", _lib.CLUSTER_MAX_REPRESENTATIVES), ("YAMS_RESIDUAL_SEPARATE", _lib.RESIDUAL_SEPARATE),
                         ("YAMS_RESIDUAL_FUSED", _lib.RESIDUAL_FUSED), ("YAMS_CLUSTER_NONE", _lib.CLUSTER_NONE)):
        m = re.search(r"#define " + macro + r" (0x[0-9a-fA-F]+|\d+)u", header)
        assert m and int(m.group(1), 0) == value, macro
    assert (ao.MAX_REPRESENTATIVES, ao.SEPARATE, ao.FUSED, ao.NONE) == (64, _lib.RESIDUAL_SEPARATE, _lib.RESIDUAL_FUSED, _lib.CLUSTER_NONE)
    assert '#define YAMS_IFACE_TOPOLOGY_ARTIFACTS_V1 "topology_artifacts_v1"' in header
    assert "#define YAMS_IFACE_TOPOLOGY_CLUSTER_V1_VERSION 1u" in header      # the k-means table stays at version 1


def test_interface_table_is_served_at_version_1_only(accel_lib):
    from yams_amd import _lib
    p = C.c_void_p()
    assert accel_lib.yams_plugin_get_interface(b"topology_artifacts_v1", 1, C.byref(p)) == 0 and p.value
    vt = C.cast(p, C.POINTER(_lib.TopologyArtifactsV1)).contents
    assert vt.abi_version == 1
    for f in ("centroids", "representatives", "residuals", "free_centroids", "free_representatives", "free_residuals"):
        assert C.cast(getattr(vt, f), C.c_void_p).value, f
    for version in (0, 2):
        q = C.c_void_p(1)
        assert accel_lib.yams_plugin_get_interface(b"topology_artifacts_v1", version, C.byref(q)) != 0 and not q.value
    assert b"topology_artifacts_v1" not in accel_lib.yams_plugin_get_manifest_json()
    # not initialised: the entries refuse instead of touching a device
    out1, out2 = _lib.f32p(), _lib.u32p()
    assert vt.centroids(None, None, 0, 4, None, None, 0, C.byref(out1), C.byref(out2)) != 0


def test_a_null_context_is_refused(accel_lib):
    from yams_amd import _lib
    assert accel_lib.yams_cluster_centroids_device(None, None, 0, 4, None, None, 0, None, None) == _lib.YAMS_ERR_INVALID_ARG
    assert accel_lib.yams_cluster_representatives_host(None, None, 0, 4, None, None, None, None, 0, 1, None, None) == _lib.YAMS_ERR_INVALID_ARG
    assert accel_lib.yams_cluster_residuals_host(None, None, 0, 4, None, 0, None, None, None, 0, None, None, None) == _lib.YAMS_ERR_INVALID_ARG


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_the_oracles_fma_is_exact():
    rng = random.Random(1)

    def draw():
        if rng.random() < 0.1:
            return rng.choice([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308])
        return struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
    checked = 0
    for _ in range(20000):
        a, b, c = draw(), draw(), draw()
        kind = rng.random()
        if kind < 0.5:      # near cancellation: the case a fused and an unfused sum disagree on
            a, b = rng.uniform(-2, 2), rng.uniform(-2, 2)
            c = -(a * b) * (1 + rng.choice([0, 1e-16, -1e-16, 2 ** -30]))
        elif kind < 0.6:    # results in the subnormal range
            a, b, c = rng.uniform(-2, 2) * 1e-160, rng.uniform(-2, 2) * 1e-160, rng.choice([0.0, 5e-324, 1e-320, -1e-320])
        if not all(map(math.isfinite, (a, b, c))):
            continue
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        try:
            want = float(exact)
        except OverflowError:
            want = math.inf if exact > 0 else -math.inf
        got = ao.fma(a, b, c)
        assert got == want, (a, b, c, got, want)
        checked += 1
    assert checked > 15000
    assert math.isnan(ao.fma(math.inf, 0.0, 1.0)) and ao.fma(math.inf, 1.0, 1.0) == math.inf
    assert math.copysign(1.0, ao.fma(-0.0, 1.0, -0.0)) == -1.0 and math.copysign(1.0, ao.fma(-0.0, 1.0, 0.0)) == 1.0


def test_the_two_residual_forms_differ_and_agree_to_rounding():
    x, cents, pri, off, cand = ao.residual_case(1, 30, 7, 19, list_len=32)
    for o, cd in ((None, None), (off, cand)):
        sep, fus = ao.residuals(x, cents, pri, o, cd, ao.SEPARATE), ao.residuals(x, cents, pri, o, cd, ao.FUSED)
        for s, f in zip(sep, fus):
            assert (ao.bits(s) != ao.bits(f)).any()
            assert np.allclose(s, f, rtol=1e-13, atol=1e-13)      # 19 roundings of relative size 2^-53 at most
    # the primary norm is the candidate chain against the primary centroid
    pn, cn, _ = ao.residuals(x, cents, pri, None, None, ao.SEPARATE)
    has = pri != ao.NONE
    assert ao.same_bits(pn[has], cn.reshape(30, 7)[np.arange(30)[has], pri[has].astype(np.int64)])
    assert (pn[~has] == 0.0).all()


def test_centroids_keep_the_order_of_the_member_list():
    x, off, desc = ao.clustered_case(11, [300, 65], 37, order="descending")
    asc = np.concatenate([np.sort(desc[:300]), np.sort(desc[300:])]).astype(np.uint32)
    a, d = ao.centroids(x, off, asc)[0], ao.centroids(x, off, desc)[0]
    assert (ao.bits(a) != ao.bits(d)).any() and np.allclose(a, d, rtol=0, atol=1e-4)
    assert ao.centroids(x, [0, 0, 1], [5])[1].tolist() == [0, 1] and ao.same_bits(ao.centroids(x, [0, 0, 1], [5])[0][1], x[5])
    assert ao.same_bits(ao.mean_embedding([{"emb": []}, {"emb": x[1]}, {"emb": [1.0]}, {"emb": x[2]}], [0, 1, 2, 3, 9]),
                        ao.centroids(x, [0, 2], [1, 2])[0][0])


def test_selection_rules():
    rng = np.random.default_rng(5)
    x = ao.random_rows(rng, 12, 6)
    x[0:6] = x[0]      # duplicates: every tie goes to the first in list order
    x[8] = 0.0         # a zero row: distance 2.0
    cent = ao.centroids(x, [0, 12], list(range(12)))[0][0]
    assert ao.select_positions(x, list(range(6)), cent, 64) == [0, 1, 2, 3, 4, 5]      # n_extra beyond the candidates
    assert ao.select_positions(x, list(range(6, 12)), cent, 1) == [2]
    assert ao.select_positions(x, list(range(6, 12)), np.full(6, np.inf, np.float32), 1) == [0]      # NaN distances: minDist stays
    assert ao.select_positions(x, list(range(6, 12)), np.zeros(6, np.float32), 1) == [0]             # every distance 2.0
    assert ao.cosine_distance(x[8:9], cent)[0] == 2.0
    sel, cnt = ao.representatives(x, [0, 6, 12], list(range(12)), np.stack([cent, cent]), 3, empty=[1, 0])
    assert cnt.tolist() == [0, 3] and (sel[0] == ao.NONE).all() and len(set(sel[1].tolist())) == 3
    docs = [{"hash": h, "emb": x[i]} for i, h in enumerate("lkjihgfedcba")]
    docs[7]["hash"] = ""; docs[9]["emb"] = x[9][:3]; docs[10]["emb"] = np.array([np.nan] * 6, np.float32)
    got = ao.select_diverse(docs, [6, 7, 8, 9, 10, 11, 40], cent, 3)
    assert len(got) == 2 and set(got) <= {"f", "d", "a"} and ao.select_diverse(docs, [6, 8], cent, 1) == []


# ---- the golden file: the reference's own functions -----------------------------------------------------------------------------
import json          # noqa: E402
import subprocess    # noqa: E402
import sys           # noqa: E402
import tempfile      # noqa: E402

import pytest        # noqa: E402

GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "cluster_artifacts.json")
GOLDEN_FILE = json.load(open(GOLDEN_PATH))
GOLDEN = {c["name"]: c for c in GOLDEN_FILE["cases"]}
RESULT_KEYS = ("mean_bits", "selected", "assignments", "overlap", "members")


def test_the_golden_file_covers_the_cases_and_stays_small():
    assert set(GOLDEN) == set(ao.GOLDEN_CASES) and len(GOLDEN) >= 7
    assert os.path.getsize(GOLDEN_PATH) < 256 * 1024
    assert all(c["n"] <= 300 for c in GOLDEN.values())
    assert GOLDEN_FILE["forms"]["separate"].startswith("the reference's translation unit")
    # the cases reach what they are there for
    assert any(b in (0x7f800000, 0xff800000) for b in GOLDEN["huge_cluster_overflows"]["separate"]["mean_bits"][0])      # the fp32 mean overflowed
    assert [len(s) for s in GOLDEN["r_beyond_the_cluster"]["separate"]["selected"]] == [3, 1, 2, 30]                      # R beyond the cluster
    assert all(c["separate"]["assignments"] > 0 for c in GOLDEN.values())


@pytest.mark.parametrize("form", ["separate", "fused"])
@pytest.mark.parametrize("name", sorted(ao.GOLDEN_CASES))
def test_oracle_equals_the_reference_functions(name, form):
    docs, clusters, memberships, cfg = ao.GOLDEN_CASES[name]()
    got = ao.run_case(docs, clusters, memberships, cfg, ao.FUSED if form == "fused" else ao.SEPARATE)
    for key in RESULT_KEYS:
        assert got[key] == GOLDEN[name][form][key], (name, form, key)


def run_driver(exe, name, form, extra=()):
    docs, clusters, memberships, cfg = ao.GOLDEN_CASES[name]()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "case.bin")
        ao.write_case(path, docs, clusters, memberships, cfg)
        r = subprocess.run([exe, path, *(["--fused"] if form == "fused" else []), *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return ao.parse_driver(r.stdout)


@pytest.mark.parametrize("sanitize", [False, True])
def test_shell_over_a_stand_in_equals_the_golden_file(sanitize):
    """sanitize=True: the stand-alone program under AddressSanitizer and UBSan, on the CPU."""
    from _artifacts_build import build_shell_test
    exe = build_shell_test(sanitize=sanitize)
    for name in sorted(ao.GOLDEN_CASES):
        for form in ("separate", "fused"):
            got = run_driver(exe, name, form)
            assert got["probe"] == form, (name, form, got["probe"])      # the probe tells the stand-in's two forms apart
            for key in RESULT_KEYS:
                assert got[key] == GOLDEN[name][form][key], (name, form, key)


def test_stress_dry_run_and_self_test():
    for flag in ("--dry-run", "--self-test"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_artifacts.py"), flag], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
