"""computePersistenceH0 on the device (yams_quality_persistence_h0_*, topology_quality_v1) without a GPU: the header, the
exports and the bindings agree; the restatements of tests/_persistence_oracle.py (numpy / exact fma, and our C++) equal each
other and what the REFERENCE'S OWN computePersistenceH0 returns in both chain forms (tests/golden/persistence_h0.json, made by
tests/golden/make_persistence_golden.py); the sorted merge weights of the reference's Kruskal are those of a Prim restatement,
ties or not; the shell include/yams_accel/topological_quality.hpp over a stand-in table equals the same file and keeps its own
rules, also as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _persistence_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "persistence_h0.json")
GOLDEN_FILE = json.load(open(GOLDEN_PATH))
GOLDEN = {c["name"]: c for c in GOLDEN_FILE["cases"]}
ENTRIES = ["yams_quality_persistence_h0_device", "yams_quality_persistence_h0_host"]


def test_header_exports_and_bindings_agree(accel_lib):
    from yams_amd import _lib
    header = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    for name in ENTRIES:
        assert re.search(r"YAMS_ACCEL_API yams_status_t " + name + r"\(", header), name
        assert name in _lib.EXPORTS and hasattr(accel_lib, name), name
    assert re.search(r"#define YAMS_QUALITY_MAX_POINTS 16384u\b", header) and _lib.QUALITY_MAX_POINTS == po.MAX_POINTS == 16384
    assert '#define YAMS_IFACE_TOPOLOGY_QUALITY_V1 "topology_quality_v1"' in header
    assert C.sizeof(_lib.PersistenceH0) == 40
    for name in ("persistence_kernels.hip", "persistence_api.cpp"):
        from yams_amd import build as b
        assert name in b.SOURCES


def test_interface_table_is_served_at_version_1_only(accel_lib):
    from yams_amd import _lib
    p = C.c_void_p()
    assert accel_lib.yams_plugin_get_interface(b"topology_quality_v1", 1, C.byref(p)) == 0 and p.value
    vt = C.cast(p, C.POINTER(_lib.TopologyQualityV1)).contents
    assert vt.abi_version == 1 and vt.persistence_h0 and vt.free_persistence_h0
    for version in (0, 2):
        q = C.c_void_p()
        assert accel_lib.yams_plugin_get_interface(b"topology_quality_v1", version, C.byref(q)) != 0 and not q.value
    # served by get_interface like the other topology interfaces; the manifest keeps its three entries (see the header)
    assert b"topology_quality_v1" not in accel_lib.yams_plugin_get_manifest_json()
    if accel_lib.yams_accel_device_count() == 0:      # without a device the door refuses
        res = _lib.PersistenceH0()
        assert vt.persistence_h0(None, None, 0, 4, None, 0, 0, C.byref(res), None, None) == _lib.YAMS_ERR_UNSUPPORTED


def test_a_null_context_is_refused(accel_lib):
    from yams_amd import _lib
    res = _lib.PersistenceH0()
    for fn in (accel_lib.yams_quality_persistence_h0_device, accel_lib.yams_quality_persistence_h0_host):
        assert fn(None, None, 0, 4, None, 0, 0, C.byref(res), None, None, None) == _lib.YAMS_ERR_INVALID_ARG


def test_the_percentile_index_is_the_references_expression():
    assert [po.percentile_index(e) for e in (0, 1, 2, 3, 21, 820, 134209536)] == [0, 0, 0, 1, 19, 778, 127499058]


def test_the_golden_file_covers_the_cases_and_stays_small():
    assert os.path.getsize(GOLDEN_PATH) < 256 << 10
    assert sorted(GOLDEN) == sorted(po.GOLDEN_CASES)
    assert set(GOLDEN_FILE["forms"]) == {"separate", "fused"}
    mixed = [c for n, c in GOLDEN.items() if n.startswith("mixed_")]
    assert len(mixed) >= 40 and all(3 <= c["m"] <= 6 for c in mixed)
    assert sum(c["separate"]["returned"] != c["fused"]["returned"] for c in mixed) >= 4      # the value tells the forms apart
    assert po.plateau_is_strictly_inside(po.GOLDEN_CASES["lattice_plateau_m30"]())
    zero = GOLDEN["duplicates_norm_zero_m41"]["separate"]
    assert po.from_hex64(zero["restatement"]["norm"]) == 0.0 and po.from_hex64(zero["returned"]) == 0.0 and zero["restatement"]["n_merges"] == 0
    assert GOLDEN["two_points"]["m"] == 2 and po.from_hex64(GOLDEN["two_points"]["separate"]["returned"]) == 0.0
    assert po.from_hex64(GOLDEN["two_points"]["separate"]["restatement"]["norm"]) > 0.0
    assert po.from_hex64(GOLDEN["clusters_4x6_d9"]["separate"]["returned"]) > 0.0


@pytest.mark.parametrize("form", ["separate", "fused"])
def test_both_restatements_equal_the_reference_function(form):
    for name, make in po.GOLDEN_CASES.items():
        x = make()
        assert po.digest(x) == GOLDEN[name]["sha256"], name
        py, cpp = po.persistence_py(x, po.FORMS[form]), po.persistence_cpp(x, po.FORMS[form])
        assert po.same(py, cpp), (name, form)
        assert po.hex64(py["value"]) == GOLDEN[name][form]["returned"], (name, form)
        assert po.golden_record(py) == GOLDEN[name][form]["restatement"], (name, form)


def test_the_two_forms_differ_in_a_tenth_of_the_distances_and_agree_to_rounding():
    x = po.mixed_points(11, 40, 64)
    a, b = po.persistence_cpp(x, po.SEPARATE)["distances"], po.persistence_cpp(x, po.FUSED)["distances"]
    share = float((po.bits64(a) != po.bits64(b)).mean())
    assert 0.02 < share < 0.5, share
    assert np.abs(a - b).max() <= 2 * np.spacing(a.max())
    one = po.mixed_points(12, 50, 1)      # dim 1: 0.0 + d * d rounds once either way
    assert (po.bits64(po.persistence_cpp(one, po.SEPARATE)["distances"]) == po.bits64(po.persistence_cpp(one, po.FUSED)["distances"])).all()


def test_kruskals_sorted_weights_are_those_of_any_minimum_spanning_tree():
    """The reference's stable sort does not have to be reproduced: on clouds full of equal distances the sorted merge weights
    of its Kruskal equal those of Prim from vertex 0, and the value is their ascending sum without the heaviest."""
    clouds = [po.lattice_points(1, 60, 2), po.lattice_points(2, 90, 3, side=3), po.GOLDEN_CASES["lattice_plateau_m30"](),
              po.duplicated_points(4, 30, 10, 5), po.duplicated_points(5, 40, 1, 7), po.cluster_points(7, 4, 12, 9), po.mixed_points(8, 70, 5)]
    for x in clouds:
        for form in (po.SEPARATE, po.FUSED):
            r = po.persistence_cpp(x, form)
            assert (np.diff(r["weights"]) >= 0).all()      # Kruskal merges in ascending order
            assert (po.bits64(r["weights"]) == po.bits64(po.prim_weights(r["distances"]))).all()
            py = po.kruskal(r["distances"])
            assert (po.bits64(py) == po.bits64(r["weights"])).all()
            total = 0.0
            for w in r["weights"][:-1]:
                total += float(w) / r["norm"] if r["norm"] > 0 else 0.0
            assert po.hex64(total) == po.hex64(r["value"])
    tied = po.persistence_cpp(clouds[0], po.SEPARATE)["weights"]
    assert len(np.unique(tied)) < len(tied) // 2      # the case is tie-heavy


def run_driver(exe, form, names, extra=()):
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, name in enumerate(names):
            paths.append(os.path.join(tmp, "case_%03d.bin" % i))
            po.write_case(paths[-1], po.GOLDEN_CASES[name]())
        r = subprocess.run([exe, *(["--fused"] if form == "fused" else []), *extra, *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = r.stdout.split("\n")
    return lines[0], [l.split()[1:] for l in lines[1:] if l.startswith("value")]


@pytest.mark.parametrize("sanitize", [False, True])
def test_shell_over_a_stand_in_equals_the_golden_file_and_keeps_its_rules(sanitize):
    """sanitize=True: the same driver as a stand-alone program under AddressSanitizer and UBSan (CPU only, its own main).  The
    self-test covers the early returns of both overloads, ragged rows, the probe answering each form and the Error, refusals."""
    from _persistence_build import build_shell_test
    exe = build_shell_test(sanitize=sanitize)
    r = subprocess.run([exe, "--selftest"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "selftest ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    names = sorted(po.GOLDEN_CASES)
    for form in ("separate", "fused"):
        probe, values = run_driver(exe, form, names)
        assert probe == "probe " + form
        assert values == [[GOLDEN[n][form]["returned"]] * 2 for n in names]


def test_stress_dry_run_and_self_test():
    script = os.path.join(ROOT, "tests", "stress_persistence.py")
    r = subprocess.run([sys.executable, script, "--dry-run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dry run OK: 60 cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([sys.executable, script, "--self-test"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "self-test OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
