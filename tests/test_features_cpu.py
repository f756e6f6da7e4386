"""The topology build's input features on the device (yams_features_*, topology_features_v1) without a GPU: the header, the
exports and the bindings agree; the restatements of tests/_features_oracle.py (numpy / exact fma, and our C++) equal each other
and what the REFERENCE'S OWN aggregateEmbedding, computeVarianceWeights, bucketCountSketch and composeFeatureVector return in
both variance forms (tests/golden/features.json, made by tests/golden/make_features_golden.py); the heap select restated in
Python keeps the dimensions this library's std::partial_sort keeps, ties or not; the shell
include/yams_accel/topology_features.hpp over a stand-in table equals the same file and keeps its own rules, also as a
stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _features_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "features.json")
GOLDEN_FILE = json.load(open(GOLDEN_PATH))
GOLDEN = {c["name"]: c for c in GOLDEN_FILE["cases"]}
ENTRIES = ["yams_features_%s_%s" % (e, t) for e in ("aggregate", "variance", "compose") for t in ("device", "host")]


def vec(hexbits):
    return np.frombuffer(bytes.fromhex(hexbits), np.float32)


def test_header_exports_and_bindings_agree(accel_lib):
    from yams_amd import _lib
    from yams_amd import build as b
    header = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    for name in ENTRIES:
        assert re.search(r"YAMS_ACCEL_API yams_status_t " + name + r"\(", header), name
        assert name in _lib.EXPORTS and hasattr(accel_lib, name), name
    assert re.search(r"#define YAMS_FEATURES_MAX_DIM 4096u\b", header) and _lib.FEATURES_MAX_DIM == fo.MAX_DIM == 4096
    assert re.search(r"#define YAMS_FEATURES_MAX_SIG_LEN 65536u\b", header) and _lib.FEATURES_MAX_SIG_LEN == fo.MAX_SIG_LEN == 65536
    assert '#define YAMS_IFACE_TOPOLOGY_FEATURES_V1 "topology_features_v1"' in header
    assert C.sizeof(_lib.TopologyFeaturesV1) == 16 + 3 * C.sizeof(C.c_void_p)
    for name in ("features_kernels.hip", "features_api.cpp"):
        assert name in b.SOURCES
    shell = open(os.path.join(ROOT, "include", "yams_accel", "topology_features.hpp")).read()
    assert "kVarianceSampleCap = 4096" in shell and fo.SAMPLE_CAP == 4096


def test_interface_table_is_served_at_version_1_only(accel_lib):
    from yams_amd import _lib
    p = C.c_void_p()
    assert accel_lib.yams_plugin_get_interface(b"topology_features_v1", 1, C.byref(p)) == 0 and p.value
    vt = C.cast(p, C.POINTER(_lib.TopologyFeaturesV1)).contents
    assert vt.abi_version == 1 and vt.aggregate and vt.variance and vt.compose
    for version in (0, 2):
        q = C.c_void_p()
        assert accel_lib.yams_plugin_get_interface(b"topology_features_v1", version, C.byref(q)) != 0 and not q.value
    # served by get_interface like the other topology interfaces; the manifest keeps its three entries (see the header)
    assert b"topology_features_v1" not in accel_lib.yams_plugin_get_manifest_json()
    if accel_lib.yams_accel_device_count() == 0:      # without a device the door refuses
        assert vt.variance(None, None, 0, 4, None, 0, 0, None, None) == _lib.YAMS_ERR_UNSUPPORTED


def test_a_null_context_is_refused(accel_lib):
    from yams_amd import _lib
    z = C.c_float(0.0)
    for t in ("device", "host"):
        assert getattr(accel_lib, "yams_features_aggregate_" + t)(None, None, 0, 4, None, None, 0, None, None) == _lib.YAMS_ERR_INVALID_ARG
        assert getattr(accel_lib, "yams_features_variance_" + t)(None, None, 0, 4, None, 0, 0, None, None) == _lib.YAMS_ERR_INVALID_ARG
        assert getattr(accel_lib, "yams_features_compose_" + t)(None, None, 0, 4, None, None, 0, None, None, 0, None, 0, z, z, None, 0,
                                                                None) == _lib.YAMS_ERR_INVALID_ARG


def test_the_golden_file_covers_the_cases_and_what_the_tests_rely_on():
    assert os.path.getsize(GOLDEN_PATH) < 256 << 10
    assert [c["name"] for c in GOLDEN_FILE["cases"]] == fo.case_names()
    assert set(GOLDEN_FILE["forms"]) == {"separate", "fused"}
    assert GOLDEN["aggregate"]["sha256"] == fo.aggregate_digest()
    assert all(GOLDEN[n]["sha256"] == fo.variance_digest(n) for n in fo.VARIANCE_CASES)
    assert all(GOLDEN[n]["sha256"] == fo.compose_digest(n) for n in fo.COMPOSE_CASES)
    flips = [n for n in GOLDEN if n.startswith("var_flip_")]
    assert sum(GOLDEN[n]["separate"] != GOLDEN[n]["fused"] for n in flips) >= 4          # the weights tell the forms apart
    assert all(GOLDEN[n]["separate"] == GOLDEN[n]["fused"] for n in GOLDEN if not n.startswith("var_"))      # the rest is form-free
    agg = GOLDEN["aggregate"]["separate"]
    assert agg[0] == "" and np.signbit(vec(agg[1])[[0, 2, 4]]).all()                      # assigned: a lone -0.0f stays
    assert np.signbit(vec(agg[2])[[0, 4]]).all() and not np.signbit(vec(agg[2])[2])       # -0.0f + -0.0f; a `0.0f +` start gives +0.0f
    tie = vec(GOLDEN["var_tie_at_cut_t2"]["separate"][0])
    assert tie[0] > 0 and (tie[1] > 0) != (tie[2] > 0)                                    # equal variances straddle the cut
    assert (vec(GOLDEN["var_zero_inside_top_t3"]["separate"][0]) > 0).sum() == 2          # kept count < target
    off = GOLDEN["compose_all_off"]["separate"]
    dense = fo.COMPOSE_CASES["compose_all_off"]["dense"]
    assert fo.same_bits(vec(off[1]), dense[1])                                            # sumSq == 0
    assert vec(off[2])[4] == 1.0                                                          # the smallest norm there is, 2^-149
    assert (vec(off[3]) == 0).all()                                                       # the norm rounds to inf
    assert (vec(GOLDEN["compose_nan_alpha"]["separate"][5])[:9] == 0).all()               # a NaN alpha: aD = 0.0f
    assert sorted(len(vec(v)) for v in GOLDEN["compose_four_combinations"]["separate"][:4]) == [9, 12, 16, 19]
    assert fo.same_bits(vec(GOLDEN["compose_weights_of_another_size"]["separate"][0]), dense[0])      # :169-171: un-normalised


def test_no_norm_can_round_to_zero():
    """sqrt(sumSq) >= the largest |x| >= 2^-149, which float represents: the smallest float alone normalises to 1.0f."""
    x = np.zeros((1, 3), np.float32)
    x[0, 1] = fo.TINY
    for compose in (fo.compose_py, fo.compose_cpp):
        out, _ = compose(x, None, None, None, None, None, 0, 0.0, 0.0)
        assert out[0].tolist() == [0.0, 1.0, 0.0]
    assert np.float32(np.sqrt(np.float64(fo.TINY) ** 2)) == fo.TINY


@pytest.mark.parametrize("form", ["separate", "fused"])
def test_both_restatements_equal_the_reference_functions(form):
    want = [c[form] for c in GOLDEN_FILE["cases"]]
    assert fo.restated(fo.FORMS[form]) == want
    assert fo.restated(fo.FORMS[form], fo.aggregate_cpp, fo.variance_cpp, fo.weights_cpp, fo.compose_cpp) == want


def test_the_two_forms_differ_in_many_variances_and_agree_to_rounding():
    rng = np.random.default_rng(11)
    x = fo.mixed(rng, (40, 64))
    a, b = fo.variance_cpp(x, None, fo.SEPARATE), fo.variance_cpp(x, None, fo.FUSED)
    assert fo.same_bits(a[0], b[0])                                      # the mean has no product
    share = float((a[1].view(np.uint64) != b[1].view(np.uint64)).mean())
    assert 0.1 < share, share
    assert np.abs(a[1] - b[1]).max() <= 64 * np.spacing(a[1].max())
    one = fo.mixed(rng, (1, 9))                                          # m == 1: d == 0, both forms give +0.0
    assert fo.same_bits(fo.variance_cpp(one, None, 0)[1], np.zeros(9)) and fo.same_bits(fo.variance_cpp(one, None, 1)[1], np.zeros(9))


def test_the_heap_select_keeps_what_partial_sort_keeps():
    for seed in range(300):
        rng = np.random.default_rng(seed)
        dim = int(rng.integers(2, 70))
        target = int(rng.integers(1, dim))
        var = rng.integers(0, 5, dim).astype(np.float64) if seed % 2 else rng.random(dim)      # tie-heavy, or none
        assert fo.same_bits(fo.weights_py(var, target), fo.weights_cpp(var, target)), seed
    nan = np.array([1.0, np.nan, 2.0])
    assert fo.weights_py(nan, 1) is None and fo.weights_cpp(nan, 1) is None


def test_the_sketch_chain_is_exact_in_any_order():
    """Counts are integers summing to sig_len <= 65536: every partial sum of their squares is an integer <= 2^32."""
    rng = np.random.default_rng(5)
    sig = rng.integers(0, 1 << 32, (3, 65536), dtype=np.uint64).astype(np.uint32)
    sig[1] = 7
    for sd in (1, 7, 4096):
        counts = np.stack([np.bincount(s.astype(np.int64) % sd, minlength=sd) for s in sig])
        total = (counts.astype(np.uint64) ** 2).sum(1)
        assert total.max() <= 1 << 32
        out, _ = fo.compose_cpp(np.ones((3, 1), np.float32), None, None, None, sig, np.ones(3, np.uint8), sd, 0.0, 1.0)
        norm = np.sqrt(total.astype(np.float64)).astype(np.float32)
        assert fo.same_bits(out[:, 1:], (counts.astype(np.float32) / norm[:, None]).astype(np.float32))


def run_driver(exe, form):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.bin")
        fo.write_cases(path)
        r = subprocess.run([exe, *(["--fused"] if form == "fused" else []), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return fo.parse_driver_output(r.stdout)


@pytest.mark.parametrize("sanitize", [False, True])
def test_shell_over_a_stand_in_equals_the_golden_file_and_keeps_its_rules(sanitize):
    """sanitize=True: the same driver as a stand-alone program under AddressSanitizer and UBSan (CPU only, its own main).  The
    self-test covers the record admissions, the sample cap, the early returns, the NaN variance, the probe answering each form
    and the Error, the conditions of the composer, refusals."""
    from _features_build import build_shell_test
    exe = build_shell_test(sanitize=sanitize)
    r = subprocess.run([exe, "--selftest"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "selftest ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    for form in ("separate", "fused"):
        probe, got = run_driver(exe, form)
        assert probe == form
        assert got == [c[form] for c in GOLDEN_FILE["cases"]]


def test_the_probe_samples_are_the_recorded_ones():
    shell = open(os.path.join(ROOT, "include", "yams_accel", "topology_features.hpp")).read()
    for seed in fo.FLIP_SEEDS[3]:
        x = fo.flip_sample(seed, 3)
        assert ", ".join("0x%08xu" % v for v in x.reshape(-1).view(np.uint32)) in shell, seed
        for form in (fo.SEPARATE, fo.FUSED):
            w = fo.shell_variance_weights([r for r in x], 1, form)
            assert ", ".join("0x%08xu" % v for v in w.view(np.uint32)) in shell, (seed, form)


def test_stress_dry_run_and_self_test():
    script = os.path.join(ROOT, "tests", "stress_features.py")
    r = subprocess.run([sys.executable, script, "--dry-run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dry run OK: 60 cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([sys.executable, script, "--self-test"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "self-test OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
