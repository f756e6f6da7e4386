"""Entity-vector search (yams_scan_entity_topk_device, vector_entity_scan_v1) without a GPU: the numpy restatement of the
reference's arithmetic pinned bit for bit on the reference-compiled computeCosineSimilarity (where oracle/_ref travelled) and
on the plain-C oracle, hand-computed cases of the order rule, the exported symbol and the interface table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _entity_oracle as eo

FLT_MAX = np.finfo(np.float32).max
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_entity_index_test():
    """Compiles tests/cpp/entity_index_test.cpp (plain g++, this repository's own record types; it dlopens the plugin at
    run time).  Returns the executable."""
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "entity_index_test")
    src = os.path.join(ROOT, "tests", "cpp", "entity_index_test.cpp")
    deps = [src, os.path.join(ROOT, "include", "yams_mi355x_accel.h")] + \
        [os.path.join(ROOT, "include", "yams_accel", f) for f in os.listdir(os.path.join(ROOT, "include", "yams_accel"))]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, src, "-ldl"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("entity_index_test failed to compile:\n" + r.stdout.decode())
    return exe


def special_rows(rng, n, d):
    """Seeded rows with the special cases of the contract: zero, inf, NaN, duplicates, the -0.0f construction, FLT_MAX / 4
    magnitudes, denormals."""
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[1] = 0.0                                              # zero row: +0.0 against anything
    rows[2, 2] = np.inf
    rows[3, 0] = np.nan
    rows[4] = rows[0]; rows[5] = rows[0]                       # duplicates
    rows[6] = 0.0; rows[6, 0] = np.float32(-1e-40); rows[6, 1] = np.float32(1e6)    # -0.0f against e0
    rows[7] = np.float32(FLT_MAX / 4)
    rows[8] = rows[8] * np.float32(1e-42)                      # denormals
    rows[9] = 0.0; rows[9, 0] = np.float32(1e-45)              # one denormal component (its square, 1e-90, is a normal fp64)
    rows[10] = -rows[0]
    return rows


def special_queries(rng, d, rows):
    e0 = np.zeros(d, np.float32); e0[0] = 1.0
    qn = rng.standard_normal(d).astype(np.float32); qn[2] = np.nan
    qi = rng.standard_normal(d).astype(np.float32); qi[1] = -np.inf
    return [rng.standard_normal(d).astype(np.float32), np.zeros(d, np.float32), e0, qn, qi, rows[0] * np.float32(3.0),
            np.full(d, FLT_MAX / 4, np.float32), (rng.standard_normal(d) * 1e-42).astype(np.float32)]


def same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize("d", [3, 50, 96, 384])
def test_restatement_equals_the_plain_c_oracle(oracle, d):
    rng = np.random.default_rng(d)
    rows = special_rows(rng, 300, d)
    for q in special_queries(rng, d, rows):
        want = np.array([oracle.cosine(q, r) for r in rows], np.float64).astype(np.float32)
        assert same_bits(eo.scores(rows, q), want)


@pytest.mark.parametrize("d", [3, 50, 96, 384])
def test_restatement_equals_the_reference_compiled_cosine(d):
    import _oracle
    t = _oracle.scan_ref()
    if t is None:
        pytest.skip("oracle/_ref/libyams_scan_ref.so not present (built only where the reference checkout exists)")
    rng = np.random.default_rng(100 + d)
    rows = special_rows(rng, 300, d)
    for q in special_queries(rng, d, rows):
        want = np.array([t.cosine(q, r) for r in rows], np.float64).astype(np.float32)
        assert same_bits(eo.scores(rows, q), want)


def test_the_special_scores_the_contract_names():
    d = 8
    rows = np.zeros((4, d), np.float32)
    rows[1, 2] = np.nan; rows[2, 2] = np.inf
    rows[3, 0] = np.float32(-1e-40); rows[3, 1] = np.float32(1e6)
    e0 = np.zeros(d, np.float32); e0[0] = 1.0
    s = eo.scores(rows, e0)
    assert s[0].view(np.uint32) == 0 and np.isnan(s[1]) and np.isnan(s[2])
    assert s[3].view(np.uint32) == 0x80000000                  # -0.0f: the fp64 quotient -1e-46 underflows in the cast
    z = eo.scores(rows, np.zeros(d, np.float32))
    assert (z.view(np.uint32) == 0).all()                      # a zero query scores +0.0 against NaN and inf rows too


def _rows_with_scores(vals):
    """Rows whose cosine against e0 is exactly the given value for 1, 0, -1 and signed zeros."""
    rows = np.zeros((len(vals), 4), np.float32)
    for i, v in enumerate(vals):
        if v == "nz":
            rows[i] = [-1e-40, 1e6, 0, 0]
        elif v == 0:
            rows[i] = [0, 1, 0, 0]
        elif v == 0.6:
            rows[i] = [3, 4, 0, 0]
        elif v == 0.8:
            rows[i] = [4, 3, 0, 0]
        else:
            rows[i] = [v, 0, 0, 0]
    return rows


E0 = np.array([1, 0, 0, 0], np.float32)


def test_order_rule_on_hand_computed_cases():
    rows = _rows_with_scores([0.6, 1, 0.6, -1, 1, 0.8, 0.6])
    r, s, vis, kept = eo.expected(rows, E0, 10, -1.0)
    assert r.tolist() == [1, 4, 5, 0, 2, 6, 3] and vis == 7 and kept == 7   # ties inside the result: row order
    assert s.tolist() == [1, 1, np.float32(0.8), np.float32(0.6), np.float32(0.6), np.float32(0.6), -1]
    r, _, _, kept = eo.expected(rows, E0, 4, -1.0)
    assert r.tolist() == [1, 4, 5, 0] and kept == 7                        # a tie run across position k: the first by row
    assert eo.expected(rows, E0, 0, -1.0)[0].tolist() == []                # k = 0
    r, _, _, kept = eo.expected(rows, E0, 3, np.float32(0.6))              # threshold exactly equal to a score: kept
    assert r.tolist() == [1, 4, 5] and kept == 6
    r, _, _, kept = eo.expected(rows, E0, 100, 0.9)                        # k > kept
    assert r.tolist() == [1, 4] and kept == 2
    r, _, vis, kept = eo.expected(rows, E0, 10, np.nan)                    # NaN threshold keeps nothing
    assert r.tolist() == [] and kept == 0 and vis == 7


def test_negative_zero_next_to_positive_zero():
    rows = _rows_with_scores([0, "nz", 0, -1, "nz"])
    r, s, _, kept = eo.expected(rows, E0, 10, 0.0)                         # -0.0f >= 0.0f: kept; one score with +0.0
    assert r.tolist() == [0, 1, 2, 4] and kept == 4
    assert s.view(np.uint32).tolist() == [0, 0x80000000, 0, 0x80000000]    # each row keeps its own bits
    assert eo.admissible(r, s, rows, E0, 10, 0.0) is None
    assert eo.admissible(r[[1, 0, 2, 3]], s[[1, 0, 2, 3]], rows, E0, 10, 0.0) is None   # the reference may order a run otherwise
    assert eo.admissible(r[:3], s[:3], rows, E0, 10, 0.0) == "score multiset"


def test_filters_and_unset_attributes():
    rows = _rows_with_scores([1, 1, 1, 1, 1, 1])
    types = np.array([0, 1, 0, 0xFF, 0, 2], np.uint8)
    nodes = np.array([5, 5, 6, 5, eo.UNSET, 5], np.uint32)
    docs = np.array([9, 9, 9, 9, 9, eo.UNSET], np.uint32)
    ex = lambda f, allowed=None: eo.expected(rows, E0, 10, 0.5, types, nodes, docs, f, allowed)[0].tolist()
    assert ex((0, None, None)) == [0, 2, 4]
    assert ex((None, 5, None)) == [0, 1, 3, 5]
    assert ex((0, 5, 9)) == [0]
    assert ex((None, None, 7)) == []                                       # an id no row carries
    assert ex((0xFF, None, None)) == [] and ex((None, eo.UNSET, None)) == [] and ex((None, None, eo.UNSET)) == []
    assert ex((0, None, None), allowed=[2, 3, 4]) == [2, 4]


def test_entity_topk_symbol_is_exported(accel_lib):
    from yams_amd import _lib
    assert hasattr(accel_lib, "yams_scan_entity_topk_device")
    assert "yams_scan_entity_topk_device" in _lib.EXPORTS
    assert C.sizeof(_lib.EntityFilter) == 16 and C.sizeof(_lib.ScanEntities) == 24


def test_vector_entity_scan_interface_and_refusal_without_a_gpu(accel_lib):
    import json
    from yams_amd import _lib
    L = accel_lib
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"vector_entity_scan_v1", 1, C.byref(p)) == 0
    vt = C.cast(p, C.POINTER(_lib.VectorEntityScanV1)).contents
    assert vt.abi_version == 1
    for fname, _ in _lib.VectorEntityScanV1._fields_[2:]:
        assert getattr(vt, fname), f"vector_entity_scan_v1.{fname} is NULL"
    for ver in (0, 2):
        q = C.c_void_p()
        assert L.yams_plugin_get_interface(b"vector_entity_scan_v1", ver, C.byref(q)) == -2
        assert q.value is None
    m = json.loads(L.yams_plugin_get_manifest_json())                      # the manifest is unchanged
    assert {(i["id"], i["version"]) for i in m["interfaces"]} == {("vector_scan_v1", 1), ("content_hash_v1", 1), ("chunker_v1", 3)}
    if L.yams_accel_device_count() > 0:
        return                                                             # the refusal below is what a CPU-only host sees
    L.yams_plugin_shutdown()
    assert L.yams_plugin_init(b"{}", None) == -3
    hits = C.POINTER(_lib.ScanHit)(); counts = _lib.u32p()
    qv = np.ones(4, np.float32)
    st = vt.search_entities(None, 1, qv.ctypes.data_as(_lib.f32p), None, 1, 4, 5, 0.5, None, C.byref(hits), C.byref(counts), None, None)
    assert st == _lib.YAMS_ERR_UNSUPPORTED                                  # it refuses, it does not fall back
    assert vt.corpus_set_attributes(None, 1, 0, 0, None, None, None) == _lib.YAMS_ERR_UNSUPPORTED


def test_entity_index_adapter_compiles_and_refuses_without_a_gpu(accel_lib):
    from yams_amd import build as b
    exe = build_entity_index_test()
    if accel_lib.yams_accel_device_count() > 0:
        return                                                             # the GPU suite runs the whole binary
    r = subprocess.run([exe, b.LIB, "--expect-no-gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr
