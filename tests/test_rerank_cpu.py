"""The late-interaction rerank on the device (yams_rerank_*, late_interaction_rerank_v1) without a GPU: the header, the exports
and the bindings agree; the restatements of tests/_rerank_oracle.py (numpy with an exact fmaf, and our C++) equal each other
and what the REFERENCE'S OWN computeMaxSim, dot, maxPoolEmbeddings and normalizeEmbedding return in both forms
(tests/golden/colbert_maxsim.json, made by tests/golden/make_rerank_golden.py); every stress case discriminates, proven from
the oracle alone; the shell include/yams_accel/colbert_rerank.hpp over a stand-in table equals the same file and keeps its own
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

import _rerank_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "colbert_maxsim.json")
GOLDEN_FILE = json.load(open(GOLDEN_PATH))
GOLDEN = {c["name"]: c for c in GOLDEN_FILE["cases"]}
ENTRIES = ["yams_rerank_%s_%s" % (e, t) for e in ("maxsim", "maxpool") for t in ("device", "host")]


def test_header_exports_and_bindings_agree(accel_lib):
    from yams_amd import _lib
    from yams_amd import build as b
    header = open(os.path.join(ROOT, "include", "yams_mi355x_accel.h")).read()
    launch = open(os.path.join(ROOT, "yams_amd", "csrc", "rerank_launch.h")).read()
    for name in ENTRIES:
        assert re.search(r"YAMS_ACCEL_API yams_status_t " + name + r"\(", header), name
        assert name in _lib.EXPORTS and hasattr(accel_lib, name), name
    for macro, text, value in (("MAX_DIM", "1024u", _lib.RERANK_MAX_DIM), ("MAX_DOC_TOKENS", "(1u << 20)", _lib.RERANK_MAX_DOC_TOKENS),
                               ("MAX_QUERY_TOKENS", "(1u << 16)", _lib.RERANK_MAX_QUERY_TOKENS), ("MAX_ROWS", "(1ull << 28)", _lib.RERANK_MAX_ROWS),
                               ("MAX_DOCS", "(1ull << 20)", _lib.RERANK_MAX_DOCS), ("MAX_ROWMAX", "(1ull << 27)", _lib.RERANK_MAX_ROWMAX),
                               ("PATH_VALU", "0u", _lib.RERANK_PATH_VALU), ("PATH_MFMA", "1u", _lib.RERANK_PATH_MFMA),
                               ("NONE", "0xffffffffu", _lib.RERANK_NONE)):
        assert "#define YAMS_RERANK_%s %s" % (macro, text) in header, macro
        assert eval(text.replace("ull", "").replace("u", "")) == value, macro      # the C literal without its suffix
    # the reference shapes sit well inside: dim 48 .. 128, 512 tokens, a few hundred documents, a 32-token query
    assert _lib.RERANK_MAX_DIM >= 8 * 128 and _lib.RERANK_MAX_DOC_TOKENS >= 512 * 512 and _lib.RERANK_MAX_DOCS >= 300 * 512
    assert _lib.RERANK_MAX_ROWMAX >= 300 * 512 * 64 and _lib.RERANK_MAX_ROWS >= 300 * 512 * 64
    for const, value in (("kRerankQTile", _lib.RERANK_Q_TILE), ("kRerankDTile", _lib.RERANK_D_TILE), ("kRerankKChunk", _lib.RERANK_K_CHUNK)):
        assert re.search(r"constexpr int %s = %d;" % (const, value), launch), const
    assert '#define YAMS_IFACE_LATE_INTERACTION_RERANK_V1 "late_interaction_rerank_v1"' in header
    assert _lib.IFACE_LATE_INTERACTION_RERANK_V1 == "late_interaction_rerank_v1"
    assert C.sizeof(_lib.LateInteractionRerankV1) == 16 + 2 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.RerankDiag) == 32 and re.search(r"uint32_t path;.*\n\s*uint32_t form;.*\n\s*uint64_t rows;.*\n\s*uint64_t docs;", header)
    for name in ("rerank_kernels.hip", "rerank_api.cpp"):
        assert name in b.SOURCES
    assert ro.NONE == _lib.RERANK_NONE and (ro.SEPARATE, ro.FUSED) == (_lib.RESIDUAL_SEPARATE, _lib.RESIDUAL_FUSED)


def test_interface_table_is_served_at_version_1_only(accel_lib):
    from yams_amd import _lib
    p = C.c_void_p()
    assert accel_lib.yams_plugin_get_interface(b"late_interaction_rerank_v1", 1, C.byref(p)) == 0 and p.value
    vt = C.cast(p, C.POINTER(_lib.LateInteractionRerankV1)).contents
    assert vt.abi_version == 1 and vt.maxsim and vt.maxpool
    for version in (0, 2):
        q = C.c_void_p()
        assert accel_lib.yams_plugin_get_interface(b"late_interaction_rerank_v1", version, C.byref(q)) != 0 and not q.value
    assert b"late_interaction_rerank_v1" not in accel_lib.yams_plugin_get_manifest_json()
    if accel_lib.yams_accel_device_count() == 0:      # without a device the door refuses
        assert vt.maxpool(None, None, 4, None, 0, None) == _lib.YAMS_ERR_UNSUPPORTED


def test_a_null_context_is_refused(accel_lib):
    from yams_amd import _lib
    for t in ("device", "host"):
        assert getattr(accel_lib, "yams_rerank_maxsim_" + t)(None, None, 0, 4, None, None, 0, 0, None, None, None, None) == _lib.YAMS_ERR_INVALID_ARG
        assert getattr(accel_lib, "yams_rerank_maxpool_" + t)(None, None, 4, None, 0, None) == _lib.YAMS_ERR_INVALID_ARG


def test_the_golden_file_covers_the_cases_and_what_the_tests_rely_on():
    assert os.path.getsize(GOLDEN_PATH) < 256 << 10
    assert [c["name"] for c in GOLDEN_FILE["cases"]] == ro.case_names()
    assert set(GOLDEN_FILE["forms"]) == {"separate", "fused"}
    assert all(GOLDEN[n]["sha256"] == ro.case_digest(n) for n in GOLDEN)
    flips = [n for n in GOLDEN if n.startswith("flip_")]
    assert sum(GOLDEN[n]["separate"] != GOLDEN[n]["fused"] for n in flips) >= 4
    assert all(GOLDEN[n]["separate"] == GOLDEN[n]["fused"] for n in ro.pool_cases())
    for form in ("separate", "fused"):
        v = {n: ro.from_hex(GOLDEN[n][form]) for n in GOLDEN}
        assert v["empty_document"][0] == -np.inf and ro.hexbits(v["empty_query"]) == "00000000"
        assert v["nan_document_token"][0] == 5.0 and v["nan_query_token"][0] == -np.inf and np.isnan(v["inf_pair"][0])
        assert v["subnormal_only"][0] != 0 and abs(v["subnormal_only"][0]) < 1e-37
        assert v["pool_all_nan_dimension"][0] == 0 and not v["pool_tiny_norm"].any() and v["pool_just_above"][0] > 0.9


@pytest.mark.parametrize("form", ["separate", "fused"])
def test_both_restatements_equal_the_reference(form):
    want = ro.nan_blind([c[form] for c in GOLDEN_FILE["cases"]])
    assert ro.nan_blind(ro.restated(ro.FORMS[form])) == want                                                           # numpy
    assert ro.nan_blind(ro.restated(ro.FORMS[form], lambda q, x, o, f: ro.maxsim_cpp(q, x, o, f)[0], ro.maxpool_cpp)) == want      # C++


def test_the_restatements_agree_on_row_maxima_and_winners():
    for name, (q, x, off) in ro.maxsim_cases().items():
        dim = min(q.shape[1], x.shape[1])
        q, x = np.ascontiguousarray(q[:, :dim]), np.ascontiguousarray(x[:, :dim])
        for form in (ro.SEPARATE, ro.FUSED):
            a, b = ro.maxsim_py(q, x, off, form), ro.maxsim_cpp(q, x, off, form)
            assert all(ro.equal(u, v) for u, v in zip(a, b)), (name, form)
    # equal zeros of both signs: the first in document order stays, sign and index.  A sim is -0.0f only in the fused form, as
    # a negative product that underflows (a separate chain starts from +0.0f + -0.0f = +0.0f).
    for q, rows, off, want in ro.zero_tie_cases():
        for fn in (ro.maxsim_py, ro.maxsim_cpp):
            for form in (ro.SEPARATE, ro.FUSED):
                _, mx, arg = fn(q, rows, off, form)
                assert mx.view(np.uint32)[:, 0].tolist() == want[form] and not arg.any(), (form, mx)


def test_the_exact_fmaf_is_the_libm_one():
    rng = np.random.default_rng(3)
    a, b, c = (ro.mixed(rng, 4000, -30, 30) for _ in range(3))
    c[:500] = -(a[:500] * b[:500])      # cancellation: the low bits of the product decide
    c[500:600] = np.float32(1e-40)
    a[500:600] *= np.float32(1e-30)
    got = ro.fmaf(a, b, c)
    fm = C.CDLL("libm.so.6").fmaf
    fm.restype, fm.argtypes = C.c_float, [C.c_float] * 3
    want = np.array([fm(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert ro.same_bits(got, want)


def test_every_stress_case_discriminates():
    """From the oracle alone: the score bits of EVERY case change under a reversed i order, a dropped last document token and a
    dropped last query token; under the other form for at least half of the cases (44 of the 60 of seed 1)."""
    import stress_rerank
    cases, share = stress_rerank.draw_all(1, 60)
    for c in cases:
        r = ro.discriminates(c)
        assert all(r[:3]), (c["seed"], r)
        assert r[3] == c["other_form"]
    assert 2 * share >= len(cases)


def test_stress_harness_dry_run_and_self_test():
    script = os.path.join(ROOT, "tests", "stress_rerank.py")
    r = subprocess.run([sys.executable, script, "--dry-run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dry run OK: 60 cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([sys.executable, script, "--self-test"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "self-test OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_probe_samples_in_the_header_tell_the_forms_apart():
    shell = open(os.path.join(ROOT, "include", "yams_accel", "colbert_rerank.hpp")).read()

    def table(name):
        body = re.search(r"%s\[kCases\]\[\d\] = (.*?);" % name, shell, re.S).group(1)
        return np.array([int(h, 16) for h in re.findall(r"0x([0-9a-f]{8})u", body)], np.uint32)
    q, d, s = table("kQuery").reshape(3, 4), table("kDoc").reshape(3, 4), table("kScore").reshape(3, 2)
    for k in range(3):
        for form in (ro.SEPARATE, ro.FUSED):
            for fn in (ro.maxsim_py, ro.maxsim_cpp):
                got = fn(q[k:k + 1].view(np.float32), d[k:k + 1].view(np.float32), ro.csr([1]), form)[0]
                assert got.view(np.uint32)[0] == s[k, form], (k, form)
        assert s[k, 0] != s[k, 1]


@pytest.mark.parametrize("sanitize", [False, True])
def test_shell_over_the_stand_in_equals_the_reference(sanitize):
    """AccelColbertReranker over a table backed by the restatement, with a host function of each form: the probe finds the form,
    the cases equal the golden file; --selftest: the probe's three answers, ragged token vectors, min(dim), refusals.
    sanitize: the same stand-alone program under AddressSanitizer and UBSan."""
    from _rerank_build import build_shell_test
    exe = build_shell_test(sanitize=sanitize)
    r = subprocess.run([exe, "--selftest"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "selftest OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.bin")
        ro.write_cases(path)
        for form in ("separate", "fused"):
            r = subprocess.run([exe, *(["--fused"] if form == "fused" else []), path], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
            probe, got = ro.parse_driver_output(r.stdout)
            assert probe == form
            assert ro.nan_blind(got) == ro.nan_blind([c[form] for c in GOLDEN_FILE["cases"]]), form
