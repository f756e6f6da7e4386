"""AccelExactScanBackend::searchDocumentCandidatesWithDiagnostics on the device route (vector_doc_scan_v1) equals the
all-rows route it replaces, bestRecordPerDocument(searchAllExactCandidateRowsWithDiagnostics(...)) — results, score
bits, order and diagnostics — through the reference's own IVectorStore headers (tests/cpp/doc_candidates_test.cpp).
The binary is compiled with the reference tree's headers, so it is built where that tree exists and travels prebuilt,
the recipe of _cpp_build.build_real_headers_test."""
import inspect
import os
import subprocess

import pytest

import _cpp_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


# the reference checkout the other host-adapter binaries are built against (one place names it: _cpp_build)
REFERENCE = inspect.signature(_cpp_build.build_real_headers_test).parameters["reference"].default


def build_doc_candidates_test(reference: str = REFERENCE):
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    exe = os.path.join(out_dir, "doc_candidates_test")
    src = os.path.join(ROOT, "tests", "cpp", "doc_candidates_test.cpp")
    if not os.path.isdir(os.path.join(reference, "include", "yams")):
        return exe if os.path.exists(exe) else None
    os.makedirs(out_dir, exist_ok=True)
    deps = [src, os.path.join(ROOT, "include", "yams_mi355x_accel.h")] + \
        [os.path.join(ROOT, "include", "yams_accel", f) for f in os.listdir(os.path.join(ROOT, "include", "yams_accel"))]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    cmd = [os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-Wall", "-Wno-unused-variable", "-DYAMS_ACCEL_USE_HOST_TYPES",
           "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(reference, "include"), "-I" + os.path.join(ROOT, "include"),
           "-o", exe, src, "-lpthread", "-ldl"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("doc_candidates_test failed to compile against the reference headers:\n" + r.stdout.decode())
    return exe


def test_device_document_route_equals_the_all_rows_route():
    from yams_amd import build as b
    b.build()
    exe = build_doc_candidates_test()
    if exe is None:
        pytest.skip("no doc_candidates_test binary (built only where the reference headers exist)")
    r = subprocess.run([exe, b.LIB], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "OK (0 failures" in r.stdout
