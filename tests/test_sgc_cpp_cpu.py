"""tests/cpp/sgc_test.cpp without a GPU: AccelSGC (include/yams_accel/topology_sgc.hpp) over a stand-in table.

  - as a stand-alone program under AddressSanitizer and UBSan: the shell's early returns, write-back, refusal and lists;
  - linked, in a temporary directory, with the reference's own topology_sgc.cpp where the reference checkout is present: the
    shell's result must equal applySGCSmoothing bit for bit on seeded cases of 3000 documents (dims 1 / 37 / 64, 1-3 hops,
    ragged rows).  This is the test that holds the claim about the order of the lists to the reference itself."""
import os
import subprocess
import tempfile

import pytest

from _sgc_build import CXX, ROOT, SRC, build_sgc_test

REFERENCE = os.environ.get("YAMS_REFERENCE", "/root/reference")


def test_shell_over_a_stand_in_under_the_sanitizers():
    r = subprocess.run([build_sgc_test(sanitize=True)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "src", "topology", "topology_sgc.cpp")),
                    reason="needs the reference checkout (its own topology_sgc.cpp is linked in)")
def test_shell_equals_the_reference_function_bit_for_bit():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sgc_test_ref")
        cmd = [CXX, "-std=c++20", "-O2", "-Wall", "-Wno-unused-variable", "-DSGC_WITH_REFERENCE", "-DYAMS_ACCEL_USE_HOST_TYPES",
               "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(REFERENCE, "include"), "-I" + os.path.join(ROOT, "include"),
               "-o", exe, SRC, os.path.join(REFERENCE, "src", "topology", "topology_sgc.cpp"), "-ldl"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "6 cases" in r.stdout and "OK (0 failures)" in r.stdout, r.stdout + r.stderr
