"""The argument checks that need neither the device nor a context (yams_amd/csrc/arg_checks.h: overlaps, offsets_ascend) on the
CPU: compiled with plain g++ under AddressSanitizer and UBSan into tests/cpp/arg_checks_test and run there."""
import subprocess

import _cpp_build


def test_the_pure_argument_checks_under_asan_and_ubsan():
    exe = _cpp_build.build_arg_checks_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
