"""The adapters' side of the PQ sum-order probe on the device (tests/cpp/pq_calibration_gpu_test.cpp): after calibratePq with
the header's x8_halves_tail as the host a default-flag search equals the explicit-flag search and differs from the
sequential one on a corpus where the order decides; a host whose order is not served gets NotSupported; uncalibrated, the
result is the sequential one and the counter counts.  Compiled against the reference's headers where they exist (it drives
AccelExactScanBackend then), plain elsewhere (AccelVectorTable, which the backend forwards to)."""
import signal
import subprocess

import pytest

import _pq_calib_build

pytestmark = pytest.mark.gpu


def test_calibrated_refused_and_uncalibrated_pq_searches():
    from yams_amd import build as b
    b.build()
    exe, kind = _pq_calib_build.build_pq_calibration_gpu_test()
    r = subprocess.run([exe, b.LIB], capture_output=True, text=True, timeout=120)
    if r.returncode < 0:
        pytest.fail("pq_calibration_gpu_test was ended by signal %s\n%s" % (signal.Signals(-r.returncode).name, r.stdout[-3000:] + r.stderr[-2000:]))
    assert r.returncode == 0 and "OK (0 failures" in r.stdout and "[kind] " + kind in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    # one line on stderr for the index searched without calibration, not one per search
    assert r.stderr.count("without calibration") == 1, r.stderr[-2000:]
