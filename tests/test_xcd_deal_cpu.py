"""The deal of the int8 sweep's 512-row units to the eight XCDs (yams_amd/csrc/xcd_deal.h), on the CPU: the header the
kernels inline, compiled into a stand-alone program with AddressSanitizer + UBSan (tests/cpp/xcd_deal_test.cpp).

For n_units in {0, 1, 7, 8, 95, 96, 97, 12 019} x streams per XCD in {1, 4, 16} and each family of weights the program
checks: the units all streams produce are exactly [0, n_units), each once; equal weights reproduce the stream lengths of the
former rule `stream + j * n_streams`; no XCD and no stream exceeds its equal share by more than the clamp (8 %, + the
rounding to whole units); a stream that has ended stays ended.  `feedback`: the running average of the weights stays inside
the clamp whatever the measured times are, equal paces leave equal weights alone, a crawling XCD ends at the lower clamp,
and a launch without a usable time changes nothing."""
import subprocess

import pytest

import _xcd_deal_build


@pytest.fixture(scope="module")
def exe():
    return _xcd_deal_build.build_xcd_deal_test()


@pytest.mark.parametrize("kind", ["equal", "clamps", "one_min", "random", "feedback"])
def test_every_unit_is_dealt_once_and_no_stream_exceeds_the_clamp(exe, kind):
    p = subprocess.run([exe, kind], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "0 failures" in p.stdout, p.stdout[-2000:]
