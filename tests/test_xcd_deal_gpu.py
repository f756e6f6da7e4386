"""The int8 sweep's weighted deal of 512-row units to the XCDs (yams_amd/csrc/xcd_deal.h) on the device: whatever the weights,
the top-k is what the CPU oracle computes, bit for bit — which stream scores a row changes nothing.

The resident-query form is asked for (YAMS_SCAN_FLAG_RESIDENT_QUERIES) on small shards: 4 096 rows, 4 160 (a ragged last
block) and 66 000; dims 384 and 768 (the two-slabs-in-flight kernel); 128, 300 (a partial last query tile) and 1024 queries;
cosine and L2.  A shard of up to 8 192 rows is sampled whole (make_plan: the sample is at least 8 192 rows) — the filter pass
has no tile left and no deal happens; those shapes still have to give the oracle's answer under the knob.  The smallest
shards the resident form does accept have 64 tiles of 256 rows, every second one a filter tile: 16 384 rows (16 units: two
per XCD) and 16 704 (a last filter tile of 64 rows) are here for that.  The measurement build's YAMS_ACCEL_XCD_WEIGHTS knob
forces the weights to equal, to both clamps alternating and to one XCD at the minimum (tests/_xcd_deal_forms.py: one process
for all shapes — the measurement library is chosen at import — run once per session, one test per shape reads its
record).  A last test runs three calls in a row on one context with the feedback on."""
import itertools
import json
import os
import subprocess
import sys

import pytest

from yams_amd import _lib
from yams_amd import build as _build

pytestmark = pytest.mark.gpu

SHAPES = [[n, d, nq, m] for n, d, nq, m in itertools.product((4096, 4160, 16384, 16704, 66000), (384, 768), (128, 300, 1024), ("cosine", "l2"))]
FORCED = {"equal": [1.0] * 8, "clamps": [0.92, 1.08] * 4, "one_min": [1, 1, 1, 0.92, 1, 1, 1, 1]}
CLAMP = 0.08


@pytest.fixture(scope="module")
def records():
    assert os.path.exists(_build.MEASURE_LIB), "the measurement build is not in the tree (python -m yams_amd.build --measure)"
    env = dict(os.environ, YAMS_ACCEL_MEASURE_LIB="1", XCD_SHAPES=json.dumps(SHAPES))
    env.pop("YAMS_ACCEL_XCD_WEIGHTS", None)
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_xcd_deal_forms.py")], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert [r["shape"] for r in out["shapes"]] == SHAPES
    return out


def _check_off(off, units):
    assert len(off) == 9 and off[0] == 0 and off[8] == units, (off, units)
    assert all(a <= b for a, b in zip(off, off[1:])), off


@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=["-".join(map(str, s)) for s in SHAPES])
def test_results_do_not_depend_on_the_weights(records, idx):
    rec = records["shapes"][idx]
    runs = rec["runs"]
    print(json.dumps(rec))
    for name, forced in FORCED.items():
        r = runs[name]
        assert r["oracle"], (name, r)                     # scores, rows (distances) and counts of every query: the CPU oracle's, bit for bit
        assert r["same_as_equal"], (name, r)
        # the queries that overflowed a list or a log region and took the exhaustive pass.  (Not compared: `widened` and with it
        # `candidates` — on the 16-unit shards they differ from call to call with the SAME deal, before this rule existed too.)
        assert r["fallback"] == runs["equal"]["fallback"], (name, r, runs["equal"])
        if rec["shape"][0] <= 8192:      # sampled whole: no filter tile, no resident-query launch, no deal
            continue
        assert r["tier"] == _lib.TIER_I8, (name, r)
        assert r["weights"] is not None and all(abs(a - b) < 1e-4 for a, b in zip(r["weights"], forced)), (name, r)
        _check_off(r["off"], r["units"])
    # the forced weights did deal differently wherever an XCD's share is large enough for 8 % of it to be a unit
    units = runs["equal"]["units"] or 0
    if units >= 8 * 13:
        assert runs["clamps"]["off"] != runs["equal"]["off"], runs
        eq = [b - a for a, b in zip(runs["equal"]["off"], runs["equal"]["off"][1:])]
        for name in ("clamps", "one_min"):
            cnt = [b - a for a, b in zip(runs[name]["off"], runs[name]["off"][1:])]
            assert all(abs(c - e) <= CLAMP * units / 8 + 1 for c, e in zip(cnt, eq)), (name, cnt, eq)
    if units >= 8 * 32:     # (7 % of an eighth of the units is two units or more: it shows through the rounding)
        one = [b - a for a, b in zip(runs["one_min"]["off"], runs["one_min"]["off"][1:])]
        assert one[3] == min(one) and one[3] < eq[3], (one, eq)


def test_three_calls_with_feedback_keep_the_weights_inside_the_clamp_and_the_results(records):
    fb = records["feedback"]
    print(json.dumps(fb))
    assert len(fb["calls"]) == 3
    first = fb["calls"][0]
    assert first["weights"] == [1.0] * 8, first            # a context's first call: equal weights
    for c in fb["calls"]:
        assert c["tier"] == _lib.TIER_I8 and c["same_as_first"] and c["fallback"] == first["fallback"], c
        assert all(1.0 - CLAMP - 1e-4 <= w <= 1.0 + CLAMP + 1e-4 for w in c["weights"]), c
        _check_off(c["off"], c["units"])
    assert fb["same_as_equal"]
