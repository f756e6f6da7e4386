"""CPU pins of the host-ingest stress harness (tests/stress_ingest_host.py, tests/_ingest_model.py): the generator reaches
every ledger path with the pinned seed and case count, the comparison names every injected fault, and the batch-partition
model gives the hand-computed answers of the contract in include/yams_mi355x_accel.h.  No GPU."""
import json
import os
import subprocess
import sys

import pytest

import _ingest_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "stress_ingest_host.py")


def _run(*args, timeout=600):
    r = subprocess.run([sys.executable, HARNESS, *args], capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    return r.returncode, json.loads(line[-1])


def test_dry_run_reaches_every_ledger_path():
    rc, res = _run("--dry-run", "--seed", str(im.PINNED_SEED), "--cases", str(im.PINNED_CASES))
    assert rc == 0 and res["mode"] == "dry-run", res
    assert res["cases"] == res["cases_run"] == im.PINNED_CASES and res["mismatches"] == 0
    assert sorted(res["paths"]) == sorted(im.PATHS)
    short = {p: c for p, c in res["paths"].items() if c < im.FLOOR}
    assert not short, short


def test_self_test_names_every_injected_fault():
    rc, res = _run("--self-test")
    assert rc == 0 and res["ok"] and res["clean"] == [], res
    assert sorted(res["faults"]) == sorted(im.FAULTS)
    for fault, r in res["faults"].items():
        assert r["got"] == [r["want"]], (fault, r)
    wants = {r["want"] for r in res["faults"].values()}
    assert wants == {"boundary", "chunk_digest", "blob_digest", "blob_first", "guard:chunk_size", "deferred_not_zero"}


@pytest.mark.parametrize("lens, batch_bytes, flags, batches, slots", [
    # padded 16, 16, 32, 0, 112: 16 + 16 fit 48, the 32 would pass it; the empty blob joins; the 112 is a batch of its own
    ([10, 16, 17, 0, 100], 48, 3, [(0, 2, 32), (2, 2, 32), (4, 1, 112)], 3),
    ([10, 16, 17, 0, 100], 48, 1, [(0, 2, 32), (2, 2, 32), (4, 1, 112)], 2),          # no blob digests: two slots
    ([10, 16, 17, 0, 100], 1, 2, [(0, 1, 16), (1, 1, 16), (2, 1, 32), (3, 1, 0), (4, 1, 112)], 4),   # one blob per batch
    ([10, 16, 17, 0, 100], 176, 7, [(0, 5, 176)], 1),                                  # exactly full: one batch, one slot
    ([10, 16, 17, 0, 100], 175, 0, [(0, 4, 64), (4, 1, 112)], 2),                      # one byte less: the last blob moves
    ([0, 0, 0], 1, 3, [(0, 3, 0)], 1),                                                 # empty blobs never close a batch
    ([100, 0, 0, 5], 64, 3, [(0, 1, 112), (1, 3, 16)], 2),                             # ... unless it is over-full already
    ([1], 1 << 40, 0, [(0, 1, 16)], 1),
    ([32] * 9, 64, 3, [(0, 2, 64), (2, 2, 64), (4, 2, 64), (6, 2, 64), (8, 1, 32)], 4),    # five batches, four slots
    ([32] * 9, 64, 0, [(0, 2, 64), (2, 2, 64), (4, 2, 64), (6, 2, 64), (8, 1, 32)], 2),
    ([], 64, 3, [], 0),
])
def test_partition_model_known_answers(lens, batch_bytes, flags, batches, slots):
    assert im.partition(lens, batch_bytes, flags) == (batches, slots)


def test_merged_runs_are_counted_from_addresses_and_lengths():
    case = {"lens": [32, 0, 48, 20, 16, 16, 64]}
    #        0..32 | empty | 32..80 | 80..100 | 100..116 | (gap) 200..216 | 216..280: everything in one batch
    addrs = [1000, None, 1032, 1080, 1100, 1200, 1216]
    batches, _ = im.partition(case["lens"], 1 << 20, 3)
    # 0+2 merge across the empty blob; 3 follows 2 at a 16-byte position: merges; 4 follows 3 in host memory but 20 is no
    # multiple of 16: neighbours that do not merge; 5 is elsewhere; 6 follows 5: merges
    assert im.upload_runs(case, addrs, batches) == (3, 1, 1)
    # the same blobs, one per batch: nothing can merge
    batches, _ = im.partition(case["lens"], 1, 3)
    assert im.upload_runs(case, addrs, batches)[0] == 0


def test_constants_come_from_the_header_by_name():
    assert im.header_constant("YAMS_HASH_LONE_CHAIN_MAX") == 1 << 20
    assert im.header_constant("YAMS_HASH_CHAIN_RATIO") == 37
    assert im.header_constant("YAMS_INGEST_DEFER_LONG_BLOB_DIGESTS") == im.FLAG_DEFER
    assert im.header_constant("YAMS_CHUNK_MANY_DEFER_LONG_BUFFER_HASHES") == 2
    assert im.defer_threshold_host(0) == 1 << 20 and im.defer_threshold_host(1 << 30) == 1 << 21
