"""The shard merge (merge_topk_kernel) and the sharded search held to a whole-corpus oracle on the GPU.

Two randomised harnesses run in child processes under their own timeouts with pinned seeds — tests/stress_merge.py (the
kernel alone on synthetic records, against the model of tests/_merge_model.py, whose authority is the CPU pin of
tests/test_merge_model_cpu.py) and tests/stress_sharded.py (search + exchange + merge through ShardedScan, against the
oracle over the unsplit corpus) — and must reach every path they name at least FLOOR times; the same floors are checked
without a GPU by tests/test_merge_model_cpu.py (--dry-run).  A few scripted cases stay in-process so that a failure names
itself.

Wall times: NOT yet measured on an MI355X (MEASURED_S below is empty; docs/LAB_NOTES.md says the same).  What is known is
the host side of each run, which no device shortens: stress_merge 13 s (the model on 3000 cases) plus its uploads,
stress_sharded 16 s to draw the cases plus about 45 s in the oracle for its 2567 whole-corpus searches.  The child-process
timeouts are set from those with a wide margin (600 s and 1200 s: more than ten times the host side); once a device run is
recorded they must be at least four times the measured wall time, rounded up to a minute.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _merge_model as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE_CASES, MERGE_SEED = 3000, 1
SHARDED_CASES, SHARDED_SEED = 120, 1
FLOOR = 5
MEASURED_S = {"stress_merge": None, "stress_sharded": None}       # wall seconds of the pinned runs on an MI355X
MERGE_TIMEOUT_S, SHARDED_TIMEOUT_S = 600, 1200
NO_PART = (1 << 64) - 1
FLAG_DEFER = 1


def check_merge_summary(res):
    assert res["cases"] == MERGE_CASES and res["seed"] == MERGE_SEED and res["mismatches"] == 0, res
    assert res["merges"] >= 3000, res
    low = {p: v for p, v in res["paths"].items() if v < FLOOR}
    assert not low and len(res["paths"]) >= 40, low


def check_sharded_summary(res):
    assert res["cases"] == SHARDED_CASES and res["seed"] == SHARDED_SEED and res["mismatches"] == 0, res
    assert res["cases"] >= 120, res
    low = {p: v for p, v in res["paths"].items() if v < FLOOR}
    assert not low and len(res["paths"]) >= 40, low


def _run_harness(script, cases, seed, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), "--cases", str(cases), "--seed", str(seed)],
                       capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and line, r.stdout[-3000:] + r.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["mode"] == "device", res
    return res


@pytest.mark.timeout(MERGE_TIMEOUT_S + 60)
def test_randomised_merge_stress():
    res = _run_harness("stress_merge.py", MERGE_CASES, MERGE_SEED, MERGE_TIMEOUT_S)
    check_merge_summary(res)
    assert res["arg_checks"] == 15 and res["slots_compared"] > 1_000_000, res


@pytest.mark.timeout(SHARDED_TIMEOUT_S + 60)
def test_randomised_sharded_stress():
    res = _run_harness("stress_sharded.py", SHARDED_CASES, SHARDED_SEED, SHARDED_TIMEOUT_S)
    check_sharded_summary(res)
    assert res["batches"] >= SHARDED_CASES and res["compared_queries"] >= 1000 and res["scripted_checks"] == 2, res


# ---- scripted cases ---------------------------------------------------------------------------------------------------
def _device_merge(acc, shards, k, metric, thr=-np.inf, table=None, base=0, flags=0, entry="records", pad=0, want_dist=True):
    """One merge on the device from per-shard dicts (the model's input); returns what the model returns.  Outputs are
    pre-filled with a sentinel, so padding is the kernel's."""
    n_shards, nq = len(shards), len(shards[0]["counts"])
    has_dist, has_ranks = "dist" in shards[0], "ranks" in shards[0]
    keep = []
    up = lambda x: keep.append(acc.to_device(np.ascontiguousarray(x))) or keep[-1]
    o_s, o_r = up(np.full(nq * k, 0xDEADBEEF, np.uint32)), up(np.full(nq * k, -7777, np.int64))
    o_c, o_d = up(np.full(nq, 0xDEADBEEF, np.uint32)), up(np.full(nq * k, 0xDEADBEEF, np.uint32))
    stack = lambda name, dt: np.stack([np.asarray(s[name], dt).reshape((nq, k) if name != "counts" else (nq,)) for s in shards])
    if entry == "records":
        lay = acc.record_layout(nq, k, has_dist, has_ranks)
        stride = lay.bytes + pad
        buf = np.full(n_shards * stride // 8, int(shards[0]["rows"].flat[0]), np.int64).view(np.uint8)
        for i in range(n_shards):
            for name, dt, off in (("scores", np.float32, lay.scores_off), ("rows", np.int64, lay.rows_off), ("counts", np.uint32, lay.counts_off),
                                  ("dist", np.float32, lay.dist_off), ("ranks", np.uint32, lay.ranks_off)):
                if off != NO_PART:
                    raw = stack(name, dt)[i].reshape(-1).view(np.uint8)
                    buf[i * stride + off:i * stride + off + raw.size] = raw
        d_t = up(table) if table is not None else None
        acc.merge_records_device(n_shards, nq, k, thr, metric, up(buf).ptr, stride, lay, d_t.ptr if d_t else None, base,
                                 o_s.ptr, o_r.ptr, o_c.ptr, o_d.ptr if want_dist else None, flags=flags)
    else:
        assert table is None
        acc.merge_topk_device(n_shards, nq, k, thr, metric, up(stack("scores", np.float32)).ptr, up(stack("rows", np.int64)).ptr,
                              up(stack("counts", np.uint32)).ptr, up(stack("dist", np.float32)).ptr if has_dist else None,
                              up(stack("ranks", np.uint32)).ptr if has_ranks else None, o_s.ptr, o_r.ptr, o_c.ptr,
                              o_d.ptr if want_dist else None, flags=flags)
    acc.synchronize()
    out = (o_s.download(np.float32, nq * k).reshape(nq, k), o_r.download(np.int64, nq * k).reshape(nq, k), o_c.download(np.uint32, nq),
           o_d.download(np.float32, nq * k).reshape(nq, k))
    for b in keep:
        b.free()
    return out


def _same(got, want, dist=True):
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:4].tolist()
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    if dist:
        assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32))


def _random_shards(rng, n_shards, nq, k, tie_heavy=True):
    ids = rng.permutation(n_shards * nq * k).reshape(n_shards, nq, k).astype(np.int64)
    shards = []
    for s in range(n_shards):
        sc = rng.choice(np.array([0.0, -0.0, 0.5, 1.0, -1.0, 0.25], np.float32), (nq, k)) if tie_heavy else rng.standard_normal((nq, k)).astype(np.float32)
        di = np.abs(rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), (nq, k))) if tie_heavy else np.abs(rng.standard_normal((nq, k))).astype(np.float32)
        shards.append({"scores": sc, "rows": ids[s], "counts": rng.integers(0, k + 1, nq).astype(np.uint32), "dist": di})
    return shards


@pytest.mark.parametrize("n_shards,k", [(8, 1024), (64, 128)])
@pytest.mark.parametrize("metric", [mm.COSINE, mm.L2])
def test_merge_at_the_limit_of_8192_entries(acc, n_shards, k, metric):
    """n_shards * k == 8192 exactly, both ways the issue names, through both entry points; one entry more is refused."""
    from yams_amd import _lib
    rng = np.random.default_rng(8192 + n_shards + metric)
    shards = _random_shards(rng, n_shards, 3, k)
    shards[0]["counts"][:] = k; shards[-1]["counts"][:] = k            # the first and the last element are alive
    want = mm.merge(shards, k, metric, threshold=0.25)
    _same(_device_merge(acc, shards, k, metric, 0.25, entry="records", pad=24), want)
    _same(_device_merge(acc, shards, k, metric, 0.25, entry="dense"), want)
    one_more = _random_shards(rng, 1, 1, 8193)
    for entry in ("records", "dense"):
        with pytest.raises(_lib.AccelError) as e:
            _device_merge(acc, one_more, 8193, metric, entry=entry)
        assert e.value.status == _lib.YAMS_ERR_UNSUPPORTED


def test_records_own_ranks_beat_rank_of_row(acc):
    """Two shards, every similarity equal; the records' ranks say row 40 < 30 < 20 < 10, the rank_of_row table says the
    opposite and the row ids a third thing: the records' ranks decide (the header's order of precedence).  Without the
    records' ranks the table decides; without either, the row id."""
    k = 2
    mk = lambda rows, ranks: {"scores": np.full((1, k), 0.5, np.float32), "rows": np.array([rows], np.int64) + 1000,
                              "counts": np.array([k], np.uint32), "ranks": np.array([ranks], np.uint32)}
    shards = [mk([30, 10], [1, 3]), mk([40, 20], [0, 2])]
    table = np.zeros(64, np.uint32); table[[10, 20, 30, 40]] = [5, 1, 9, 7]      # by the table: 20 < 10 < 40 < 30
    got = _device_merge(acc, shards, k, mm.COSINE, table=table, base=1000)
    assert got[1].tolist() == [[1040, 1030]] and got[2].tolist() == [2]
    _same(got, mm.merge(shards, k, mm.COSINE, rank_of_row=table, rank_row_base=1000))
    bare = [{x: s[x] for x in ("scores", "rows", "counts")} for s in shards]
    got = _device_merge(acc, bare, k, mm.COSINE, table=table, base=1000)
    assert got[1].tolist() == [[1020, 1010]]
    got = _device_merge(acc, bare, k, mm.COSINE)
    assert got[1].tolist() == [[1010, 1020]] and got[3].tolist() == [[0.5, 0.5]]     # (1 - score: no distances came in)
    # under L2 neither kind of rank plays a part: equal distances come back in row order
    l2 = [dict(s, dist=np.full((1, k), 2.0, np.float32)) for s in shards]
    got = _device_merge(acc, l2, k, mm.L2, table=table, base=1000)
    assert got[1].tolist() == [[1010, 1020]]


def test_l2_threshold_cuts_inside_the_merged_list_and_what_defer_does(acc):
    """"The k nearest, then the threshold": the cut falls inside the merged top k, the survivors keep their order and the
    freed slots are padding — NOT refilled with nearer-than-nothing entries from behind position k.  With
    YAMS_SCAN_FLAG_DEFER_THRESHOLD merge_records drops nothing; merge_topk ignores the flag (pinned as it is today)."""
    k = 4
    a = {"scores": np.array([[0.9, 0.1, 0.8, 0.7]], np.float32), "rows": np.array([[1, 2, 3, 4]], np.int64),
         "counts": np.array([4], np.uint32), "dist": np.array([[0.1, 0.2, 0.5, 0.6]], np.float32)}
    b = {"scores": np.array([[0.2, 0.95, 0.99, 0.0]], np.float32), "rows": np.array([[11, 12, 13, 14]], np.int64),
         "counts": np.array([3], np.uint32), "dist": np.array([[0.15, 0.3, 0.55, -np.inf]], np.float32)}
    # the 4 nearest: rows 1 (0.9), 11 (0.2), 2 (0.1), 12 (0.95); threshold 0.5 keeps rows 1 and 12
    for entry in ("records", "dense"):
        got = _device_merge(acc, [a, b], k, mm.L2, 0.5, entry=entry)
        assert got[2].tolist() == [2] and got[1].tolist() == [[1, 12, -1, -1]], (entry, got)
        assert got[3][0, :2].tolist() == [np.float32(0.1), np.float32(0.3)] and np.isposinf(got[3][0, 2:]).all() and np.isneginf(got[0][0, 2:]).all()
        _same(got, mm.merge([a, b], k, mm.L2, 0.5))
    got = _device_merge(acc, [a, b], k, mm.L2, 0.5, entry="records", flags=FLAG_DEFER)
    assert got[1].tolist() == [[1, 11, 2, 12]] and got[2].tolist() == [4]
    _same(got, mm.merge([a, b], k, mm.L2, 0.5, defer=True))
    got = _device_merge(acc, [a, b], k, mm.L2, 0.5, entry="dense", flags=FLAG_DEFER)
    assert got[1].tolist() == [[1, 12, -1, -1]] and got[2].tolist() == [2]           # merge_topk: the flag is ignored


@pytest.mark.parametrize("metric", [mm.COSINE, mm.L2])
def test_query_that_is_empty_in_every_shard(acc, metric):
    """Query 1 of 3 has count 0 in all five shards (its slots hold decoys): count 0 and nothing but padding, while its
    neighbours merge as usual — with out_dist and without."""
    rng = np.random.default_rng(3)
    k = 6
    shards = _random_shards(rng, 5, 3, k)
    for s in shards:
        s["counts"][1] = 0
        s["scores"][1] = np.inf; s["dist"][1] = -np.inf
    want = mm.merge(shards, k, metric, threshold=0.25)
    for entry in ("records", "dense"):
        got = _device_merge(acc, shards, k, metric, 0.25, entry=entry)
        _same(got, want)
        assert got[2][1] == 0 and (got[1][1] == -1).all() and np.isneginf(got[0][1]).all() and np.isposinf(got[3][1]).all()
        got = _device_merge(acc, shards, k, metric, 0.25, entry=entry, want_dist=False)
        _same(got, want, dist=False)
        assert (got[3].view(np.uint32) == 0xDEADBEEF).all()                          # a null out_dist: nothing written
