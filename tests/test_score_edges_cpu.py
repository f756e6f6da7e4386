"""CPU side of the score-edge tests: the small-scan harness's draws reach every path it claims (dry run), its comparison
reports every mutation it must (self test), every zero-plateau case tells the reference's float compare from an order
by score bits before any GPU is involved, and restated_path on hand-computed cases."""
import math

import numpy as np
import pytest

import _score_edges as se
import stress_small
from _score_edges import SCAN_COSINE, SCAN_L2

COUNTERS = (["fused", "general", "qb1", "qb4", "ragged_last_chunk", "one_level", "two_level", "survivors_1024",
             "survivors_one_workgroup_over", "zero_plateau_straddles_cut", "valid_rows_below_k", "large_dense",
             "small_sparse_after_large", "record_path", "l2", "thr_neg_zero", "thr_pos_zero"]
            + ["dup_" + w for w in stress_small.DUP_LABELS] + ["mask_" + m for m in stress_small.MASK_KINDS])


@pytest.fixture(scope="module")
def dry_run(oracle):
    """The dry run at the default seed and case count, once; the zero-plateau cases it emitted ride along."""
    zero_cases = []

    def on_case(d, corpus, q, tie, allowed, answers):
        if d["content"] == "zero":
            zero_cases.append((d, {"corpus": corpus, "queries": q, "tie_rank": tie}, allowed))
    res = stress_small.run(dry_run=True, on_case=on_case)
    return res, zero_cases


def test_dry_run_reaches_every_path_at_least_five_times(dry_run):
    res, _ = dry_run
    assert res["cases"] == stress_small.DEFAULT_CASES and res["mismatches"] == 0
    low = {c: res["paths"].get(c, 0) for c in COUNTERS if res["paths"].get(c, 0) < 5}
    assert not low, (low, res["paths"])


def test_compare_reports_every_mutated_answer(oracle):
    assert stress_small.self_test(oracle) == []


def test_every_zero_plateau_case_tells_the_two_orders_apart(dry_run, oracle):
    """From the oracle alone: zeros of both signs inside the returned k and behind it, and the order by score bits (every
    +0.0 ahead of every -0.0) returns a different row set.  The harness's cases whose whole plateau is in play (no mask,
    a threshold that keeps the zeros), and the scripted shapes of the GPU file."""
    _, zero_cases = dry_run
    n_checked = 0
    for d, z, allowed in zero_cases:
        if allowed is not None or d["thr"] > 0.0:
            continue
        assert se.discriminates(oracle, z, d["k"], d["thr"]) is None, d
        n_checked += 1
    assert n_checked >= 5
    for name, (n, dim, nq, k, P, Z) in se.SCRIPTED.items():
        z = se.zero_plateau(1, n, dim, nq, k, P, Z, row_order=name == "sharded")
        assert se.discriminates(oracle, z, k) is None, name
        assert (z["tie_rank"][z["plateau"]][:-1] < z["tie_rank"][z["plateau"]][1:]).all() and z["neg_zero"][0] and not z["neg_zero"][1]


def test_zero_plateau_thresholds(oracle):
    """-1.0, +0.0 and -0.0 keep the plateau (the float compare `sim < threshold` is false for either zero against
    either zero); the smallest positive denormal drops all of it."""
    n, dim, nq, k, P, Z = 400, 32, 3, 12, 4, 30
    z = se.zero_plateau(2, n, dim, nq, k, P, Z)
    rank = z["tie_rank"].astype(np.uint64)
    for qi in range(nq):
        full = [oracle.scan_cosine(z["corpus"], z["queries"][qi], n, t, rank) for t in (-1.0, 0.0, -0.0, se.DENORM_MIN)]
        assert len(full[0][0]) == n and len(full[1][0]) == len(full[2][0]) == P + Z and len(full[3][0]) == P
        assert np.array_equal(full[1][0], full[2][0]) and np.array_equal(full[1][0], full[0][0][:P + Z])
        assert np.array_equal(full[0][0][P:P + Z], z["plateau"])          # the plateau in rank order, whatever the sign
        assert np.array_equal(full[0][1][P:P + Z].view(np.uint32) == 0x80000000, z["neg_zero"])
        assert (full[0][1][P + Z:] <= np.float32(-0.05)).all() and (full[0][1][:P] > 0).all()


@pytest.mark.parametrize("args,want", [
    # (n, dim, nq, k, metric, flags, aligned)
    ((10_000, 384, 1, 10, SCAN_COSINE, 0, True), 1),                 # BASELINE config 1: 40 workgroups x 10 = 400
    ((16_384, 128, 16, 16, SCAN_COSINE, 0, True), 1),                # 64 x 16 = 1024: the limit itself
    ((16_384, 128, 16, 17, SCAN_COSINE, 0, True), 0),                # 64 x 17 = 1088
    ((16_385, 128, 1, 1, SCAN_COSINE, 0, True), 0),
    ((1024, 64, 4, 256, SCAN_L2, 0, True), 1),                       # 4 x 256 = 1024
    ((1025, 64, 4, 256, SCAN_L2, 0, True), 0),                       # 5 x 256
    ((1000, 64, 4, 257, SCAN_COSINE, 0, True), 0),                   # k above 256 even though 4 x 256 fits
    ((1, 32, 1, 256, SCAN_COSINE, 0, True), 1),
    ((0, 32, 1, 5, SCAN_COSINE, 0, True), 0),
    ((5000, 384, 17, 10, SCAN_COSINE, 0, True), 0),                  # 17 queries
    ((5000, 100, 1, 10, SCAN_COSINE, 0, True), 0),                   # dim % 32
    ((5000, 1056, 1, 10, SCAN_COSINE, 0, True), 0),                  # dim > 1024
    ((5000, 1024, 1, 10, SCAN_COSINE, 0, True), 1),
    ((5000, 384, 1, 10, SCAN_COSINE, 0, False), 0),                  # rows not 16-byte aligned
    ((5000, 384, 1, 10, SCAN_COSINE, se.FLAG_FORCE_EXACT, True), 0),
    ((5000, 384, 1, 10, SCAN_COSINE, se.FLAG_F32_FILTER, True), 0),
    ((5000, 384, 1, 10, SCAN_COSINE, se.FLAG_SPLIT_FILTER, True), 0),
    ((5000, 384, 1, 10, SCAN_COSINE, se.FLAG_WIDE_TILE, True), 0),
    ((5000, 384, 1, 10, SCAN_COSINE, se.FLAG_NO_I8_FILTER, True), 0),
    ((5000, 384, 1, 10, SCAN_COSINE, se.FLAG_RESIDENT_QUERIES, True), 0),
    ((5000, 384, 1, 10, SCAN_COSINE, se.FLAG_RECORD_PATH, True), 1),
    ((5000, 384, 1, 10, SCAN_L2, se.FLAG_DEFER_THRESHOLD, True), 1),
    ((5000, 384, 1, 10, SCAN_L2, 256, True), 0),                     # fp32 accumulation, sequential
    ((5000, 384, 1, 10, SCAN_L2, 768 | 2048, True), 0),              # sixteen lanes, fused
    ((5000, 384, 1, 10, SCAN_L2, 2048, True), 1),                    # FUSED alone names no fp32 accumulation (ignored with F64)
    ((5000, 384, 1, 10, SCAN_COSINE, 256, True), 1),                 # the accumulate bits mean nothing under cosine
])
def test_restated_path_by_hand(args, want):
    assert se.restated_path(*args) == want


@pytest.mark.parametrize("args,want", [
    # (n, allowed | None, dim, nq, k, metric, flags, aligned)
    ((10_000, None, 384, 1, 10, SCAN_COSINE, 0, True), 1),           # the fused scan
    ((10_000, None, 384, 17, 10, SCAN_COSINE, 0, True), 0),          # 17 queries, 10000 rows: a filter tier
    ((4095, None, 384, 17, 10, SCAN_COSINE, 0, True), 1),            # fewer than 4096 rows: the exhaustive pipeline
    ((4096, None, 384, 17, 10, SCAN_COSINE, 0, True), 0),
    ((16_384, None, 128, 16, 17, SCAN_COSINE, 0, True), 0),          # one survivor list too many for the fused scan
    ((16_384, 16_383, 128, 16, 17, SCAN_COSINE, 0, True), 1),        # ... behind a mask of fewer than 16384 rows
    ((20_000, 16_384, 128, 16, 17, SCAN_COSINE, 0, True), 0),
    ((20_000, None, 64, 3, 50, SCAN_COSINE, se.FLAG_FORCE_EXACT, True), 1),
    ((20_000, None, 64, 3, 50, SCAN_COSINE, 0, False), 1),           # rows not 16-byte aligned
    ((20_000, None, 37, 3, 50, SCAN_COSINE, 0, True), 1),            # dim % 4
    ((20_000, None, 100, 3, 50, SCAN_COSINE, 0, True), 0),
    ((5000, None, 384, 1, 10, SCAN_L2, 256, True), 0),               # fp32 accumulation steps off the fused scan onto a filter tier
    ((3000, None, 384, 1, 10, SCAN_L2, 256, True), 1),
])
def test_restated_diag_path_by_hand(args, want):
    assert se.restated_diag_path(*args) == want


def test_packed_key_order_is_the_order_by_bits():
    sims = np.array([0.0, -0.0, 0.5, -0.0, 0.0, -1.0], np.float32)
    rows, ranks = np.arange(6), np.array([5, 0, 3, 1, 4, 2], np.uint64)
    r, s = se.packed_key_order(rows, sims, ranks, 4)
    assert r.tolist() == [2, 4, 0, 1] and [math.copysign(1.0, float(x)) for x in s] == [1.0, 1.0, 1.0, -1.0]
