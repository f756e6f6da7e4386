"""The PQ sum-order probe (include/yams_accel/pq_calibration.hpp) and the numpy restatement of the 25 orders (tests/_pq_sum.py),
without a GPU.  tests/cpp/pq_calibration_test.cpp (plain g++, AddressSanitizer + UBSan, its own main) prints what the header
decides; the expected classes, names and bits come from _pq_sum, which is written from the text of yams_mi355x_accel.h."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _pq
import _pq_calib_build
import _pq_sum as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = [32, 8, 16, 64, 40, 7, 100, 128]


def run(*args):
    r = subprocess.run([_pq_calib_build.build_pq_calibration_test(), *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def test_the_names_and_the_preference_order():
    names = [S.name(f) for f in S.definitions()]
    assert len(names) == 25 and len(set(names)) == 25
    assert names[:4] == ["seq", "x4", "x4_tail", "x4_halves"] and names[-1] == "x16_halves4_pairs_tail" and "x8_halves" in names
    assert S.definitions()[:1] == [0] and [f for f in S.definitions() if f < 4 and (f & ~3) == 0] == [0, 1, 2, 3]
    lines = run("classes", 32)                              # the header lists the same 25 in the same order
    assert [ln.split()[0] for ln in lines[::2]] == names


@pytest.mark.parametrize("m", MS)
def test_every_definition_is_recognised_as_its_own_class(m):
    """Each definition plays the host, behind both host shapes: `matching` is exactly the set of definitions that are the same
    function at this m (equal expression trees), `flags` the first of them in preference order."""
    lines = run("classes", m)
    assert len(lines) == 50
    for ln in lines:
        host, shape, matched, flags, *matching = ln.split()
        want = [S.name(f) for f in S.class_of(S.by_name(host), m)]
        assert matched == "1" and flags == want[0] and matching == want, (m, ln, want)


@pytest.mark.parametrize("m", [40, 64, 100, 128])
def test_hosts_whose_order_is_not_served_are_refused(m):
    """Reverse sequential, a recursive pairwise sum over elements, 2 lanes, 32 lanes, an fp64 accumulator rounded once, a
    function that fails, a function that returns NaN.  (m > 32: up to 32 sub-quantisers a 32-lane sum holds one element per
    lane and IS one of the served functions; the program exits non-zero if any of them matched.)"""
    lines = run("refused", m)
    assert len(lines) == 14
    for ln in lines:
        assert ln.split()[1] == "0" and "matches NO served order" in ln, ln
    assert "failed calls 128" in lines[10] and "NaN results 128" in lines[12], lines[10:13]


@pytest.mark.skipif(not _pq_calib_build.has_avx2(), reason="no avx2 in /proc/cpuinfo")
def test_two_avx2_hosts_are_recognised():
    """_mm256_i32gather_ps loops with a scalar tail; one reduces with extract-high / movehl / shuffle, the other with
    extract-high / movehdup / movehl.  At m = 40 (no tail: 40 = 5 * 8) the tail bit changes nothing, so both x8_halves and
    x8_halves_tail reproduce the first host; at m = 44 and 100 only the _tail forms do."""
    a, b = (ln.split() for ln in run("avx2", 40))
    assert a[2] == "1" and "x8_halves_tail" in a[4:] and a[4:] == ["x8_halves", "x8_halves_tail"], a
    assert b[2] == "1" and "x8_halves4_pairs_tail" in b[4:] and b[4:] == ["x8_halves4_pairs", "x8_halves4_pairs_tail"], b
    for m in (44, 100):
        a, b = (ln.split() for ln in run("avx2", m))
        assert a[2:] == ["1", "x8_halves_tail", "x8_halves_tail"], (m, a)
        assert b[2:] == ["1", "x8_halves4_pairs_tail", "x8_halves4_pairs_tail"], (m, b)


@pytest.mark.parametrize("m", [32, 40, 7, 100])
def test_the_headers_definitions_equal_the_restatement_bit_for_bit(m):
    lines = run("--dump", m)
    probes = S.probes(m)
    got = {}
    codes = []
    for ln in lines:
        p = ln.split()
        if p[0] == "code":
            codes.append([int(x) for x in p[2:]])
        else:
            got[(int(p[0]), p[1])] = int(p[2], 16)
    assert len(got) == len(probes) * 25
    for f in S.definitions():
        for i, (tab, code) in enumerate(probes):
            want = int(np.float32(S.adc_sum(f, tab, code)).view(np.uint32))
            assert got[(i, S.name(f))] == want, (m, i, S.name(f))
    assert codes == [c.tolist() for c in S.probe_codes(m)]


def test_pq_search_flags_equals_the_oracle_for_the_four_lane_counts(oracle):
    """The recipe of tests/test_pq_oracle_cpu.py: flags 0 - 3 are the oracle's sum_lanes 1 / 4 / 8 / 16."""
    from test_pq_oracle_cpu import case
    corpus, pq, codes, keys, rank = case(oracle)
    queries = oracle.synth_rows(3, 1 << 40, 4, corpus.shape[1]) * np.float32(3.0)
    for flags, lanes in ((0, 1), (1, 4), (2, 8), (3, 16)):
        for q in queries:
            lut = pq.lut(q)
            for k, rf, thr in ((5, 2, -1.0), (10, 1, -1.0), (10, 4, 0.2), (700, 2, -1.0), (3, 2, 0.9)):
                rows, sims, _ = oracle.pq_search(corpus, codes, lut, q, k, thr, rf, tie_keys=keys, chunk_rank=rank, sum_lanes=lanes)
                nr, ns = S.pq_search_flags(corpus, codes, lut, q, k, thr, rf, keys, None, rank, None, flags)
                assert rows.tolist() == nr, (flags, k, rf, thr)
                assert np.array_equal(sims.view(np.uint32), np.array(ns, np.float32).view(np.uint32))
    # with candidates, a row map that lost rows, and the single-code score
    cand = np.arange(3, corpus.shape[0], 5, dtype=np.uint32)
    roi = np.arange(corpus.shape[0], dtype=np.uint32); roi[[8, 13, 18]] = corpus.shape[0] + 7
    lut = pq.lut(queries[0])
    rows, sims, _ = oracle.pq_search(corpus, codes, lut, queries[0], 12, -1.0, 3, tie_keys=keys, row_of_index=roi, chunk_rank=rank, candidates=cand, sum_lanes=8)
    nr, ns = S.pq_search_flags(corpus, codes, lut, queries[0], 12, -1.0, 3, keys, roi, rank, cand, S.X8)
    assert rows.tolist() == nr and np.array_equal(sims.view(np.uint32), np.array(ns, np.float32).view(np.uint32))
    for flags, lanes in ((0, 1), (1, 4), (2, 8), (3, 16)):
        assert np.float32(oracle.pq_adc_score(codes[5], lut, lanes)).tobytes() == np.float32(S.adc_sum(flags, lut, codes[5])).tobytes()


@pytest.mark.parametrize("m", MS)
def test_the_probes_tell_apart_what_can_be_told_apart(m):
    assert run("distinguishing", m) == ["1"]


def test_every_scripted_gpu_case_discriminates():
    """tests/test_pq_sum_orders_gpu.py's cases: under every definition they are run with, the expected rows differ on at least
    one query from the expected rows under every definition that is another function at that m."""
    for m in S.UNFILTERED_M:
        case, cache = S.unfiltered_case(m), {}
        assert all(S.discriminates(case, f, cache) for f in S.definitions()), ("unfiltered", m)
    for m in S.FILTERED_M:
        case, cache = S.filtered_case(m), {}
        assert all(S.discriminates(case, f, cache) for f in S.definitions()), ("filtered", m)
    assert S.discriminates(S.combined_case(), S.COMBINED_FLAGS)


def test_the_overflow_case_separates_sequential_from_the_lane_forms():
    case = S.overflow_case()
    seq = S.adc_scores(S.SEQ, case.luts[0], case.codes)
    halves = S.adc_scores(S.X4 | S.HALVES, case.luts[0], case.codes)
    pairs = S.adc_scores(S.X4 | S.PAIRS, case.luts[0], case.codes)
    hot = case.members
    assert np.all(np.isinf(seq[hot])) and np.all(np.isfinite(halves[hot])) and np.all(np.isnan(pairs[hot]))
    cold = np.setdiff1d(np.arange(case.n), hot)
    assert np.all(np.isfinite(seq[cold])) and np.all(np.isfinite(pairs[cold]))


def test_the_stress_harness_dry_run_and_self_test():
    """The committed seed of the GPU stress (tests/test_pq_sum_orders_gpu.py) keeps at most 10 of its 100 cases blind."""
    import test_pq_sum_orders_gpu as g
    exe = [sys.executable, os.path.join(ROOT, "tests", "stress_pq_sum.py")]
    r = subprocess.run(exe + ["--self-test"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and json.loads(r.stdout.splitlines()[-1])["self_test"] == "ok", r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run(exe + ["--dry-run", "--cases", str(g.STRESS_CASES), "--seed", str(g.STRESS_SEED)], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.splitlines()[-1])
    assert res["ran"] == g.STRESS_CASES == 100 and len(res["blind"]) <= 10 and res["orders"] == 25, res
