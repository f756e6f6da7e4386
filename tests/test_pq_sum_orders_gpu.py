"""The 25 orders of the ADC sum (YAMS_PQ_SUM_*: lanes | combine | tail) on the device, in both ADC kernels, against the numpy
restatement tests/_pq_sum.py: rows, score bits and counts.  Every case is built so that the ORDER of the additions decides
which rows come back (a family of permuted codes across the approxK cut); tests/test_pq_calibration_cpu.py holds each
scripted case to _pq_sum.discriminates() — the expected rows under the tested definition differ from those under every
definition that is another function at that m, so a kernel that adds in any other served order fails here."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _pq_sum as S
from yams_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRESS_CASES, STRESS_SEED = 100, 5

unfiltered_case = functools.lru_cache(maxsize=None)(S.unfiltered_case)
filtered_case = functools.lru_cache(maxsize=None)(S.filtered_case)
IDS = [S.name(f) for f in S.definitions()]


def search(acc, case, **order):
    d_rows = acc.to_device(case.corpus)
    bufs = [d_rows]
    tie_p = inv_p = None
    if case.rank is not None:
        inv = np.empty_like(case.rank); inv[case.rank] = np.arange(case.rank.size, dtype=np.uint32)
        bufs += [acc.to_device(case.rank), acc.to_device(inv)]
        tie_p, inv_p = bufs[1].ptr, bufs[2].ptr
    try:
        v = acc.corpus_view(d_rows.ptr, case.corpus.shape[0], case.dim, tie_rank_ptr=tie_p, rank_row_ptr=inv_p)
        return acc.scan_pq_topk(v, case.codes, case.luts, case.queries, case.k, case.thr, case.rf, tie_keys=case.keys,
                                row_of_index=case.roi, candidates=case.cand, **order)
    finally:
        for b in bufs:
            b.free()


def same(r, case, flags):
    for qi, (rows, sims) in enumerate(S.expected(case, flags)):
        cnt = int(r.counts[qi])
        assert cnt == len(rows), (S.name(flags), qi, cnt, len(rows), r.diag)
        assert r.rows[qi, :cnt].tolist() == rows, (S.name(flags), qi, r.diag)
        assert np.array_equal(r.scores[qi, :cnt].view(np.uint32), np.array(sims, np.float32).view(np.uint32)), (S.name(flags), qi)


@pytest.mark.parametrize("flags", S.definitions(), ids=IDS)
@pytest.mark.parametrize("m", S.UNFILTERED_M)
def test_unfiltered_form_under_every_definition(acc, m, flags):
    """pq_adc_keys_kernel: 2048 codes, a family of 512, 5 queries (a partial query group), k = 256, rerank factor 1."""
    case = unfiltered_case(m)
    r = search(acc, case, sum_flags=flags)
    assert r.diag["exact_fallback_queries"] == case.nq, r.diag          # all through the unfiltered form
    same(r, case, flags)


@pytest.mark.parametrize("flags", S.definitions(), ids=IDS)
@pytest.mark.parametrize("m", S.FILTERED_M)
def test_filtered_form_under_every_definition(acc, m, flags):
    """pq_adc_filter_kernel, sample and scan: 70 000 codes and a family of 400 on top, 9 queries, k = 100, rerank factor 2."""
    case = filtered_case(m)
    r = search(acc, case, sum_flags=flags)
    assert r.diag["exact_fallback_queries"] == 0, r.diag                # every query was served by the filtered form
    same(r, case, flags)


def test_candidates_tie_keys_and_a_row_map_under_a_new_order(acc):
    case = S.combined_case()
    same(search(acc, case, sum_flags=S.COMBINED_FLAGS), case, S.COMBINED_FLAGS)


@pytest.mark.parametrize("flags", S.OVERFLOW_FLAGS, ids=[S.name(f) for f in S.OVERFLOW_FLAGS])
def test_overflow_follows_the_order_too(acc, flags):
    """+-3e38 entries: sequentially the family sums to +inf (and leads), as halves it stays finite, as x4 pairs it is
    inf - inf: not a number, and such rows are left out."""
    case = S.overflow_case()
    same(search(acc, case, sum_flags=flags), case, flags)


def test_flag_words_0_to_3_are_the_four_lane_counts(acc):
    case = unfiltered_case(40)
    for flags, lanes in ((0, 1), (1, 4), (2, 8), (3, 16)):
        a, b = search(acc, case, sum_flags=flags), search(acc, case, sum_lanes=lanes)
        assert np.array_equal(a.counts, b.counts) and np.array_equal(a.rows, b.rows)
        assert np.array_equal(a.scores.view(np.uint32), b.scores.view(np.uint32))
        same(a, case, flags)
    # bits above YAMS_PQ_SUM_ORDER_MASK are ignored, as they always were
    same(search(acc, case, sum_flags=0xFFFFFFE0 | S.X8 | S.HALVES), case, S.X8 | S.HALVES)
    same(search(acc, case, sum_flags=0x20), case, S.SEQ)


def test_one_lane_with_a_combine_or_tail_bit_is_refused_and_nothing_is_written(acc):
    case = unfiltered_case(32)
    nq, k, n, m = case.nq, 10, case.n, case.m
    guard = 64
    corpus = np.random.default_rng(9).standard_normal((n, case.dim)).astype(np.float32)      # (index i is row i here)
    keep = [acc.to_device(corpus), acc.to_device(case.codes), acc.to_device(case.queries), acc.to_device(case.luts)]
    pat = {}
    for nm, nbytes in (("scores", nq * k * 4), ("rows", nq * k * 8), ("counts", nq * 4)):
        pat[nm] = np.random.default_rng(len(nm)).integers(1, 255, nbytes + 2 * guard).astype(np.uint8)
        keep.append(acc.to_device(pat[nm]))
    d_s, d_r, d_n = keep[4:7]
    try:
        v = acc.corpus_view(keep[0].ptr, n, case.dim)
        pq = _lib.ScanPqIndex(keep[1].ptr, n, m, 0, None, None)
        for bad in (S.HALVES, S.PAIRS, S.HALVES4_PAIRS, S.TAIL_SCALAR, S.HALVES | S.TAIL_SCALAR, 0x1C, 0xFFFFFFE0 | S.TAIL_SCALAR):
            prm = _lib.ScanPqParams(k, -1.0, 2, bad)
            diag = _lib.ScanDiag()
            st = acc.L.yams_scan_pq_topk_device(acc.ctx, C.byref(v), C.byref(pq), keep[2].ptr, keep[3].ptr, nq, C.byref(prm), None, 0,
                                                d_s.ptr + guard, d_r.ptr + guard, d_n.ptr + guard, C.byref(diag))
            assert st == _lib.YAMS_ERR_INVALID_ARG, (bad, st)
            for nm, buf in (("scores", d_s), ("rows", d_r), ("counts", d_n)):
                assert np.array_equal(buf.download(np.uint8, pat[nm].size), pat[nm]), (bad, nm)
        # the same call with a served word fills the outputs and leaves the guard words alone; the context is still usable
        prm = _lib.ScanPqParams(k, -1.0, 2, S.X4 | S.HALVES | S.TAIL_SCALAR)
        st = acc.L.yams_scan_pq_topk_device(acc.ctx, C.byref(v), C.byref(pq), keep[2].ptr, keep[3].ptr, nq, C.byref(prm), None, 0,
                                            d_s.ptr + guard, d_r.ptr + guard, d_n.ptr + guard, None)
        assert st == 0
        for nm, buf in (("scores", d_s), ("rows", d_r), ("counts", d_n)):
            got = buf.download(np.uint8, pat[nm].size)
            assert np.array_equal(got[:guard], pat[nm][:guard]) and np.array_equal(got[-guard:], pat[nm][-guard:]), nm
        assert d_n.download(np.uint8, pat["counts"].size)[guard:-guard].view(np.uint32).tolist() == [k] * nq
    finally:
        for b in keep:
            b.free()


def test_search_pq_of_the_plugin_door_passes_a_new_order(accel_lib):
    """vector_scan_v1.search_pq masks its flag word with YAMS_PQ_SUM_ORDER_MASK: a combine and a tail bit reach the device."""
    L = accel_lib
    case = unfiltered_case(40)
    flags = S.X8 | S.HALVES4_PAIRS | S.TAIL_SCALAR
    L.yams_plugin_shutdown()
    assert L.yams_plugin_init(b'{"device": 0}', None) == 0
    try:
        p = C.c_void_p()
        assert L.yams_plugin_get_interface(b"vector_scan_v1", 1, C.byref(p)) == 0
        vt = C.cast(p, C.POINTER(_lib.VectorScanV1)).contents
        cid = C.c_uint64()
        assert vt.corpus_create(None, case.dim, C.byref(cid)) == 0
        assert vt.corpus_append(None, cid, case.corpus.ctypes.data_as(_lib.f32p), case.corpus.shape[0]) == 0
        assert vt.pq_index_set(None, cid, case.codes.ctypes.data_as(_lib.u8p), case.n, case.m, None, case.roi.ctypes.data_as(_lib.u32p)) == 0
        hits = C.POINTER(_lib.ScanHit)(); counts = _lib.u32p(); diag = _lib.ScanDiag()
        for word in (flags, flags | 0x40):
            st = vt.search_pq(None, cid, case.queries.ctypes.data_as(_lib.f32p), case.luts.ctypes.data_as(_lib.f32p), case.nq, case.dim,
                              case.k, case.thr, case.rf, word, None, 0, C.byref(hits), C.byref(counts), C.byref(diag))
            assert st == 0, st
            for qi, (rows, sims) in enumerate(S.expected(case, flags)):
                assert counts[qi] == len(rows), (qi, counts[qi], len(rows))
                assert [hits[qi * case.k + i].row for i in range(len(rows))] == rows, qi
                got = np.array([hits[qi * case.k + i].similarity for i in range(len(rows))], np.float32)
                assert np.array_equal(got.view(np.uint32), np.array(sims, np.float32).view(np.uint32)), qi
            vt.free_hits(None, hits, counts)
        st = vt.search_pq(None, cid, case.queries.ctypes.data_as(_lib.f32p), case.luts.ctypes.data_as(_lib.f32p), case.nq, case.dim,
                          case.k, case.thr, case.rf, S.TAIL_SCALAR, None, 0, C.byref(hits), C.byref(counts), None)
        assert st == _lib.YAMS_ERR_INVALID_ARG, st
        assert vt.corpus_destroy(None, cid) == 0
    finally:
        L.yams_plugin_shutdown()


def test_randomised_sum_order_stress_against_the_restatement():
    """tests/stress_pq_sum.py: 100 seeded cases on one context — a random definition and m, index sizes on both sides of
    65 536, 1 to 9 queries, with and without candidates — under its own time limit; cases that do not discriminate are not
    counted, and at most 10 may be such (tests/test_pq_calibration_cpu.py checks the same seed without a GPU)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stress_pq_sum.py"), "--cases", str(STRESS_CASES), "--seed", str(STRESS_SEED),
                        "--time-limit", "200"], capture_output=True, text=True, timeout=280)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["ran"] == STRESS_CASES and res["mismatches"] == 0 and not res["timed_out"], res
    assert res["counted"] >= STRESS_CASES - 10 and res["filtered_calls"] > 10 and res["unfiltered_calls"] > 10 and res["orders"] == 25, res
