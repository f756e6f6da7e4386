"""Entity-vector search on the device (yams_scan_entity_topk_device, vector_entity_scan_v1): every comparison goes through
_entity_oracle.compare — counts, matching rows, score bits (the sign of a zero included), rows under the device's order rule,
and separately what the reference alone guarantees.  The inputs hold ties, zero / NaN / inf rows and queries on purpose: the
device's rule is total, no case is skipped."""
import ctypes as C

import numpy as np
import pytest

import _entity_oracle as eo
from test_entity_cpu import build_entity_index_test, special_queries, special_rows
from yams_amd import _lib

pytestmark = pytest.mark.gpu


def attributes(rng, n, n_node=7, n_doc=40):
    types = rng.integers(0, 4, n).astype(np.uint8)
    nodes = rng.integers(0, n_node, n).astype(np.uint32)
    docs = rng.integers(0, n_doc, n).astype(np.uint32)
    types[rng.choice(n, max(1, n // 50), replace=False)] = eo.TYPE_UNSET
    nodes[rng.choice(n, max(1, n // 50), replace=False)] = eo.UNSET
    docs[rng.choice(n, max(1, n // 50), replace=False)] = eo.UNSET
    return types, nodes, docs


def check(acc, rows, queries, k, thr, attrs=(None, None, None), filters=None, mask_rows=None, row_base=0, qsample=None, rows_offset=0):
    res = eo.run(acc, rows, queries, k, thr, *attrs, filters=filters, mask_rows=mask_rows, row_base=row_base, rows_offset=rows_offset)
    allowed = None if mask_rows is None else np.unique(np.asarray(mask_rows, np.int64))
    assert res.diag["used_exact_scan"] == 1 and res.diag["path"] == 1
    assert res.diag["returned_rows"] == int(res.matching.sum())
    if qsample is None:
        assert res.diag["rows_visited"] == eo.visited_total(rows.shape[0], queries, *attrs, filters, allowed)
    for qi in (range(len(queries)) if qsample is None else qsample):
        why = eo.compare(res, qi, rows, queries, k, thr, *attrs, filters=filters, allowed=allowed, row_base=row_base)
        assert why is None, (qi, why)
    return res


@pytest.mark.parametrize("d,offset", [(384, 0), (768, 0), (1024, 0), (3, 0), (50, 0), (770, 0), (128, 1), (50, 1)])
def test_dims_and_unaligned_rows_with_the_special_rows_and_queries(acc, d, offset):
    rng = np.random.default_rng(d + offset)
    rows = special_rows(rng, 1500, d)
    queries = np.stack(special_queries(rng, d, rows))
    for thr in (-1.0, 0.0, 0.02):
        check(acc, rows, queries, 25, thr, rows_offset=offset)


def test_zero_query_over_nan_rows_returns_the_first_rows_with_plus_zero(acc):
    rng = np.random.default_rng(1)
    rows = special_rows(rng, 900, 96)
    rows[20:40, 5] = np.nan
    r = check(acc, rows, np.zeros((1, 96), np.float32), 50, 0.0)
    assert r.rows[0].tolist() == list(range(50)) and (r.scores[0].view(np.uint32) == 0).all() and int(r.matching[0]) == 900


@pytest.mark.parametrize("n", [1, 63, 64, 257, 4097, 300_000])
def test_row_counts(acc, n):
    rng = np.random.default_rng(n)
    d = 64 if n > 10_000 else 96
    rows = rng.standard_normal((n, d)).astype(np.float32)
    if n > 20:
        rows[10:14] = rows[3]
    queries = rng.standard_normal((3, d)).astype(np.float32)
    queries[0] = rows[min(3, n - 1)] * np.float32(2.0)
    check(acc, rows, queries, 10, -1.0, qsample=None if n < 100_000 else [0, 2])


@pytest.mark.parametrize("nq", [1, 2, 4, 5, 8, 9, 17])
def test_query_group_forms_with_a_filter_per_query(acc, nq):
    rng = np.random.default_rng(50 + nq)
    n, d = 6000, 64
    rows = special_rows(rng, n, d)
    attrs = attributes(rng, n)
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    queries[nq - 1] = rows[0] * np.float32(0.5)
    pool = [(None, None, None), (1, None, None), (None, 3, None), (None, None, 11), (2, 3, None), (0, 1, 5), (None, None, 9999),
            (eo.TYPE_UNSET, None, None)]
    filters = [pool[(i * 3 + nq) % len(pool)] for i in range(nq)]
    check(acc, rows, queries, 30, -1.0, attrs, filters)
    check(acc, rows, queries, 30, 0.05, attrs, filters, mask_rows=np.nonzero(rng.random(n) < 0.5)[0], row_base=1 << 33)


def test_each_filter_alone_all_together_and_none_matching(acc):
    rng = np.random.default_rng(7)
    n, d = 20_000, 96
    rows = special_rows(rng, n, d)
    attrs = attributes(rng, n)
    q = rng.standard_normal((1, d)).astype(np.float32)
    for f in [(2, None, None), (None, 4, None), (None, None, 17), (2, 4, 17), (None, None, 4242), (None, eo.UNSET, None)]:
        for mask in (None, np.nonzero(rng.random(n) < 0.3)[0], np.zeros(0, np.int64)):
            check(acc, rows, q, 20, -1.0, attrs, [f], mask_rows=mask, row_base=5)
    # every query carries a filter (the compacted form) and one query carries none (every row is an item)
    q4 = rng.standard_normal((4, d)).astype(np.float32)
    check(acc, rows, q4, 20, -1.0, attrs, [(1, None, None), (None, None, 3), (1, None, None), (3, 2, None)])
    check(acc, rows, q4, 20, -1.0, attrs, [(1, None, None), (None, None, None), (None, None, 3), (3, 2, None)])
    check(acc, rows, q4, 20, -1.0, attrs, None, mask_rows=np.nonzero(rng.random(n) < 0.01)[0])
    check(acc, rows, q4, 20, -1.0, (attrs[0], None, None), [(1, None, None)] * 4)      # columns no filter names may be null


def test_k_edges_row_base_and_more_than_one_query_slice(acc):
    rng = np.random.default_rng(9)
    n, d = 3000, 48
    rows = special_rows(rng, n, d)
    queries = rng.standard_normal((3, d)).astype(np.float32)
    r = eo.run(acc, rows, queries, 0, -1.0)
    assert (r.counts == 0).all() and r.scores.shape == (3, 0)
    check(acc, rows, queries, 1024, -1.0, row_base=1_000_000)                           # k = YAMS_SCAN_MAX_K
    check(acc, rows[:100], queries, 1024, -1.0)                                         # k > n
    r = check(acc, rows, queries, 10, 1.5)                                              # above every score
    assert (r.counts == 0).all() and (r.matching == 0).all()
    r = check(acc, rows, queries, 10, float("nan"))
    assert (r.counts == 0).all()
    # 600 000 rows x 8 bytes: 55 queries fit 256 MiB, a slice holds 48 (whole groups of 8), 70 queries leave a last slice of 22
    n2, d2 = 600_000, 16
    rows2 = rng.standard_normal((n2, d2)).astype(np.float32)
    q2 = rng.standard_normal((70, d2)).astype(np.float32)
    attrs = attributes(rng, n2)
    filters = [(None, None, None) if i % 2 else (i % 4, None, None) for i in range(70)]
    check(acc, rows2, q2, 15, 0.3, attrs, filters, qsample=[0, 47, 48, 49, 69])


def test_refusals_leave_the_context_usable(acc):
    rng = np.random.default_rng(11)
    n, d = 2000, 32
    rows = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((2, d)).astype(np.float32)
    types = rng.integers(0, 4, n).astype(np.uint8)
    with pytest.raises(_lib.AccelError) as e:                                           # a filter names a null column
        eo.run(acc, rows, queries, 5, -1.0, types, None, None, filters=[(1, None, None), (None, 2, None)])
    assert e.value.status == _lib.YAMS_ERR_INVALID_ARG
    with pytest.raises(_lib.AccelError) as e:
        eo.run(acc, rows, queries, 1025, -1.0)
    assert e.value.status == _lib.YAMS_ERR_UNSUPPORTED
    d_rows = acc.to_device(rows)
    try:
        with pytest.raises(_lib.AccelError) as e:
            acc.scan_entity_topk(acc.corpus_view(d_rows.ptr, n, d, stripe_rows=1024, n_stripes=3), acc.entities_view(), queries, 5, -1.0)
        assert e.value.status == _lib.YAMS_ERR_UNSUPPORTED
    finally:
        d_rows.free()
    check(acc, rows, queries, 5, -1.0, (types, None, None), [(1, None, None), (None, None, None)])


def _u32(a):
    return np.ascontiguousarray(a, np.uint32).ctypes.data_as(_lib.u32p)


def test_through_the_plugin(accel_lib, acc):
    L = accel_lib
    L.yams_plugin_shutdown()
    assert L.yams_plugin_init(b'{"device": 0}', None) == 0
    try:
        p = C.c_void_p(); pe = C.c_void_p()
        assert L.yams_plugin_get_interface(b"vector_scan_v1", 2, C.byref(p)) == 0
        assert L.yams_plugin_get_interface(b"vector_entity_scan_v1", 1, C.byref(pe)) == 0
        vs = C.cast(p, C.POINTER(_lib.VectorScanV1)).contents
        es = C.cast(pe, C.POINTER(_lib.VectorEntityScanV1)).contents
        rng = np.random.default_rng(4)
        n1, n2, d, k = 5000, 2500, 128, 12
        rows = special_rows(rng, n1 + n2, d)
        types, nodes, docs = attributes(rng, n1 + n2)
        queries = rng.standard_normal((3, d)).astype(np.float32)
        filt = [(1, None, None), (None, None, None), (None, 2, 7)]
        fl = (_lib.EntityFilter * 3)(*[_lib.EntityFilter((1 if t is not None else 0) | (2 if nt is not None else 0) | (4 if dc is not None else 0),
                                                         t or 0, nt or 0, dc or 0) for t, nt, dc in filt])

        def search(kk=k, thr=-1.0, words=None, q=queries):
            hits = C.POINTER(_lib.ScanHit)(); counts = _lib.u32p(); diag = _lib.ScanDiag(); matching = np.zeros(len(q), np.uint64)
            qq = np.ascontiguousarray(q, np.float32)
            st = es.search_entities(None, cid, qq.ctypes.data_as(_lib.f32p), fl, len(q), q.shape[1], kk, thr,
                                    _u32(words) if words is not None else None, C.byref(hits), C.byref(counts),
                                    matching.ctypes.data_as(_lib.u64p), C.byref(diag))
            if st != 0:
                return st
            out = [([hits[qi * kk + i].row for i in range(counts[qi])],
                    np.array([hits[qi * kk + i].similarity for i in range(counts[qi])], np.float32)) for qi in range(len(q))]
            es.free_entity_hits(None, hits, counts)
            return out, matching

        def same(got, n, ty, nd, dc, allowed=None, thr=-1.0):
            out, matching = got
            for qi in range(3):
                e_rows, e_sc, _, e_match = eo.expected(rows[:n], queries[qi], k, thr, ty, nd, dc, filt[qi], allowed)
                assert out[qi][0] == e_rows.tolist() and int(matching[qi]) == e_match, qi
                assert np.array_equal(out[qi][1].view(np.uint32), e_sc.view(np.uint32)), qi

        unset = lambda n: (np.full(n, eo.TYPE_UNSET, np.uint8), np.full(n, eo.UNSET, np.uint32), np.full(n, eo.UNSET, np.uint32))
        cid = C.c_uint64()
        assert vs.corpus_create(None, d, C.byref(cid)) == 0
        empty = search()                                                                 # a fresh corpus: empty results, filters or not
        assert not isinstance(empty, int) and all(len(o[0]) == 0 for o in empty[0]) and not empty[1].any()
        assert vs.corpus_append(None, cid, np.ascontiguousarray(rows[:n1]).ctypes.data_as(_lib.f32p), n1) == 0
        same(search(), n1, *unset(n1))                                                   # no attributes yet: only query 1 finds rows
        assert vs.corpus_append(None, cid, np.ascontiguousarray(rows[n1:]).ctypes.data_as(_lib.f32p), n2) == 0
        # two ranges after two appends; the rows between them stay unset
        a, b = 3000, 6000
        t8 = np.ascontiguousarray(types)
        assert es.corpus_set_attributes(None, cid, 0, a, t8[:a].ctypes.data_as(_lib.u8p), _u32(nodes[:a]), _u32(docs[:a])) == 0
        assert es.corpus_set_attributes(None, cid, b, n1 + n2 - b, t8[b:].ctypes.data_as(_lib.u8p), _u32(nodes[b:]), _u32(docs[b:])) == 0
        assert es.corpus_set_attributes(None, cid, b, n1 + n2, None, None, None) == _lib.YAMS_ERR_INVALID_ARG
        ty, nd, dc = types.copy(), nodes.copy(), docs.copy()
        ty[a:b] = eo.TYPE_UNSET; nd[a:b] = eo.UNSET; dc[a:b] = eo.UNSET
        same(search(), n1 + n2, ty, nd, dc)
        cand = np.nonzero(rng.random(n1 + n2) < 0.4)[0]
        same(search(thr=0.01, words=eo.mask_words(n1 + n2, cand)[0]), n1 + n2, ty, nd, dc, cand, 0.01)
        assert search(q=queries[:, :d - 1]) == _lib.YAMS_ERR_INVALID_ARG
        assert search(kk=1025) == _lib.YAMS_ERR_UNSUPPORTED
        assert vs.corpus_clear(None, cid) == 0                                           # drops the columns
        empty = search()                                                                 # a cleared corpus, filtered queries: empty, OK
        assert not isinstance(empty, int) and all(len(o[0]) == 0 for o in empty[0]) and not empty[1].any()
        assert vs.corpus_append(None, cid, np.ascontiguousarray(rows[:n1]).ctypes.data_as(_lib.f32p), n1) == 0
        same(search(), n1, *unset(n1))
        assert vs.corpus_destroy(None, cid) == 0
        assert search() == _lib.YAMS_ERR_NOT_FOUND
    finally:
        L.yams_plugin_shutdown()


def test_filters_over_an_empty_table_or_an_empty_mask_give_empty_results(acc):
    """No rows: nothing for a column to describe, so a filter that names a null column is served an empty result."""
    q = np.ones((2, 8), np.float32)
    f = [(1, None, None), (None, 2, 3)]
    r = eo.run(acc, np.zeros((0, 8), np.float32), q, 5, -1.0, filters=f)
    assert (r.counts == 0).all() and (r.rows == -1).all() and np.isneginf(r.scores).all() and (r.matching == 0).all()
    rows = np.ones((100, 8), np.float32)
    r = eo.run(acc, rows, q, 5, -1.0, filters=f, mask_rows=np.zeros(0, np.int64))
    assert (r.counts == 0).all() and (r.rows == -1).all()
    types = np.zeros(100, np.uint8)                                                     # a filter that admits nothing: same
    r = check(acc, rows, q, 5, -1.0, (types, None, None), [(3, None, None)] * 2)
    assert (r.counts == 0).all() and r.diag["rows_visited"] == 0


def test_entity_index_adapter_against_a_host_loop():
    """tests/cpp/entity_index_test.cpp: AccelEntityIndex (CRUD, INSERT OR REPLACE, deletes, compaction, filters, a string
    never interned, rounds above YAMS_SCAN_MAX_K) against a host loop with the same arithmetic."""
    import subprocess
    from yams_amd import build as b
    b.build()
    r = subprocess.run([build_entity_index_test(), b.LIB], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "OK (0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_randomised_entity_stress():
    """tests/stress_entity.py in a child process under its own timeout: random shapes, filters, masks, special rows and
    queries; the first mismatch ends it with a non-zero exit; every code path must have been reached."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "stress_entity.py"), "--cases", "150", "--seed", "3"],
                       capture_output=True, text=True, timeout=280)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["cases"] == 150 and res["mismatches"] == 0 and res["checked_queries"] >= 150, res
    assert all(v > 0 for v in res["paths"].values()), res["paths"]
