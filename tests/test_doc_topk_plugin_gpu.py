"""vector_doc_scan_v1: document-level top-k through the plugin boundary equals the C ABI call (yams_scan_doc_topk_device)
over the same rows, tie ranks and document map — after the first upload, after a further append (the new rows have no
document until the map is set again) and after corpus_clear + a re-upload.  A corpus dealt to several devices is refused."""
import ctypes as C

import numpy as np
import pytest

from test_doc_topk_gpu import NO_DOC, corpus, layout, run
from yams_amd import _lib

pytestmark = pytest.mark.gpu


def _u32(a):
    return np.ascontiguousarray(a, np.uint32).ctypes.data_as(_lib.u32p)


def _ifaces(L):
    p = C.c_void_p(); pd = C.c_void_p()
    assert L.yams_plugin_get_interface(b"vector_scan_v1", 2, C.byref(p)) == 0
    assert L.yams_plugin_get_interface(b"vector_doc_scan_v1", 1, C.byref(pd)) == 0
    return C.cast(p, C.POINTER(_lib.VectorScanV1)).contents, C.cast(pd, C.POINTER(_lib.VectorDocScanV1)).contents


def _search(ds, cid, queries, k, thr, mask_words=None):
    nq, d = queries.shape
    hits = C.POINTER(_lib.ScanHit)(); counts = _lib.u32p(); diag = _lib.ScanDiag()
    matching = np.zeros(nq, np.uint64)
    q = np.ascontiguousarray(queries, np.float32)
    st = ds.search_docs(None, cid, q.ctypes.data_as(_lib.f32p), nq, d, k, thr, _u32(mask_words) if mask_words is not None else None,
                        C.byref(hits), C.byref(counts), matching.ctypes.data_as(_lib.u64p), C.byref(diag))
    if st != 0:
        return st
    out = [([hits[qi * k + i].row for i in range(counts[qi])],
            np.array([hits[qi * k + i].similarity for i in range(counts[qi])], np.float32),
            np.array([hits[qi * k + i].distance for i in range(counts[qi])], np.float32)) for qi in range(nq)]
    ds.free_doc_hits(None, hits, counts)
    return out, matching, diag


def _same(acc, res, rows, queries, k, thr, row_doc, n_docs, tie, doc_rank, mask_rows=None):
    ref = run(acc, rows, queries, k, thr, row_doc, n_docs, tie, doc_rank, mask_rows)
    out, matching, diag = res
    assert np.array_equal(matching, ref.matching)
    assert diag.rows_visited == ref.diag["rows_visited"] and diag.returned_rows == ref.diag["returned_rows"]
    for qi in range(len(queries)):
        cnt = int(ref.counts[qi])
        assert out[qi][0] == ref.rows[qi, :cnt].tolist(), qi
        assert np.array_equal(out[qi][1].view(np.uint32), ref.scores[qi, :cnt].view(np.uint32)), qi
        assert np.array_equal(out[qi][2], (np.float32(1.0) - ref.scores[qi, :cnt]).astype(np.float32)), qi


def test_doc_scan_through_the_vtable_equals_the_c_abi(accel_lib, acc):
    L = accel_lib
    L.yams_plugin_shutdown()
    assert L.yams_plugin_init(b'{"device": 0}', None) == 0
    try:
        vs, ds = _ifaces(L)
        rng = np.random.default_rng(4)
        n1, n2, d, n_docs, k = 6000, 2500, 256, 300, 12
        rows = corpus(rng, n1 + n2, d)
        row_doc = layout(rng, n1 + n2, n_docs, "contiguous")
        row_doc[rng.choice(n1 + n2, 50, replace=False)] = NO_DOC
        doc_rank = rng.permutation(n_docs).astype(np.uint32)
        queries = rng.standard_normal((5, d)).astype(np.float32)
        cid = C.c_uint64()
        assert vs.corpus_create(None, d, C.byref(cid)) == 0
        assert vs.corpus_append(None, cid, np.ascontiguousarray(rows[:n1]).ctypes.data_as(_lib.f32p), n1) == 0
        tie1 = rng.permutation(n1).astype(np.uint32)
        assert vs.corpus_set_tie_ranks(None, cid, _u32(tie1), n1) == 0
        rd1 = np.ascontiguousarray(row_doc[:n1])
        assert ds.corpus_set_documents(None, cid, _u32(rd1), n1, _u32(doc_rank), n_docs) == 0
        assert ds.corpus_set_documents(None, cid, _u32(rd1), n1 + 1, _u32(doc_rank), n_docs) == _lib.YAMS_ERR_INVALID_ARG
        _same(acc, _search(ds, cid, queries, k, -1.0), rows[:n1], queries, k, -1.0, rd1, n_docs, tie1, doc_rank)
        # a candidate mask (document restriction) crosses the boundary as host words
        cand = np.nonzero(np.isin(rd1, rng.choice(n_docs, 20, replace=False)))[0]
        words = np.zeros((n1 + 31) // 32, np.uint32)
        np.bitwise_or.at(words, cand >> 5, (np.uint32(1) << (cand & 31).astype(np.uint32)))
        _same(acc, _search(ds, cid, queries, k, 0.01, words), rows[:n1], queries, k, 0.01, rd1, n_docs, tie1, doc_rank, cand)
        # a further append: the new rows have no document until the map is set again
        assert vs.corpus_append(None, cid, np.ascontiguousarray(rows[n1:]).ctypes.data_as(_lib.f32p), n2) == 0
        tie = rng.permutation(n1 + n2).astype(np.uint32)
        assert vs.corpus_set_tie_ranks(None, cid, _u32(tie), n1 + n2) == 0
        padded = np.concatenate([rd1, np.full(n2, NO_DOC, np.uint32)])
        _same(acc, _search(ds, cid, queries, k, -1.0), rows, queries, k, -1.0, padded, n_docs, tie, doc_rank)
        assert ds.corpus_set_documents(None, cid, _u32(row_doc), n1 + n2, _u32(doc_rank), n_docs) == 0
        _same(acc, _search(ds, cid, queries, k, -1.0), rows, queries, k, -1.0, row_doc, n_docs, tie, doc_rank)
        # corpus_clear drops the map; a re-upload (compaction) sets it again
        assert vs.corpus_clear(None, cid) == 0
        assert vs.corpus_append(None, cid, np.ascontiguousarray(rows[n2:]).ctypes.data_as(_lib.f32p), n1) == 0
        r = _search(ds, cid, queries, k, -1.0)
        assert all(len(o[0]) == 0 for o in r[0]) and (r[1] > 0).all()
        rd = np.ascontiguousarray(row_doc[n2:])
        assert ds.corpus_set_documents(None, cid, _u32(rd), n1, None, n_docs) == 0
        _same(acc, _search(ds, cid, queries, k, -1.0), rows[n2:], queries, k, -1.0, rd, n_docs, None, None)
        # what the call refuses
        assert _search(ds, cid, queries[:, :d - 1], k, -1.0) == _lib.YAMS_ERR_INVALID_ARG
        assert _search(ds, cid, queries, 1025, -1.0) == _lib.YAMS_ERR_UNSUPPORTED
        assert vs.corpus_destroy(None, cid) == 0
        assert _search(ds, cid, queries, k, -1.0) == _lib.YAMS_ERR_NOT_FOUND
    finally:
        L.yams_plugin_shutdown()


def test_a_corpus_on_several_devices_is_unsupported(accel_lib):
    L = accel_lib
    L.yams_plugin_shutdown()
    assert L.yams_plugin_init(b'{"devices": [0, 0], "stripe_rows": 4096}', None) == 0
    try:
        vs, ds = _ifaces(L)
        rng = np.random.default_rng(8)
        n, d = 10_000, 64
        rows = rng.standard_normal((n, d)).astype(np.float32)
        cid = C.c_uint64()
        assert vs.corpus_create(None, d, C.byref(cid)) == 0
        assert vs.corpus_append(None, cid, rows.ctypes.data_as(_lib.f32p), n) == 0
        rd = (np.arange(n) // 10).astype(np.uint32)
        assert ds.corpus_set_documents(None, cid, _u32(rd), n, None, n // 10) == _lib.YAMS_ERR_UNSUPPORTED
        assert _search(ds, cid, rows[:2], 5, -1.0) == _lib.YAMS_ERR_UNSUPPORTED
        assert vs.corpus_destroy(None, cid) == 0
    finally:
        L.yams_plugin_shutdown()
