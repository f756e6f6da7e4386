"""Document-level top-k (yams_scan_doc_topk_device, vector_doc_scan_v1) without a GPU: the restatement of the
reference's reduction on hand-computed tie cases, the exported symbol and the interface table, and — where the
reference's own scan is compiled (oracle/_ref) — the input of the reduction pinned on the reference's loop."""
import ctypes as C

import numpy as np
import pytest

from _doc_select import best_per_document


def test_restatement_ties_within_a_document():
    # equal scores inside one document: the smaller chunk_id wins (:99-103), whatever the input order
    rows = [0, 1, 2]
    for perm in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        r = [rows[i] for i in perm]
        s = [np.float32(0.5)] * 3
        c = [["c2", "c0", "c1"][i] for i in perm]
        d = ["A"] * 3
        assert best_per_document(r, s, c, d, 10) == [(1, np.float32(0.5), b"A")]


def test_restatement_ties_across_documents_and_empty_hashes():
    r = [0, 1, 2, 3, 4, 5]
    s = [np.float32(x) for x in (0.9, 0.7, 0.7, 0.7, 0.95, 0.1)]
    c = ["z", "a", "b", "c", "d", "e"]
    d = ["B", "C", "A", "B", "", "C"]       # row 4 (the best score) has no document: dropped
    out = best_per_document(r, s, c, d, 10)
    # B: 0.9 (row 0); C: 0.7 (row 1); A: 0.7 (row 2); equal scores -> document_hash asc (:116-118)
    assert out == [(0, np.float32(0.9), b"B"), (2, np.float32(0.7), b"A"), (1, np.float32(0.7), b"C")]
    assert best_per_document(r, s, c, d, 2) == out[:2]
    assert best_per_document(r, s, c, d, 0) == []
    assert best_per_document([4], [np.float32(1.0)], ["x"], [""], 5) == []


def test_restatement_compares_bytes():
    # std::string order is byte order: "B" < "a", "a" < "aa"
    out = best_per_document([0, 1, 2], [np.float32(0.3)] * 3, ["x", "y", "z"], ["a", "B", "aa"], 3)
    assert [t[2] for t in out] == [b"B", b"a", b"aa"]


def test_doc_topk_symbol_is_exported(accel_lib):
    from yams_amd import _lib
    assert hasattr(accel_lib, "yams_scan_doc_topk_device")
    assert "yams_scan_doc_topk_device" in _lib.EXPORTS


def test_vector_doc_scan_interface(accel_lib):
    from yams_amd import _lib
    L = accel_lib
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"vector_doc_scan_v1", 1, C.byref(p)) == 0
    vt = C.cast(p, C.POINTER(_lib.VectorDocScanV1)).contents
    assert vt.abi_version == 1
    for fname, _ in _lib.VectorDocScanV1._fields_[2:]:
        assert getattr(vt, fname), f"vector_doc_scan_v1.{fname} is NULL"
    for ver in (0, 2):
        q = C.c_void_p()
        assert L.yams_plugin_get_interface(b"vector_doc_scan_v1", ver, C.byref(q)) == -2
        assert q.value is None


def _scan_ref_or_skip():
    import _oracle
    t = _oracle.scan_ref()
    if t is None:
        pytest.skip("oracle/_ref/libyams_scan_ref.so not present (built only where the reference checkout exists)")
    return t


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_all_matching_equals_reference_on_candidate_documents(oracle, seed):
    """The input of the restated reduction: oracle.scan_cosine(rows, q, k=n) over the rows of the candidate documents
    equals the reference-compiled bruteForceSearchUnlocked(AllMatching, candidate_hashes) on rows, score bits and
    counts, under shuffled chunk ids and document hashes."""
    t = _scan_ref_or_skip()
    rng = np.random.default_rng(seed)
    n, d, n_docs = 600, 48, 40
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[rng.choice(n, 30, replace=False)] = rows[rng.choice(n, 30, replace=False)]   # duplicated rows
    rows[5] = 0.0
    ids = [f"c{v:05d}" for v in rng.permutation(n)]                                   # chunk ids out of row order
    names = [f"{v:08x}" for v in rng.integers(0, 2 ** 32, n_docs)]
    doc_of = rng.integers(0, n_docs, n)
    t.insert_rows(rows, chunk_ids=ids, document_hashes=[names[i] for i in doc_of])
    cand = set(names[i] for i in rng.choice(n_docs, 12, replace=False))
    sel = np.array([i for i in range(n) if names[doc_of[i]] in cand], np.int64)
    rank = np.argsort(np.argsort(np.array(ids, dtype=object)[sel])).astype(np.uint64)
    q = rng.standard_normal(d).astype(np.float32)
    for thr in (-1.0, 0.05):
        got = t.search(q, 0, thr, all_matching=True, candidate_hashes=cand)
        assert not isinstance(got, int), got
        r_ords, r_sc, r_dg = got
        o_rows, o_sc, _, _ = oracle.scan_cosine(rows[sel], q, len(sel), thr, tie_rank=rank)
        assert np.array_equal(sel[o_rows], r_ords)
        assert np.array_equal(o_sc.view(np.uint32), r_sc.view(np.uint32))
        assert r_dg["returned_rows"] == len(o_rows) and r_dg["rows_visited"] == len(sel)
        # and the restated reduction over it is what the backend's document mode returns
        best = best_per_document(r_ords, r_sc, [ids[i] for i in r_ords], [names[doc_of[i]] for i in r_ords], 5)
        assert len(best) == min(5, len({names[doc_of[i]] for i in r_ords}))
