"""Document-level top-k on the device (yams_scan_doc_topk_device): every matching row of the allowed set (the oracle's
exact cosine, oracle_exact_scan_cosine with k = all rows) reduced by the restatement of retainBestRecordPerDocument
(tests/_doc_select.py, sqlite_vec_backend.cpp:86-125).  Rows, document ordinals, score bits, order, counts and the
matching-row counts must be identical."""
import numpy as np
import pytest

from _doc_select import best_per_document
from yams_amd import _lib

pytestmark = pytest.mark.gpu

NO_DOC = _lib.NO_DOC


def expected(oracle, rows, q, k, thr, row_doc, tie=None, doc_rank=None, allowed=None):
    """(rows, scores, docs, matching) of one query: the oracle's matching rows, then the restated reduction.  Chunk ids
    and document hashes are the zero-padded ranks, so that byte order is rank order."""
    n = rows.shape[0]
    sel = np.arange(n) if allowed is None else np.asarray(allowed, np.int64)
    tie = np.arange(n, dtype=np.uint64) if tie is None else tie.astype(np.uint64)
    r = oracle.scan_cosine(rows[sel], q, max(len(sel), 1), thr, tie_rank=tie[sel]) if len(sel) else (np.zeros(0, np.int64), np.zeros(0, np.float32), 0, 0)
    assert r is not None
    m_rows, m_sc = sel[r[0]], r[1]
    n_docs = int(row_doc[row_doc != NO_DOC].max()) + 1 if (row_doc != NO_DOC).any() else 0
    rank = np.arange(max(n_docs, 1)) if doc_rank is None else doc_rank
    hashes = ["" if row_doc[i] == NO_DOC else "%010d" % rank[row_doc[i]] for i in m_rows]
    best = best_per_document(m_rows, m_sc, ["%010d" % tie[i] for i in m_rows], hashes, k)
    out_rows = np.array([b[0] for b in best], np.int64)
    return out_rows, np.array([b[1] for b in best], np.float32), row_doc[out_rows] if len(out_rows) else np.zeros(0, np.uint32), len(m_rows)


def run(acc, rows, queries, k, thr, row_doc, n_docs, tie=None, doc_rank=None, mask_rows=None, row_base=0, flags=0, metric=0):
    n, d = rows.shape
    bufs = [acc.to_device(rows), acc.to_device(row_doc.astype(np.uint32))]
    tie_p = inv_p = rank_p = mask_p = None
    if tie is not None:
        inv = np.empty_like(tie); inv[tie] = np.arange(n, dtype=tie.dtype)
        bufs += [acc.to_device(tie.astype(np.uint32)), acc.to_device(inv.astype(np.uint32))]
        tie_p, inv_p = bufs[-2].ptr, bufs[-1].ptr
    if doc_rank is not None:
        bufs.append(acc.to_device(doc_rank.astype(np.uint32))); rank_p = bufs[-1].ptr
    count = 0
    if mask_rows is not None:
        words = np.zeros((n + 31) // 32, np.uint32)
        for r in mask_rows:
            words[r >> 5] |= np.uint32(1 << (r & 31))
        bufs.append(acc.to_device(words)); mask_p = bufs[-1].ptr; count = len(set(int(r) for r in mask_rows))
    try:
        v = acc.corpus_view(bufs[0].ptr, n, d, tie_rank_ptr=tie_p, rank_row_ptr=inv_p, row_base=row_base, row_mask_ptr=mask_p,
                            row_mask_count=count)
        return acc.scan_doc_topk(v, acc.docs_view(bufs[1].ptr, n_docs, rank_p), queries, k, thr, metric=metric, flags=flags)
    finally:
        for b in bufs:
            b.free()


def check(acc, oracle, rows, queries, k, thr, row_doc, n_docs, tie=None, doc_rank=None, mask_rows=None, row_base=0, qsample=None):
    res = run(acc, rows, queries, k, thr, row_doc, n_docs, tie, doc_rank, mask_rows, row_base)
    allowed = None if mask_rows is None else np.unique(np.asarray(mask_rows, np.int64))
    n_eff = rows.shape[0] if allowed is None else len(allowed)
    assert res.diag["used_exact_scan"] == 1 and res.diag["path"] == 1
    assert res.diag["rows_visited"] == len(queries) * n_eff == res.diag["exact_distance_evaluations"]
    assert res.diag["returned_rows"] == int(res.matching.sum())
    for qi in (range(len(queries)) if qsample is None else qsample):
        e_rows, e_sc, e_docs, e_match = expected(oracle, rows, queries[qi], k, thr, row_doc, tie, doc_rank, allowed)
        cnt = int(res.counts[qi])
        assert int(res.matching[qi]) == e_match, qi
        assert cnt == len(e_rows), (qi, cnt, len(e_rows))
        assert res.rows[qi, :cnt].tolist() == (e_rows + row_base).tolist(), qi
        assert res.docs[qi, :cnt].tolist() == e_docs.tolist(), qi
        assert np.array_equal(res.scores[qi, :cnt].view(np.uint32), e_sc.view(np.uint32)), qi
        assert (res.rows[qi, cnt:] == -1).all() and (res.docs[qi, cnt:] == NO_DOC).all() and np.isneginf(res.scores[qi, cnt:]).all()
    return res


def layout(rng, n, n_docs, kind):
    if kind == "contiguous":
        cuts = np.sort(rng.choice(np.arange(1, n), n_docs - 1, replace=False))
        return np.repeat(np.arange(n_docs), np.diff(np.concatenate([[0], cuts, [n]]))).astype(np.uint32)
    if kind == "interleaved":
        return (np.arange(n) % n_docs).astype(np.uint32)
    return rng.integers(0, n_docs, n).astype(np.uint32)


def corpus(rng, n, d, special=True):
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[10:20] = rows[3]                                  # duplicated rows: equal scores within and across documents
    rows[200:203] = rows[7]
    if special:
        rows[30] = 0.0                                     # zero norm: dropped
        rows[31] = 0.0; rows[31, 0] = np.float32(1e-6)     # at the 1e-12 bound
        rows[32] = 0.0; rows[32, 0] = np.float32(1.0000001e-6)
        rows[33] = 0.0; rows[33, 1] = np.float32(-1e-6); rows[33, 2] = np.float32(1e-7)
        rows[34, 5] = np.nan                               # non-finite norms: dropped
        rows[35, 0] = np.inf
        rows[36] = rows[36] * np.float32(1e-20)            # tiny but non-zero
    return rows


@pytest.mark.parametrize("nq,d,kind,k", [(1, 100, "contiguous", 10), (7, 384, "interleaved", 5), (256, 768, "random", 10),
                                         (7, 1024, "contiguous", 1024), (1, 384, "random", 1), (7, 100, "random", 1024)])
def test_matches_oracle_and_restatement(acc, oracle, nq, d, kind, k):
    rng = np.random.default_rng(nq * 1000 + d)
    n, n_docs = 3000, 240
    rows = corpus(rng, n, d)
    row_doc = layout(rng, n, n_docs, kind)
    row_doc[rng.choice(n, 100, replace=False)] = NO_DOC    # rows without a document_hash: counted, never returned
    row_doc[10:20] = row_doc[10]                           # a run of identical rows in one document ...
    row_doc[200:203] = [1, 2, 3]                           # ... and identical rows in three documents
    tie = rng.permutation(n).astype(np.uint32)
    doc_rank = rng.permutation(n_docs).astype(np.uint32)
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    queries[0] = rows[3] * np.float32(3.0)                 # the duplicated row: ties decide
    for thr in (-1.0, 0.02):
        check(acc, oracle, rows, queries, k, thr, row_doc, n_docs, tie, doc_rank)
    check(acc, oracle, rows, queries, k, -1.0, row_doc, n_docs)      # ordinal order: no rank tables


def test_large_document_and_one_document_per_row(acc, oracle):
    rng = np.random.default_rng(5)
    n, d = 30_000, 128
    rows = corpus(rng, n, d)
    queries = rng.standard_normal((7, d)).astype(np.float32)
    row_doc = np.zeros(n, np.uint32)
    row_doc[20_000:] = 1 + np.arange(n - 20_000) // 7      # one 20 000-row document, then small ones
    check(acc, oracle, rows, queries, 50, -1.0, row_doc, int(row_doc.max()) + 1, tie=rng.permutation(n).astype(np.uint32))
    rd = rng.permutation(n).astype(np.uint32)               # n_docs == n_rows
    check(acc, oracle, rows, queries, 1024, -1.0, rd, n, doc_rank=rng.permutation(n).astype(np.uint32))


def test_threshold_k_and_edge_cases(acc, oracle):
    rng = np.random.default_rng(9)
    n, d, n_docs = 2000, 64, 50
    rows = corpus(rng, n, d)
    row_doc = layout(rng, n, n_docs, "random")
    queries = rng.standard_normal((3, d)).astype(np.float32)
    r = check(acc, oracle, rows, queries, 10, 1.5, row_doc, n_docs)              # above every score
    assert (r.counts == 0).all() and (r.matching == 0).all()
    r = check(acc, oracle, rows, queries, 200, -1.0, row_doc, n_docs)            # k > n_docs
    assert (r.counts == n_docs).all()
    r = run(acc, rows, queries, 0, -1.0, row_doc, n_docs)                        # k = 0: empty
    assert (r.counts == 0).all()
    r = check(acc, oracle, rows, queries, 10, -1.0, np.full(n, NO_DOC, np.uint32), 0)   # no documents at all
    assert (r.counts == 0).all() and (r.matching > 0).all()
    # invalid query: the batch fails; L2 / record path / threshold deferral: unsupported
    bad = queries.copy(); bad[1, 3] = np.nan
    with pytest.raises(_lib.AccelError) as e:
        run(acc, rows, bad, 10, -1.0, row_doc, n_docs)
    assert e.value.status == _lib.YAMS_ERR_INVALID_ARG
    with pytest.raises(_lib.AccelError) as e:
        run(acc, rows, np.zeros((1, d), np.float32), 10, -1.0, row_doc, n_docs)
    assert e.value.status == _lib.YAMS_ERR_INVALID_ARG
    for kw in ({"metric": _lib.SCAN_L2}, {"flags": _lib.FLAG_RECORD_PATH}, {"flags": _lib.FLAG_DEFER_THRESHOLD}):
        with pytest.raises(_lib.AccelError) as e:
            run(acc, rows, queries, 10, -1.0, row_doc, n_docs, **kw)
        assert e.value.status == _lib.YAMS_ERR_UNSUPPORTED, kw
    with pytest.raises(_lib.AccelError) as e:                                    # a document ordinal out of range
        rd = row_doc.copy(); rd[7] = n_docs
        run(acc, rows, queries, 10, -1.0, rd, n_docs)
    assert e.value.status == _lib.YAMS_ERR_INVALID_ARG
    check(acc, oracle, rows, queries, 10, -1.0, row_doc, n_docs, qsample=[0])    # the context is still usable


@pytest.mark.parametrize("density", ["sparse", "dense"])
def test_masks_and_row_base(acc, oracle, density):
    rng = np.random.default_rng(17)
    n, d, n_docs = 20_000, 96, 400
    rows = corpus(rng, n, d)
    row_doc = layout(rng, n, n_docs, "contiguous")
    queries = rng.standard_normal((7, d)).astype(np.float32)
    if density == "sparse":                                # a few candidate documents (gathered first)
        docs = rng.choice(n_docs, 12, replace=False)
        mask = np.nonzero(np.isin(row_doc, docs))[0]
    else:                                                  # most rows (read in place)
        mask = np.nonzero(rng.random(n) < 0.7)[0]
    check(acc, oracle, rows, queries, 20, -1.0, row_doc, n_docs, tie=rng.permutation(n).astype(np.uint32),
          doc_rank=rng.permutation(n_docs).astype(np.uint32), mask_rows=mask, row_base=1_000_000)


def test_one_million_rows_768_fifty_thousand_documents(acc, oracle):
    n, d, n_docs = 1_000_000, 768, 50_000
    rows = oracle.synth_rows(21, 0, n, d)
    rng = np.random.default_rng(21)
    row_doc = layout(rng, n, n_docs, "contiguous")
    queries = oracle.synth_rows(21, 1 << 40, 16, d)
    check(acc, oracle, rows, queries, 10, 0.05, row_doc, n_docs, doc_rank=rng.permutation(n_docs).astype(np.uint32),
          qsample=[0, 7, 15])


def test_query_slices_of_the_document_workspace(acc, oracle):
    """600 queries x 1 M document ordinals: 16 bytes per (query, document) exceed the 256 MiB budget, so the batch runs
    as slices of 16 queries; queries on both sides of slice boundaries are checked."""
    n, d, n_docs = 200_000, 32, 1_000_000
    rng = np.random.default_rng(33)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    row_doc = rng.choice(n_docs, n, replace=False).astype(np.uint32)
    row_doc[:5000] = row_doc[0]                            # and one large document
    queries = rng.standard_normal((600, d)).astype(np.float32)
    check(acc, oracle, rows, queries, 25, 0.3, row_doc, n_docs, tie=rng.permutation(n).astype(np.uint32),
          qsample=[0, 15, 16, 17, 300, 599])
