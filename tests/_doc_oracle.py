"""Shared by tests/test_doc_topk_gpu.py and tests/stress_doc.py: one call of yams_scan_doc_topk_device from host arrays
(`run`), and what it must return for one query (`expected`): the oracle's matching rows of the allowed set
(oracle_exact_scan_cosine with k = all rows), reduced by the restatement of retainBestRecordPerDocument
(tests/_doc_select.py, sqlite_vec_backend.cpp:86-125)."""
import numpy as np

from _doc_select import best_per_document
from yams_amd import _lib

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


def mask_words(n, mask_rows):
    """The allow-mask bit words of the given rows (one bit per row, LSB first) and the number of distinct rows."""
    words = np.zeros((n + 31) // 32, np.uint32)
    r = np.unique(np.asarray(mask_rows, np.int64))
    np.bitwise_or.at(words, r >> 5, (np.uint32(1) << (r & 31).astype(np.uint32)))
    return words, len(r)


def run(acc, rows, queries, k, thr, row_doc, n_docs, tie=None, doc_rank=None, mask_rows=None, row_base=0, flags=0, metric=0,
        rows_offset=0):
    """rows_offset > 0 places the rows that many floats past a fresh (16-byte aligned) allocation: a row pointer that is
    not 16-byte aligned."""
    n, d = rows.shape
    src = rows if not rows_offset else np.concatenate([np.zeros(rows_offset, np.float32), rows.ravel()])
    bufs = [acc.to_device(src), acc.to_device(row_doc.astype(np.uint32))]
    rows_p = bufs[0].ptr + 4 * rows_offset
    tie_p = inv_p = rank_p = mask_p = None
    if tie is not None:
        inv = np.empty_like(tie); inv[tie] = np.arange(n, dtype=tie.dtype)
        bufs += [acc.to_device(tie.astype(np.uint32)), acc.to_device(inv.astype(np.uint32))]
        tie_p, inv_p = bufs[-2].ptr, bufs[-1].ptr
    if doc_rank is not None:
        bufs.append(acc.to_device(doc_rank.astype(np.uint32))); rank_p = bufs[-1].ptr
    count = 0
    if mask_rows is not None:
        words, count = mask_words(n, mask_rows)
        bufs.append(acc.to_device(words)); mask_p = bufs[-1].ptr
    try:
        v = acc.corpus_view(rows_p, n, d, tie_rank_ptr=tie_p, rank_row_ptr=inv_p, row_base=row_base, row_mask_ptr=mask_p,
                            row_mask_count=count)
        return acc.scan_doc_topk(v, acc.docs_view(bufs[1].ptr, n_docs, rank_p), queries, k, thr, metric=metric, flags=flags)
    finally:
        for b in bufs:
            b.free()


def compare(oracle, res, rows, queries, qi, k, thr, row_doc, tie=None, doc_rank=None, allowed=None, row_base=0):
    """None when query qi of `res` is what it must be, else a short description of the first difference."""
    e_rows, e_sc, e_docs, e_match = expected(oracle, rows, queries[qi], k, thr, row_doc, tie, doc_rank, allowed)
    cnt = int(res.counts[qi])
    if int(res.matching[qi]) != e_match:
        return "matching %d != %d" % (int(res.matching[qi]), e_match)
    if cnt != len(e_rows):
        return "count %d != %d" % (cnt, len(e_rows))
    if res.rows[qi, :cnt].tolist() != (e_rows + row_base).tolist():
        return "rows"
    if res.docs[qi, :cnt].tolist() != e_docs.tolist():
        return "documents"
    if not np.array_equal(res.scores[qi, :cnt].view(np.uint32), e_sc.view(np.uint32)):
        return "score bits"
    if not ((res.rows[qi, cnt:] == -1).all() and (res.docs[qi, cnt:] == NO_DOC).all() and np.isneginf(res.scores[qi, cnt:]).all()):
        return "padding"
    return None
