"""Shared by tests/test_entity_cpu.py, tests/test_entity_gpu.py and tests/stress_entity.py (test infrastructure): what
yams_scan_entity_topk_device must return for one query (`expected`), one call of it from host arrays (`run`), the comparison
(`compare`) and, separately, what the reference alone guarantees (`admissible`).

`scores` is the vectorised numpy restatement of float(VectorDatabase::computeCosineSimilarity(query, row))
(vector_database.cpp:1786-1810, cast at sqlite_vec_backend.cpp:2859): the three sums in fp64, ONE pass over the elements in
order (a product of two floats is exact in fp64, so `+= a * b` is the reference's multiply-then-add), sqrt of each norm, 0.0
if either norm == 0.0 tested before the division, the cast to fp32.  tests/test_entity_cpu.py pins it bit for bit on the
reference-compiled scanref_cosine and on the plain-C oracle.  `expected` then applies searchEntities' steps (:2854-2884):
the predicate, `similarity >= threshold`, and the order.  The reference's std::sort is not stable and has one key: the order
inside a run of equal similarities the reference leaves open; the device's rule — (similarity desc with -0.0 == +0.0, row
ordinal asc), a stable sort of the table order — is what `expected` states."""
import numpy as np

from yams_amd import _lib

UNSET, TYPE_UNSET = _lib.ENTITY_UNSET, _lib.ENTITY_TYPE_UNSET


def scores(rows, q):
    rows = np.ascontiguousarray(rows, np.float32); q = np.ascontiguousarray(q, np.float32)
    n, d = rows.shape
    dot = np.zeros(n, np.float64); nb = np.zeros(n, np.float64); na = np.float64(0.0)
    with np.errstate(all="ignore"):
        for i in range(d):
            x = rows[:, i].astype(np.float64); a = np.float64(q[i])
            dot += a * x
            na += a * a
            nb += x * x
        na = np.sqrt(na); nb = np.sqrt(nb)
        zero = (nb == 0.0) | (na == 0.0)
        sd = np.where(zero, 0.0, dot / np.where(zero, 1.0, na * nb))
        return sd.astype(np.float32)


def admitted(n, types, node_types, docs, filt, allowed):
    """Ordinals (ascending) the row mask (`allowed`: ordinals or None) and the filter (type, node_type, doc; None = not set) admit."""
    on = np.zeros(n, bool)
    on[np.arange(n) if allowed is None else np.asarray(allowed, np.int64)] = True
    if filt is not None:
        t, nt, dc = filt
        if t is not None:
            on &= (types == t) & (t < TYPE_UNSET)
        if nt is not None:
            on &= (node_types == nt) & (nt != UNSET)
        if dc is not None:
            on &= (docs == dc) & (dc != UNSET)
    return np.nonzero(on)[0]


def expected(rows, q, k, thr, types=None, node_types=None, docs=None, filt=None, allowed=None):
    """(row ordinals, scores, rows visited, rows kept) of one query under the device's order rule."""
    adm = admitted(rows.shape[0], types, node_types, docs, filt, allowed)
    s = scores(rows[adm], q) if len(adm) else np.zeros(0, np.float32)
    with np.errstate(invalid="ignore"):
        kept = np.nonzero(s >= np.float32(thr))[0]              # float compare: NaN on either side keeps nothing
    order = kept[np.argsort(-s[kept], kind="stable")]           # -0.0 == +0.0 under the compare; equal scores stay in row order
    order = order[:k]
    return adm[order], s[order], len(adm), len(kept)


def mask_words(n, mask_rows):
    words = np.zeros((n + 31) // 32, np.uint32)
    r = np.unique(np.asarray(mask_rows, np.int64))
    np.bitwise_or.at(words, r >> 5, (np.uint32(1) << (r & 31).astype(np.uint32)))
    return words, len(r)


def run(acc, rows, queries, k, thr, types=None, node_types=None, docs=None, filters=None, mask_rows=None, row_base=0, rows_offset=0):
    """rows_offset > 0 places the rows that many floats past a 16-byte aligned allocation (an unaligned row pointer)."""
    n, d = rows.shape
    src = rows if not rows_offset else np.concatenate([np.zeros(rows_offset, np.float32), rows.ravel()])
    bufs = [acc.to_device(src)]
    ptrs = []
    for col, dt in ((types, np.uint8), (node_types, np.uint32), (docs, np.uint32)):
        if col is None:
            ptrs.append(None)
        else:
            bufs.append(acc.to_device(np.ascontiguousarray(col, dt))); ptrs.append(bufs[-1].ptr)
    mask_p, count = None, 0
    if mask_rows is not None:
        words, count = mask_words(n, mask_rows)
        bufs.append(acc.to_device(words)); mask_p = bufs[-1].ptr
    try:
        v = acc.corpus_view(bufs[0].ptr + 4 * rows_offset, n, d, row_base=row_base, row_mask_ptr=mask_p, row_mask_count=count)
        return acc.scan_entity_topk(v, acc.entities_view(*ptrs), queries, k, thr, filters)
    finally:
        for b in bufs:
            b.free()


def admissible(got_rows, got_scores, rows, q, k, thr, types=None, node_types=None, docs=None, filt=None, allowed=None):
    """Only what the reference guarantees for a result (ordinals, scores): every returned row is a kept row carrying its own
    score bits, no row twice, scores never increase, and the multiset of scores (as values: -0.0 == +0.0) is that of the
    min(k, kept) best kept rows.  None when it holds, else a description."""
    adm = admitted(rows.shape[0], types, node_types, docs, filt, allowed)
    s = scores(rows[adm], q) if len(adm) else np.zeros(0, np.float32)
    with np.errstate(invalid="ignore"):
        keep = s >= np.float32(thr)
    own = dict(zip(adm[keep].tolist(), s[keep].view(np.uint32).tolist()))
    if len(set(got_rows.tolist())) != len(got_rows):
        return "a row twice"
    for r, b in zip(got_rows.tolist(), got_scores.view(np.uint32).tolist()):
        if own.get(r) != b:
            return "row %d is not a kept row with these score bits" % r
    if len(got_scores) > 1 and (np.diff(got_scores) > 0).any():
        return "a worse score before a better one"
    best = np.sort(s[keep])[::-1][:k]
    if len(best) != len(got_scores) or not np.array_equal(best + np.float32(0.0), got_scores + np.float32(0.0)):
        return "score multiset"
    return None


def compare(res, qi, rows, queries, k, thr, types=None, node_types=None, docs=None, filters=None, allowed=None, row_base=0):
    """None when query qi of `res` is what it must be, else a short description of the first difference."""
    filt = None if filters is None else filters[qi]
    e_rows, e_sc, e_vis, e_match = expected(rows, queries[qi], k, thr, types, node_types, docs, filt, allowed)
    cnt = int(res.counts[qi])
    if int(res.matching[qi]) != e_match:
        return "matching %d != %d" % (int(res.matching[qi]), e_match)
    if cnt != len(e_rows):
        return "count %d != %d" % (cnt, len(e_rows))
    if not np.array_equal(res.scores[qi, :cnt].view(np.uint32), e_sc.view(np.uint32)):
        return "score bits"
    if res.rows[qi, :cnt].tolist() != (e_rows + row_base).tolist():
        return "rows"
    if not ((res.rows[qi, cnt:] == -1).all() and np.isneginf(res.scores[qi, cnt:]).all()):
        return "padding"
    return admissible(res.rows[qi, :cnt] - row_base, res.scores[qi, :cnt], rows, queries[qi], k, thr, types, node_types, docs, filt, allowed)


def visited_total(n, queries, types, node_types, docs, filters, allowed):
    return sum(len(admitted(n, types, node_types, docs, None if filters is None else filters[qi], allowed)) for qi in range(len(queries)))
