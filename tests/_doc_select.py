"""A Python restatement of retainBestRecordPerDocument (src/vector/sqlite_vec_backend.cpp:86-125 of the reference), the
reduction behind document-level selection (CandidateFilterMode::DocumentTopK): every matching row goes in, the best row
per document and the best `limit` documents come out.  Strings compare as the reference's std::string does (byte-wise)."""
from __future__ import annotations


def _b(s) -> bytes:
    return s if isinstance(s, bytes) else s.encode()


def best_per_document(rows, scores, chunk_ids, document_hashes, limit):
    """rows / scores (float32) / chunk_ids / document_hashes: one entry per matching row, in any order.
    Returns [(row, score, document_hash)] best first."""
    best = {}
    for row, score, cid, doc in zip(rows, scores, chunk_ids, document_hashes):
        if len(_b(doc)) == 0:                                   # :90-92: a row without a document is dropped
            continue
        key = _b(doc)
        cur = best.get(key)
        if cur is None:                                         # :94-98: the document's first row
            best[key] = (row, score, _b(cid))
            continue
        # :99-103: a better score, or the same score and a smaller chunk_id, replaces it
        if score > cur[1] or (score == cur[1] and _b(cid) < cur[2]):
            best[key] = (row, score, _b(cid))
    out = [(r, s, d, c) for d, (r, s, c) in best.items()]
    # :111-121: score desc, then document_hash asc, then chunk_id asc
    out.sort(key=lambda t: (-float(t[1]), t[2], t[3]))
    return [(r, s, d) for r, s, d, _ in out[:limit]]                # :122-124
