"""Document-level top-k on the device (yams_scan_doc_topk_device): every matching row of the allowed set (the oracle's
exact cosine, oracle_exact_scan_cosine with k = all rows) reduced by the restatement of retainBestRecordPerDocument
(tests/_doc_select.py, sqlite_vec_backend.cpp:86-125).  Rows, document ordinals, score bits, order, counts and the
matching-row counts must be identical."""
import numpy as np
import pytest

from _doc_oracle import NO_DOC, expected, run  # noqa: F401  (run and NO_DOC: also used by test_doc_topk_plugin_gpu.py)
from yams_amd import _lib

pytestmark = pytest.mark.gpu


def check(acc, oracle, rows, queries, k, thr, row_doc, n_docs, tie=None, doc_rank=None, mask_rows=None, row_base=0, qsample=None,
          rows_offset=0):
    res = run(acc, rows, queries, k, thr, row_doc, n_docs, tie, doc_rank, mask_rows, row_base, rows_offset=rows_offset)
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


@pytest.mark.parametrize("d,offset", [(1, 0), (3, 0), (33, 0), (385, 0), (128, 1), (33, 1)])
def test_scalar_staging_of_rows_that_are_not_16_byte_loads(acc, oracle, d, offset):
    """doc_score_kernel stages a row with 16-byte loads only when dim % 4 == 0 and the row pointer is 16-byte aligned;
    every other shape goes through the scalar staging and its tail bound (the last 1-3 elements of a 32-element chunk)."""
    rng = np.random.default_rng(400 + d + offset)
    n, n_docs = 2_500, 300
    rows = corpus(rng, n, d, special=d >= 6)
    row_doc = layout(rng, n, n_docs, "random")
    row_doc[rng.choice(n, 50, replace=False)] = NO_DOC
    queries = rng.standard_normal((5, d)).astype(np.float32)
    queries[1] = rows[3] * np.float32(1.5)
    check(acc, oracle, rows, queries, 40, -1.0, row_doc, n_docs, tie=rng.permutation(n).astype(np.uint32),
          doc_rank=rng.permutation(n_docs).astype(np.uint32), rows_offset=offset)
    check(acc, oracle, rows, queries[:1], 7, 0.05, row_doc, n_docs, rows_offset=offset)


@pytest.mark.parametrize("nq", [2, 4, 5, 9])
def test_query_group_forms(acc, oracle, nq):
    """QG = 4 for 2-4 queries, 8 above (a ragged last group for 5 and 9): every query of the group against the oracle."""
    rng = np.random.default_rng(500 + nq)
    n, d, n_docs = 5_000, 64, 700
    rows = corpus(rng, n, d)
    row_doc = layout(rng, n, n_docs, "contiguous")
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    queries[nq - 1] = rows[10] * np.float32(0.5)
    check(acc, oracle, rows, queries, 30, -1.0, row_doc, n_docs, tie=rng.permutation(n).astype(np.uint32))


@pytest.mark.parametrize("nq", [17, 19])
def test_last_query_slice_of_one_and_of_three_queries(acc, oracle, nq):
    """1 M document ordinals: a slice holds 256 MiB / (16 * 1 M) = 16 queries, so 17 and 19 queries leave a last slice of
    1 (QG = 1) and of 3 (QG = 4) queries at q0 = 16: their query vectors, norms and matching counters are offset."""
    n, d, n_docs = 20_000, 36, 1_000_000
    rng = np.random.default_rng(600 + nq)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    row_doc = rng.choice(n_docs, n, replace=False).astype(np.uint32)
    row_doc[:3000] = row_doc[0]
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    queries[16] = rows[5] * np.float32(3.0)
    check(acc, oracle, rows, queries, 20, 0.1, row_doc, n_docs, doc_rank=rng.permutation(n_docs).astype(np.uint32),
          qsample=[0, 15] + list(range(16, nq)))


def test_document_runs_at_wave_and_workgroup_edges(acc, oracle):
    """The segmented max over runs of equal documents inside a wave: runs that start and end on, one before and one after
    64- and 256-row edges, single-row runs, and runs spanning several workgroups; a dense and a sparse (gathered) mask."""
    rng = np.random.default_rng(77)
    runs = [64, 64, 1, 63, 65, 127, 1, 256, 255, 257, 2, 512, 190, 66, 700, 1, 1, 64]
    n, d = sum(runs), 48
    rows = corpus(rng, n, d)
    row_doc = np.repeat(np.arange(len(runs)) * 3 % len(runs), runs).astype(np.uint32)
    queries = rng.standard_normal((9, d)).astype(np.float32)
    check(acc, oracle, rows, queries, 18, -1.0, row_doc, len(runs), tie=rng.permutation(n).astype(np.uint32))
    check(acc, oracle, rows, queries, 18, -1.0, row_doc, len(runs), mask_rows=np.nonzero(rng.random(n) < 0.6)[0])
    check(acc, oracle, rows, queries, 18, -1.0, row_doc, len(runs), mask_rows=np.nonzero(rng.random(n) < 0.05)[0])


def test_mask_at_the_sparse_dense_switch(acc, oracle):
    """A mask of fewer than n_rows / 8 rows is gathered first, one of n_rows / 8 or more is read in place: 511, 512 and
    513 allowed rows of 4096."""
    rng = np.random.default_rng(88)
    n, d, n_docs = 4096, 40, 333
    rows = corpus(rng, n, d)
    row_doc = layout(rng, n, n_docs, "random")
    queries = rng.standard_normal((3, d)).astype(np.float32)
    for cnt in (511, 512, 513):
        mask = np.sort(rng.choice(n, cnt, replace=False))
        check(acc, oracle, rows, queries, 25, -1.0, row_doc, n_docs, mask_rows=mask, row_base=5)


def test_refusals_leave_the_context_usable(acc, oracle):
    """A doc_rank that is not a permutation (a repeated rank, every rank in range), a striped shard and a tie_rank without
    rank_row are refused; the next call on the same context is served."""
    rng = np.random.default_rng(99)
    n, d, n_docs = 3000, 64, 120
    rows = corpus(rng, n, d)
    row_doc = layout(rng, n, n_docs, "random")
    queries = rng.standard_normal((3, d)).astype(np.float32)
    rep = rng.permutation(n_docs).astype(np.uint32)
    rep[17] = rep[90]                                      # rank rep[90] twice, one rank missing
    with pytest.raises(_lib.AccelError) as e:
        run(acc, rows, queries, 10, -1.0, row_doc, n_docs, doc_rank=rep)
    assert e.value.status == _lib.YAMS_ERR_INVALID_ARG
    check(acc, oracle, rows, queries, 10, -1.0, row_doc, n_docs, doc_rank=rng.permutation(n_docs).astype(np.uint32))
    d_rows, d_doc, d_tie = acc.to_device(rows), acc.to_device(row_doc), acc.to_device(np.arange(n, dtype=np.uint32))
    try:
        dv = acc.docs_view(d_doc.ptr, n_docs)
        with pytest.raises(_lib.AccelError) as e:
            acc.scan_doc_topk(acc.corpus_view(d_rows.ptr, n, d, stripe_rows=1024, n_stripes=3), dv, queries, 10, -1.0)
        assert e.value.status == _lib.YAMS_ERR_UNSUPPORTED
        check(acc, oracle, rows, queries, 10, -1.0, row_doc, n_docs)
        with pytest.raises(_lib.AccelError) as e:
            acc.scan_doc_topk(acc.corpus_view(d_rows.ptr, n, d, tie_rank_ptr=d_tie.ptr), dv, queries, 10, -1.0)
        assert e.value.status == _lib.YAMS_ERR_INVALID_ARG
        check(acc, oracle, rows, queries, 10, -1.0, row_doc, n_docs)
    finally:
        for b in (d_rows, d_doc, d_tie):
            b.free()


def test_randomised_doc_stress_against_the_oracle():
    """tests/stress_doc.py: random dims (scalar and 16-byte staging), query groups and slices, document counts around the
    select cap, layouts with runs at wave / workgroup edges, masks at the sparse / dense switch, tie and document ranks;
    every checked query bit-exact against the oracle + the restated reduction, and every path reached."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "stress_doc.py"), "--cases", "240", "--seed", "5"],
                       capture_output=True, text=True, timeout=280)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["cases"] == 240 and res["mismatches"] == 0 and res["checked_queries"] >= 240, res
    assert all(v > 0 for v in res["paths"].values()), res["paths"]
