"""Score edges on the device: the seeded small-scan harness (tests/stress_small.py: the fused one-launch kernel and the
general path around its rule, held to the CPU oracle alone), and scripted zero-plateau cases — a top-k cut that runs
through similarities of +0.0f and -0.0f, which the reference's float compares treat as ONE score ordered by chunk id
(sqlite_vec_backend.cpp:4218-4223, :4296-4298, :100-120) — through every path that selects by key.  Each returned zero
must carry its own sign bit.  tests/test_score_edges_cpu.py proves from the oracle alone that every shape used here tells
that order from an order by score bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _doc_oracle
import _pq
import _score_edges as se
import stress_small
from test_doc_topk_gpu import check as doc_check
from test_pq_gpu import check as pq_check
from test_scan_gpu import _check_vs_oracle, _masked, _one_shard_views, check, run
from yams_amd import _lib
from yams_amd._lib import SCAN_COSINE, FLAG_FORCE_EXACT, FLAG_RECORD_PATH

pytestmark = pytest.mark.gpu

NEG_ZERO, POS_ZERO = 0x80000000, 0


def plateau(name, **kw):
    n, dim, nq, k, P, Z = se.SCRIPTED[name]
    return se.zero_plateau(1, n, dim, nq, k, P, Z, **kw), k


def both_zeros_returned(r):
    """The answer of every query holds zeros of both signs (the oracle comparison has already pinned which)."""
    for qi in range(r.scores.shape[0]):
        bits = set(r.scores[qi, :int(r.counts[qi])].view(np.uint32).tolist())
        assert {NEG_ZERO, POS_ZERO} <= bits, (qi, sorted(bits)[:4])


def test_small_scan_harness_against_the_cpu_oracle():
    """tests/stress_small.py at its default seed and case count (test_score_edges_cpu.py asserts what they reach): every
    query of every case equals the CPU oracle, diag.path equals the stated rule; one context, cases in sequence."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "stress_small.py")], capture_output=True, text=True, timeout=280)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(line[-1])
    print(line[-1])
    assert r.returncode == 0 and "failed" not in res, res
    assert res["cases"] == stress_small.DEFAULT_CASES and res["mismatches"] == 0 and not res["dry_run"], res
    assert res["paths"]["fused"] >= 5 and res["paths"]["general"] >= 5, res


@pytest.mark.parametrize("name", ["fused_nq1", "fused_nq5"])
def test_zero_plateau_on_the_fused_path(acc, oracle, name):
    z, k = plateau(name)
    for thr in (-1.0, -0.0, 0.0):
        r = check(acc, oracle, z["corpus"], z["queries"], k, thr, tie_rank=z["tie_rank"], expect_path=1)
        both_zeros_returned(r)
    r = check(acc, oracle, z["corpus"], z["queries"], k, se.DENORM_MIN, tie_rank=z["tie_rank"], expect_path=1)
    assert (r.counts == se.SCRIPTED[name][4]).all()                  # the smallest denormal drops the whole plateau
    rr = run(acc, z["corpus"], z["queries"], k, -1.0, SCAN_COSINE, FLAG_RECORD_PATH, z["tie_rank"])
    assert rr.diag["path"] == 1
    _records(oracle, z, rr, k, None)


def _records(oracle, z, r, k, allowed):
    """A FLAG_RECORD_PATH answer against oracle.scan_cosine_records."""
    n = z["corpus"].shape[0]
    allow = np.ones(n, np.uint8)
    if allowed is not None:
        allow[:] = 0; allow[allowed] = 1
    ans = []
    for q in z["queries"]:
        rows, sims = oracle.scan_cosine_records(z["corpus"], q, k, -1.0, z["tie_rank"].astype(np.uint64), allow)[:2]
        ans.append((rows, sims, None))
    msg = se.compare(r.counts, r.rows, r.scores, r.dist, r.diag["rows_visited"], ans, k, SCAN_COSINE, len(ans) * int(allow.sum()))
    assert msg is None, (msg, r.diag)


def test_zero_plateau_on_the_general_path(acc, oracle):
    """The bf16 filter tier and its fp64 re-score; the exhaustive pipeline; the record path behind an allow-mask."""
    z, k = plateau("general")
    r = check(acc, oracle, z["corpus"], z["queries"], k, -1.0, tie_rank=z["tie_rank"], expect_path=0, expect_tier=_lib.TIER_BF16)
    both_zeros_returned(r)
    r = check(acc, oracle, z["corpus"], z["queries"], k, 0.0, tie_rank=z["tie_rank"], expect_path=0)
    both_zeros_returned(r)
    r = check(acc, oracle, z["corpus"], z["queries"], k, -1.0, flags=FLAG_FORCE_EXACT, tie_rank=z["tie_rank"], expect_path=1)
    both_zeros_returned(r)
    n = z["corpus"].shape[0]
    rng = np.random.default_rng(3)
    keep = rng.random(n) < 0.6
    keep[z["plateau"][[0, 1]]] = True                              # (the best-ranked -0.0 and the +0.0 behind it stay in)
    allowed = np.flatnonzero(keep)
    rr = run(acc, z["corpus"], z["queries"], k, -1.0, SCAN_COSINE, FLAG_RECORD_PATH, z["tie_rank"], mask=keep)
    assert rr.diag["path"] == se.restated_diag_path(n, len(allowed), z["corpus"].shape[1], len(z["queries"]), k, SCAN_COSINE, FLAG_RECORD_PATH) == 1
    _records(oracle, z, rr, k, allowed)
    both_zeros_returned(rr)
    r = _masked(acc, oracle, z["corpus"], z["queries"], k, allowed, tie_rank=z["tie_rank"])   # the fast path behind the same mask
    both_zeros_returned(r)


def test_zero_plateau_wider_than_the_rescore_and_the_candidate_lists(acc, oracle):
    """5000 rows of one score at the cut: more than one re-score launch sorts (2048) and than the candidate lists hold, so the
    exhaustive pipeline's top-2048 cut decides — it must keep the best-RANKED rows of the plateau, -0.0 ones included."""
    z, k = plateau("general_wide_plateau")
    r = check(acc, oracle, z["corpus"], z["queries"], k, -1.0, tie_rank=z["tie_rank"], expect_path=0)
    both_zeros_returned(r)
    print("route:", {x: r.diag[x] for x in ("filter_tier", "widened_queries", "escalated_queries", "exact_fallback_queries")})


@pytest.mark.parametrize("layout", [0, _lib.I8_ROTATED])
def test_zero_plateau_on_the_int8_tier(acc, oracle, layout):
    z, k = plateau("int8")
    r = check(acc, oracle, z["corpus"], z["queries"], k, -1.0, tie_rank=z["tie_rank"], expect_path=0, shadow="i8",
              expect_tier=_lib.TIER_I8, i8_flags=layout)
    both_zeros_returned(r)
    # (the route is recorded, not asserted: whether the proof needs widening here is the tier's business)
    print("route:", {x: r.diag[x] for x in ("widened_queries", "escalated_queries", "exact_fallback_queries")})


def test_zero_plateau_in_document_top_k(acc, oracle):
    """(i) One document holds a +0.0 row and a -0.0 row with the lower chunk id: equal scores to :99-103, so the -0.0 row
    and its bits come back.  (ii) The plateau across documents at the cut: ordered by document rank, not by sign."""
    z, k = plateau("doc")
    n = z["corpus"].shape[0]
    row_doc = np.arange(n, dtype=np.uint32)                        # one document per row ...
    neg, pos = int(z["plateau"][0]), int(z["plateau"][1])          # ... but the best-ranked -0.0 row and the +0.0 behind it share one
    row_doc[pos] = row_doc[neg]
    rng = np.random.default_rng(4)
    doc_rank = rng.permutation(n).astype(np.uint32)
    best = int(np.flatnonzero(doc_rank == 0)[0])                   # that document has the best document rank: inside every cut
    doc_rank[best], doc_rank[row_doc[neg]] = doc_rank[row_doc[neg]], 0
    for thr in (-1.0, 0.0):
        res = doc_check(acc, oracle, z["corpus"], z["queries"], k, thr, row_doc, n, tie=z["tie_rank"], doc_rank=doc_rank)
        both_zeros_returned(res)
        for qi in range(len(z["queries"])):
            at = np.flatnonzero(res.docs[qi, :int(res.counts[qi])] == row_doc[neg])
            assert at.size == 1 and res.rows[qi, at[0]] == neg and res.scores[qi, at[0]:at[0] + 1].view(np.uint32)[0] == NEG_ZERO
            assert _doc_oracle.compare(oracle, res, z["corpus"], z["queries"], qi, k, thr, row_doc, z["tie_rank"], doc_rank) is None
    # no rank tables: row order is chunk-id order, document ordinals are document-hash order
    zr = se.zero_plateau(1, *se.SCRIPTED["doc"], row_order=True)
    res = doc_check(acc, oracle, zr["corpus"], zr["queries"], k, -1.0, np.arange(n, dtype=np.uint32), n)
    both_zeros_returned(res)


def test_zero_plateau_in_the_pq_rerank(acc, oracle):
    """An index of n_codes <= k * rerank_factor codes: the whole plateau is shortlisted whatever the ADC order, the exact
    re-rank orders it — (similarity desc, chunk_id asc), the two zeros one score.  (Signed zeros in the ADC sum itself are
    out of scope: the order of that sum is unpinned.)"""
    z, k = plateau("pq")
    corpus = z["corpus"]
    n = corpus.shape[0]
    assert n <= k * 2
    u = _pq.unit(corpus)
    pq = _pq.Pq(u, 8, 1)
    codes = pq.encode(u)
    keys = np.array([_pq.stable_string_key("c%07d" % i) for i in range(n)], np.uint64)
    r = pq_check(acc, oracle, corpus, pq, codes, keys, z["tie_rank"], z["queries"], k, -1.0, rf=2)
    both_zeros_returned(r)
    r = pq_check(acc, oracle, corpus, pq, codes, keys, z["tie_rank"], z["queries"], k, 0.0, rf=2)
    both_zeros_returned(r)


def test_zero_plateau_across_three_shards_on_one_device(oracle):
    """Three shards on device 0, the plateau's rows (and with them its ranks: the row order) interleaved across the shards:
    each shard's own top k and the merge must order the zeros as one score."""
    from yams_amd.accel import ShardedScan
    n, d, nq, k, P, Z = se.SCRIPTED["sharded"]
    z = se.zero_plateau(1, n, d, nq, k, P, Z, row_order=True)
    corpus = np.ascontiguousarray(z["corpus"])
    parts = [(n * i // 3, n * (i + 1) // 3) for i in range(3)]
    assert all(((z["plateau"] >= lo) & (z["plateau"] < hi)).sum() >= 20 for lo, hi in parts)
    sh = ShardedScan([0, 0, 0], lanes=1)
    try:
        keep, views = _one_shard_views(sh, oracle, corpus, d, parts)
        for thr in (-1.0, 0.0):
            r = sh.topk(views, z["queries"], k, thr, SCAN_COSINE)
            _check_vs_oracle(oracle, corpus, z["queries"], r, k, thr, SCAN_COSINE)
            both_zeros_returned(r)
    finally:
        sh.close()


def test_unused_slots_hold_the_documented_values(acc):
    """Slots counts[q] .. k-1 of EVERY output array of yams_scan_topk_device hold score -inf / row -1 / distance +inf / rank
    0xffffffff (contract_rules.h, write_empty_slot), written by the kernel into buffers that held other bytes: 5 rows x dim 8,
    2 queries, k = 8, cosine and L2 with distances and ranks requested — served by the fused small scan, and by the re-score
    behind FLAG_FORCE_EXACT.  The other entry points' padding is asserted where their results are checked and is left out
    here: yams_scan_doc_topk_device (scores, rows, documents) by tests/test_doc_topk_gpu.py `check` and
    tests/_doc_oracle.py `compare`; yams_scan_entity_topk_device by tests/_entity_oracle.py `compare` ("padding") and
    tests/test_entity_gpu.py; yams_scan_merge_topk_device (scores, rows, distances) by
    tests/test_merge_gpu.py::test_query_that_is_empty_in_every_shard."""
    n, d, nq, k = 5, 8, 2, 8
    rng = np.random.default_rng(11)
    corpus = rng.standard_normal((n, d)).astype(np.float32)
    corpus[3] = 0.0                                                 # cosine drops it; L2 keeps it with cosine 0
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    dc, dq = acc.to_device(corpus), acc.to_device(queries)
    view = acc.corpus_view(dc.ptr, n, d)
    poison = np.full(nq * k * 8, 0x5a, np.uint8)
    bufs = [acc.to_device(poison) for _ in range(5)]
    d_s, d_r, d_n, d_d, d_k = bufs
    try:
        for metric in (SCAN_COSINE, _lib.SCAN_L2):
            for flags in (0, FLAG_FORCE_EXACT):
                for b in bufs:
                    b.upload(poison)
                acc.scan_topk_device(view, dq.ptr, nq, k, 0.0, metric, d_s.ptr, d_r.ptr, d_n.ptr, d_d.ptr, d_k.ptr, flags=flags)
                acc.synchronize()
                counts = d_n.download(np.uint32, nq)
                scores = d_s.download(np.float32, nq * k).reshape(nq, k)
                rows = d_r.download(np.int64, nq * k).reshape(nq, k)
                dist = d_d.download(np.float32, nq * k).reshape(nq, k)
                ranks = d_k.download(np.uint32, nq * k).reshape(nq, k)
                what = (metric, flags, counts.tolist())
                assert (counts < k).all() and counts.max() >= 1, what
                for qi in range(nq):
                    c = int(counts[qi])
                    assert ((rows[qi, :c] >= 0) & (rows[qi, :c] < n)).all() and (ranks[qi, :c] == rows[qi, :c]).all(), what
                    assert np.isneginf(scores[qi, c:]).all(), (what, scores[qi])
                    assert (rows[qi, c:] == -1).all(), (what, rows[qi])
                    assert np.isposinf(dist[qi, c:]).all(), (what, dist[qi])
                    assert (ranks[qi, c:] == 0xffffffff).all(), (what, ranks[qi])
    finally:
        for b in bufs + [dc, dq]:
            b.free()
