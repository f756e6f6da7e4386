"""Randomised stress of the product-quantised engine (yams_scan_pq_topk_device) on the GPU against the oracle
(oracle_pq_search, the committed plain-C restatement of simeonPqSearchUnlocked): random index sizes on both sides of the
unfiltered / filtered switch (65 536), sub-quantiser counts on both sides of every table-group boundary of both ADC
kernels, every served sum order, k and rerank factors up to approxK 2047, thresholds, many-to-one row maps with lost rows,
candidate lists (none, sparse, >= 65 536, empty), refused (zero / tiny) queries, random or product-quantiser tables, some
of them coarse or all-equal (fallbacks), and query batches larger than one unfiltered key batch.  Rows, score bits and
counts of every checked query must be identical.  Test infrastructure (uses oracle/).

    python tests/stress_pq.py [--cases 40] [--seed 1]

The summary counts the code paths the cases reached, as the host code chooses them (pq_api.cpp, pq_kernels.hip).
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import _oracle
import _pq
from yams_amd.accel import Accel

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=40)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()
rng = np.random.default_rng(a.seed)
acc = Accel(0, torch.cuda.current_stream().cuda_stream)
o = _oracle.oracle()

M_EDGES = [4, 7, 8, 16, 32, 33, 36, 37, 64, 65, 72, 73, 127, 128]
FILTER_MIN = 65536                    # pq_api.cpp: indexes (or candidate lists) of at least this many entries are filtered
KEY_BUDGET = 1 << 31                  # pq_api.cpp: bytes of unfiltered keys per batch of queries
PATHS = ["filtered", "unfiltered", "filter_qg1", "filter_qg2", "filter_qg4", "keys_qg1", "keys_qg2", "keys_qg4",
         "filter_words", "filter_bytes", "keys_words", "keys_bytes", "radix_tau", "multi_batch"]


def log_uniform(lo, hi):
    return int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1))))


def paths_of(n_items, m, nq, approx, n_fallback, hits):
    """The kernels pq_api.cpp launched for this call (restated from its choices)."""
    if n_items == 0:
        return
    if n_items >= FILTER_MIN:
        hits["filtered"] += nq - n_fallback
        qg = 4 if m * 4096 <= 144 * 1024 else (2 if m * 2048 <= 144 * 1024 else 1)
        hits["filter_qg%d" % qg] += 1
        hits["filter_words" if m % 4 == 0 else "filter_bytes"] += 1
        stride = min(64, max(1, n_items // 16384))
        rank = max(16, -(-max(4 * approx, 1024) // stride))
        if rank > 256:
            hits["radix_tau"] += 1
    if n_fallback:
        hits["unfiltered"] += n_fallback
        batch = min(max(1, KEY_BUDGET // (n_items * 8)), n_fallback)
        if n_fallback > batch:
            hits["multi_batch"] += 1
        for b0 in range(0, n_fallback, batch):
            nb = min(batch, n_fallback - b0)
            qg = 4
            while qg > 1 and qg * m * 1024 > 128 * 1024:
                qg >>= 1
            if qg > nb:
                qg = 2 if nb >= 2 else 1
            hits["keys_qg%d" % qg] += 1
        hits["keys_words" if m % 4 == 0 else "keys_bytes"] += 1


def draw_case(case):
    """One random case.  Cases 8i, 8i + 1 and 8i + 2 are pinned to a scenario (the index sizes at the filtered form's switch,
    the radix branch of the threshold selection, more queries than one unfiltered key batch) with m cycling through group
    boundaries, so that every path is reached at any seed; the others are drawn freely."""
    scen = {0: "edge", 1: "radix", 2: "multi"}.get(case % 8, "free")
    m = int(rng.choice(M_EDGES)) if rng.random() < 0.6 else int(rng.integers(1, 129))
    if scen == "edge":
        m = [36, 37, 72, 73, 128, 4, 65][(case // 8) % 7]
        n = int(rng.choice([65535, 65536, 65537]))
    elif scen == "radix":
        m = [7, 33, 65, 16, 100][(case // 8) % 5]
        n = log_uniform(FILTER_MIN, 400_000)
    elif scen == "multi":
        n = int(rng.integers(56_000, 65_536))
        m = int(rng.integers(1, 9))
    else:
        n = int(rng.choice([65535, 65536, 65537])) if rng.random() < 0.15 else log_uniform(1, 400_000)
    nq = int(rng.integers(1, 71))
    if scen == "multi":
        nq = max(1, KEY_BUDGET // (n * 8)) + int(rng.integers(1, 70))
    k = log_uniform(1, 1024)
    rf = int(rng.integers(1, 17))
    if scen == "radix":                                  # approxK >= 300: a threshold rank above 256
        k = int(rng.integers(150, 1024)); rf = 2
    return scen, m, n, nq, k, rf


bad, hits, checked, calls = [], {p: 0 for p in PATHS}, 0, 0
for case in range(a.cases):
    scen, m, n, nq, k, rf = draw_case(case)
    lanes = int(rng.choice([1, 4, 8, 16]))
    thr = -1.0 if rng.random() < 0.6 else float(rng.uniform(-0.3, 0.5))
    # candidates: none, sparse, >= 65 536 (filtered), empty
    cand = None
    ck = rng.random()
    if scen not in ("radix", "multi") and ck < 0.3:
        cand = np.sort(rng.choice(n, int(rng.integers(1, max(1, n // 4) + 1)), replace=False)).astype(np.uint32)
    elif scen != "multi" and ck < 0.45 and n > FILTER_MIN:
        cand = np.sort(rng.choice(n, int(rng.integers(FILTER_MIN, n + 1)), replace=False)).astype(np.uint32)
    elif scen == "free" and ck < 0.5:
        cand = np.zeros(0, np.uint32)
    n_items = n if cand is None else cand.size
    while rf > 1 and min(n_items, max(k, k * rf)) > 2047:      # approxK <= 2047 (pq_api.cpp refuses more)
        rf -= 1
    approx = min(n_items, max(k, k * rf))
    # the rows the re-rank reads: an identity map over the index, or many-to-one with rows the table lost
    identity = n <= 20_000 and rng.random() < 0.4
    n_rows = n if identity else int(rng.integers(1, 20_001))
    ds = int(rng.choice([1, 2, 4]))
    use_pq = m * ds <= 512 and n_rows >= 1 and rng.random() < 0.5
    dim = m * ds if use_pq else int(rng.integers(1, 257))
    rows = rng.standard_normal((n_rows, dim)).astype(np.float32) * rng.uniform(0.25, 4.0, (n_rows, 1)).astype(np.float32)
    if n_rows > 40:
        src = int(rng.integers(0, n_rows)); lo = int(rng.integers(0, n_rows - 20))
        rows[lo:lo + int(rng.integers(2, 20))] = rows[src]                     # equal exact similarities: the chunk rank decides
    roi = None
    if not identity:
        roi = rng.integers(0, n_rows, n).astype(np.uint32)
        lost = rng.random(n) < rng.choice([0.0, 0.01, 0.2])
        roi[lost] = n_rows + rng.integers(0, 100, int(lost.sum())).astype(np.uint32)
    pq = _pq.Pq(_pq.unit(rows), m, int(rng.integers(0, 1 << 30))) if use_pq else None
    if pq is not None and identity and n <= 5000:
        codes = pq.encode(_pq.unit(rows))
    else:
        codes = rng.integers(0, 256, (n, m)).astype(np.uint8)
    if n > 100 and rng.random() < 0.5:
        lo = int(rng.integers(0, n - 64)); codes[lo:lo + int(rng.integers(2, 64))] = codes[lo]   # equal ADC scores: tie key decides
    keys = None
    if rng.random() < 0.7:
        keys = rng.integers(0, 1 << 63, n, dtype=np.uint64)
        if n > 10 and rng.random() < 0.3:
            keys[rng.choice(n, n // 10, replace=False)] = keys[0]               # equal tie keys: the index decides
    rank = rng.permutation(n_rows).astype(np.uint32) if rng.random() < 0.5 else None
    queries = rng.standard_normal((nq, dim)).astype(np.float32) * np.float32(rng.uniform(0.1, 3.0))
    if n_rows > 0 and nq > 1 and rng.random() < 0.5:
        queries[0] = rows[int(rng.integers(0, n_rows))] * np.float32(0.7)
    if nq > 2 and rng.random() < 0.3:
        queries[int(rng.integers(0, nq))] = 0.0                                 # refused: norm^2 <= 1e-20
    if nq > 2 and rng.random() < 0.3:
        queries[int(rng.integers(0, nq))] = np.float32(1e-12)
    if pq is not None:
        luts = np.stack([pq.lut(q) if float((q.astype(np.float64) ** 2).sum()) > 1e-20 else np.zeros((m, 256), np.float32)
                         for q in queries])
    else:
        luts = (rng.standard_normal((nq, m, 256)) * rng.uniform(0.01, 1.0)).astype(np.float32)
    for qi in range(nq):                                                        # coarse or all-equal tables: fallbacks
        u = rng.random()
        if u < 0.05:
            luts[qi] = 0.0
        elif u < 0.12:
            luts[qi] = np.round(luts[qi] * 4) / 4
    pick = {0, nq - 1}
    if scen == "multi":
        batch = max(1, KEY_BUDGET // (n_items * 8))
        pick |= {batch - 1, batch, min(batch + 1, nq - 1)}
    while len(pick) < min(6, nq):
        pick.add(int(rng.integers(0, nq)))
    d_rows = acc.to_device(rows)
    bufs = [d_rows]
    tie_p = inv_p = None
    if rank is not None:
        inv = np.empty_like(rank); inv[rank] = np.arange(n_rows, dtype=np.uint32)
        bufs += [acc.to_device(rank), acc.to_device(inv)]
        tie_p, inv_p = bufs[1].ptr, bufs[2].ptr
    desc = {"case": case, "scen": scen, "n": n, "n_items": n_items, "m": m, "nq": nq, "k": k, "rf": rf, "lanes": lanes,
            "thr": thr, "dim": dim, "pq": use_pq, "identity": identity, "rank": rank is not None, "keys": keys is not None}
    try:
        v = acc.corpus_view(d_rows.ptr, n_rows, dim, tie_rank_ptr=tie_p, rank_row_ptr=inv_p)
        r = acc.scan_pq_topk(v, codes, luts, queries, k, thr, rf, tie_keys=keys, row_of_index=roi, candidates=cand, sum_lanes=lanes)
    except Exception as e:                                                      # every drawn call is a valid one
        bad.append(dict(desc, error=str(e)[:200]))
        for b in bufs:
            b.free()
        break
    for b in bufs:
        b.free()
    calls += 1
    fb = int(r.diag["exact_fallback_queries"])
    if n_items:
        paths_of(n_items, m, nq, approx, fb, hits)
    for qi in sorted(pick):
        e_rows, e_sims, _ = o.pq_search(rows, codes, luts[qi], queries[qi], k, thr, rf, tie_keys=keys, row_of_index=roi,
                                        chunk_rank=rank.astype(np.uint64) if rank is not None else None, candidates=cand,
                                        sum_lanes=lanes)
        cnt = int(r.counts[qi])
        checked += 1
        why = None
        if cnt != len(e_rows):
            why = "count %d != %d" % (cnt, len(e_rows))
        elif r.rows[qi, :cnt].tolist() != e_rows.tolist():
            why = "rows"
        elif not np.array_equal(r.scores[qi, :cnt].view(np.uint32), e_sims.view(np.uint32)):
            why = "score bits"
        if why:
            bad.append(dict(desc, query=qi, why=why, fallback=fb))
            break
print(json.dumps({"cases": a.cases, "calls": calls, "mismatches": len(bad), "checked_queries": checked, "paths": hits,
                  "first_bad": bad[:3]}))
sys.exit(1 if bad else 0)
