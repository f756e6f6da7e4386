"""Randomised stress of document-level top-k (yams_scan_doc_topk_device) on the GPU against the oracle: dims that are not
a multiple of four and row pointers that are not 16-byte aligned (the scalar staging of doc_score_kernel), every query-group
form (1 / 4 / 8 queries per workgroup) and ragged last groups, document counts around the select cap (4096) and above the
query-slice budget (more than one slice), contiguous / interleaved / random layouts and document runs that start and end at
wave (64) and workgroup (256) boundaries (the segmented max), rows without a document, duplicate rows (ties), tie ranks and
document ranks on or off, row_base, allow-masks (none, empty, sparse, dense, and at the sparse/dense switch +-1), k,
thresholds.  The expected result of a query is the oracle's matching rows of the allowed set reduced by the restatement
of retainBestRecordPerDocument (tests/_doc_oracle.py); rows, document ordinals, score bits, counts and matching-row counts
of every checked query must be identical.  Test infrastructure (uses oracle/).

    python tests/stress_doc.py [--cases 40] [--seed 1]

The summary counts the code paths the cases reached, as the host code chooses them (doc_api.cpp, doc_kernels.hip).
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import _oracle
from _doc_oracle import NO_DOC, compare, run
from yams_amd.accel import Accel

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=40)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()
rng = np.random.default_rng(a.seed)
acc = Accel(0, torch.cuda.current_stream().cuda_stream)
o = _oracle.oracle()

KEY_BUDGET = 256 << 20               # doc_api.cpp: bytes of per-document keys one slice of queries may hold (16 per document)
SPARSE_DIVISOR = 8                   # doc_api.cpp: a mask that lets fewer than n_rows / 8 rows through is gathered first
PATHS = ["vec4_0", "vec4_1", "qg1", "qg4", "qg8", "mask_sparse", "mask_dense", "multi_slice"]


def log_uniform(lo, hi):
    return int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1))))


def layout(n, n_docs, kind):
    if kind == "contiguous" and n_docs > 1 and n > 1:
        cuts = np.sort(rng.choice(np.arange(1, n), min(n_docs, n) - 1, replace=False))
        d = np.repeat(np.arange(min(n_docs, n)), np.diff(np.concatenate([[0], cuts, [n]])))
        return (d * (n_docs // min(n_docs, n))).astype(np.uint32)           # (spread over the ordinals when n_docs > n)
    if kind == "interleaved":
        return (np.arange(n) % n_docs).astype(np.uint32)
    if kind == "boundary":                                                   # runs that start / end at 64- and 256-row edges
        runs, tot = [], 0
        while tot < n:
            ln = int(rng.choice([1, 2, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 512]))
            runs.append(min(ln, n - tot)); tot += runs[-1]
        docs = rng.integers(0, n_docs, len(runs))
        return np.repeat(docs, runs).astype(np.uint32)
    return rng.integers(0, n_docs, n).astype(np.uint32)


bad, hits, checked = [], {p: 0 for p in PATHS}, 0
for case in range(a.cases):
    slices = case % 10 == 4                                                  # pinned: more than one query slice
    dim = int(rng.choice([1, 3, 33, 385, 4, 32, 64, 100, 128, 256])) if rng.random() < 0.7 else int(rng.integers(1, 520))
    if dim > 256 and slices:
        dim = 33
    offset = 1 if (dim % 4 == 0 and rng.random() < 0.3) or case % 10 == 1 else 0
    u = rng.random()
    n = int(rng.choice([63, 64, 65, 256, 257])) if u < 0.2 else log_uniform(1, 50_000 if dim <= 128 else 12_000)
    nq = int(rng.choice([1, 2, 3, 4, 5, 8, 9, 17]))
    v = rng.random()
    if slices:
        n_docs = int(rng.integers(1_000_000, 2_500_000)); nq = 17
    elif v < 0.25:
        n_docs = int(rng.choice([4095, 4096, 4097]))
    else:
        n_docs = log_uniform(1, max(2, int(n * 1.3)))
    kind = str(rng.choice(["contiguous", "interleaved", "random", "boundary"]))
    row_doc = layout(n, n_docs, kind)
    if rng.random() < 0.5:
        row_doc[rng.random(n) < rng.uniform(0.0, 0.3)] = NO_DOC             # rows without a document: counted, never returned
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    if n > 8:
        for _ in range(int(rng.integers(0, 4))):                            # duplicate rows: equal scores in and across documents
            src, lo = int(rng.integers(0, n)), int(rng.integers(0, n - 4))
            rows[lo:lo + int(rng.integers(1, 5))] = rows[src]
        rows[int(rng.integers(0, n))] = 0.0                                 # zero norm: never matches
        if rng.random() < 0.3:
            rows[int(rng.integers(0, n)), int(rng.integers(0, dim))] = np.nan
    tie = rng.permutation(n).astype(np.uint32) if rng.random() < 0.5 else None
    doc_rank = rng.permutation(n_docs).astype(np.uint32) if rng.random() < 0.5 else None
    row_base = int(rng.choice([0, 0, 7, 1 << 33]))
    mk = rng.random()
    mask = None
    if mk < 0.15:
        mask = np.zeros(0, np.int64)                                         # empty
    elif mk < 0.35:
        mask = np.sort(rng.choice(n, max(1, int(n * rng.uniform(0.0, 0.12))), replace=False))
    elif mk < 0.5:
        mask = np.sort(rng.choice(n, int(n * rng.uniform(0.2, 1.0)), replace=False))
    elif mk < 0.65:
        at = -(-n // SPARSE_DIVISOR) + int(rng.integers(-1, 2))             # the switch +-1
        mask = np.sort(rng.choice(n, min(max(at, 0), n), replace=False))
    k = log_uniform(1, 1024)
    thr = -1.0 if rng.random() < 0.5 else float(rng.uniform(-0.3, 0.4))
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    if n and rng.random() < 0.5:
        queries[0] = rows[int(rng.integers(0, n))] * np.float32(2.0)         # a (possibly duplicated) row: ties decide
        if not np.isfinite(queries[0]).all() or not float((queries[0].astype(np.float64) ** 2).sum()) > 1e-6:
            queries[0] = rng.standard_normal(dim).astype(np.float32)
    desc = {"case": case, "n": n, "dim": dim, "offset": offset, "nq": nq, "n_docs": n_docs, "layout": kind, "k": k, "thr": thr,
            "tie": tie is not None, "doc_rank": doc_rank is not None, "mask": None if mask is None else len(mask)}
    try:
        res = run(acc, rows, queries, k, thr, row_doc, n_docs, tie, doc_rank, mask, row_base, rows_offset=offset)
    except Exception as e:                                                   # every drawn call is a valid one
        bad.append(dict(desc, error=str(e)[:200]))
        break
    n_eff = n if mask is None else len(mask)
    if res.diag["rows_visited"] != nq * n_eff or res.diag["returned_rows"] != int(res.matching.sum()):
        bad.append(dict(desc, why="diagnostics", diag=res.diag))
        break
    # the paths doc_api.cpp / launch_doc_score chose
    slice_q = min(nq, max(1, KEY_BUDGET // (max(n_docs, 1) * 16)))
    if n_eff:
        hits["vec4_1" if dim % 4 == 0 and offset == 0 else "vec4_0"] += 1
        for q0 in range(0, nq, slice_q):
            ns = min(slice_q, nq - q0)
            hits["qg1" if ns == 1 else ("qg4" if ns <= 4 else "qg8")] += 1
    if mask is not None:
        hits["mask_sparse" if n_eff * SPARSE_DIVISOR < n else "mask_dense"] += 1
    if slice_q < nq:
        hits["multi_slice"] += 1
    pick = {0, nq - 1}
    if slice_q < nq:
        pick |= {slice_q - 1, slice_q}
    while len(pick) < min(5, nq):
        pick.add(int(rng.integers(0, nq)))
    allowed = None if mask is None else mask
    for qi in sorted(pick):
        checked += 1
        why = compare(o, res, rows, queries, qi, k, thr, row_doc, tie, doc_rank, allowed, row_base)
        if why:
            bad.append(dict(desc, query=qi, why=why))
            break
    if bad:
        break
print(json.dumps({"cases": a.cases, "mismatches": len(bad), "checked_queries": checked, "paths": hits, "first_bad": bad[:3]}))
sys.exit(1 if bad else 0)
