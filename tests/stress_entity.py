"""Randomised stress of the entity-vector search (yams_scan_entity_topk_device) on the GPU against the restatement of
tests/_entity_oracle.py: dims that are not a multiple of four and row pointers that are not 16-byte aligned (the scalar
staging), every query-group form (1 / 4 / 8 queries per workgroup) and ragged last groups, more than one query slice, each
filter field alone and combined, a different filter per query, filters nothing matches, unset attributes, row masks (none,
empty, sparse, dense), zero / NaN / inf rows and queries, duplicate rows (ties), the -0.0f construction, row_base, k,
thresholds.  Test infrastructure.

    python tests/stress_entity.py [--cases 40] [--seed 1]

The harness stops at the first failing case and never retries; the summary counts the code paths the cases reached, as the
host code chooses them (entity_api.cpp, entity_kernels.hip).
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import _entity_oracle as eo
from yams_amd.accel import Accel

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=40)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()
rng = np.random.default_rng(a.seed)
acc = Accel(0, torch.cuda.current_stream().cuda_stream)

KEY_BUDGET = 256 << 20               # entity_api.cpp: bytes of keys one slice of queries may hold (8 per item)
PATHS = ["vec4_0", "vec4_1", "qg1", "qg4", "qg8", "dense", "compacted", "multi_slice", "filters", "mask", "zero_winner"]


def log_uniform(lo, hi):
    return int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1))))


bad, hits, checked = [], {p: 0 for p in PATHS}, 0
for case in range(a.cases):
    slices = case % 10 == 4                                                  # pinned: more than one query slice
    dim = int(rng.choice([1, 3, 33, 50, 4, 32, 64, 100, 128, 384])) if rng.random() < 0.7 else int(rng.integers(1, 520))
    offset = 1 if (dim % 4 == 0 and rng.random() < 0.3) or case % 10 == 1 else 0
    nq = int(rng.choice([1, 2, 3, 4, 5, 8, 9, 17]))
    if slices:
        dim, n, nq = int(rng.choice([3, 8])), int(rng.integers(2_200_000, 2_600_000)), 17
    else:
        n = int(rng.choice([63, 64, 65, 256, 257])) if rng.random() < 0.2 else log_uniform(1, 40_000 if dim <= 128 else 10_000)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    if n > 8:
        for _ in range(int(rng.integers(0, 4))):                            # duplicate rows: equal scores
            src, lo = int(rng.integers(0, n)), int(rng.integers(0, n - 4))
            rows[lo:lo + int(rng.integers(1, 5))] = rows[src]
        rows[int(rng.integers(0, n))] = 0.0
        if rng.random() < 0.4:
            rows[int(rng.integers(0, n)), int(rng.integers(0, dim))] = rng.choice([np.nan, np.inf, -np.inf])
        if dim >= 2 and rng.random() < 0.4:
            r = int(rng.integers(0, n)); rows[r] = 0.0; rows[r, 0] = np.float32(-1e-40); rows[r, 1] = np.float32(1e6)
    types = rng.integers(0, 4, n).astype(np.uint8)
    nodes = rng.integers(0, 5, n).astype(np.uint32)
    docs = rng.integers(0, max(2, n // 20), n).astype(np.uint32)
    if rng.random() < 0.5:
        types[rng.random(n) < 0.1] = eo.TYPE_UNSET; nodes[rng.random(n) < 0.1] = eo.UNSET; docs[rng.random(n) < 0.1] = eo.UNSET
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    u = rng.random()
    if u < 0.15:
        queries[0] = 0.0                                                     # a zero query: every admitted row scores +0.0
    elif u < 0.3:
        queries[0] = 0.0; queries[0, 0] = 1.0                                # e0: the -0.0f row, if drawn, scores -0.0f
    elif u < 0.4:
        queries[0, int(rng.integers(0, dim))] = rng.choice([np.nan, np.inf])
    elif u < 0.7:
        queries[0] = rows[int(rng.integers(0, n))] * np.float32(2.0)
    f = rng.random()
    filters = None
    if f < 0.25:                                                             # every query carries a filter
        filters = [[(int(rng.integers(0, 4)), None, None), (None, int(rng.integers(0, 5)), None), (None, None, int(docs[0])),
                    (int(rng.integers(0, 4)), int(rng.integers(0, 5)), None), (None, None, 1 << 30)][int(rng.integers(0, 5))] for _ in range(nq)]
    elif f < 0.45:                                                           # some do, some do not
        filters = [(int(rng.integers(0, 4)), None, None) if rng.random() < 0.5 else (None, None, None) for _ in range(nq)]
    elif f < 0.55:
        filters = [(None, None, int(docs[int(rng.integers(0, n))]))] * nq    # one small document for every query
    mk = rng.random()
    mask = None
    if mk < 0.1:
        mask = np.zeros(0, np.int64)
    elif mk < 0.3:
        mask = np.sort(rng.choice(n, max(1, int(n * rng.uniform(0.0, 0.1))), replace=False))
    elif mk < 0.45:
        mask = np.sort(rng.choice(n, int(n * rng.uniform(0.2, 1.0)), replace=False))
    row_base = int(rng.choice([0, 0, 7, 1 << 33]))
    k = log_uniform(1, 1024)
    thr = float(rng.choice([-1.0, 0.0, float(rng.uniform(-0.3, 0.4))]))
    desc = {"case": case, "n": n, "dim": dim, "offset": offset, "nq": nq, "k": k, "thr": thr, "filters": filters,
            "mask": None if mask is None else len(mask)}
    try:
        res = eo.run(acc, rows, queries, k, thr, types, nodes, docs, filters, mask, row_base, rows_offset=offset)
    except Exception as e:                                                   # every drawn call is a valid one
        bad.append(dict(desc, error=str(e)[:200]))
        break
    # the paths entity_api.cpp / launch_entity_score chose
    all_restrict = filters is not None and all(any(x is not None for x in fl) for fl in filters)
    compact = mask is not None or all_restrict
    if all_restrict:                                                         # the gather's count sizes keys and slices
        on = np.zeros(n, bool)
        for fl in set(filters):
            on[eo.admitted(n, types, nodes, docs, fl, mask)] = True
        n_items = int(on.sum())
    else:
        n_items = n if mask is None else len(mask)
    slice_q = min(nq, max(1, KEY_BUDGET // (max(n_items, 1) * 8)))
    if slice_q > 8:
        slice_q -= slice_q % 8
    if n_items:
        hits["vec4_1" if dim % 4 == 0 and offset == 0 else "vec4_0"] += 1
        hits["compacted" if compact else "dense"] += 1
        for q0 in range(0, nq, slice_q):
            ns = min(slice_q, nq - q0)
            hits["qg1" if ns == 1 else ("qg4" if ns <= 4 else "qg8")] += 1
        if slice_q < nq:
            hits["multi_slice"] += 1
    hits["filters"] += filters is not None
    hits["mask"] += mask is not None
    pick = {0, nq - 1}
    if slice_q < nq:
        pick |= {slice_q - 1, slice_q}
    while len(pick) < min(4, nq):
        pick.add(int(rng.integers(0, nq)))
    if slices:
        pick = {0, min(slice_q, nq - 1)}                                                  # (the restatement walks 2 M rows per query)
    for qi in sorted(pick):
        checked += 1
        why = eo.compare(res, qi, rows, queries, k, thr, types, nodes, docs, filters, mask, row_base)
        if why:
            bad.append(dict(desc, query=qi, why=why))
            break
        cnt = int(res.counts[qi])
        hits["zero_winner"] += bool(cnt and (res.scores[qi, :cnt] == 0).any())
    if bad:
        break
print(json.dumps({"cases": a.cases, "mismatches": len(bad), "checked_queries": checked, "paths": hits, "first_bad": bad[:3]}, default=str))
sys.exit(1 if bad else 0)
