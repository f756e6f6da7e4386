"""Entity-vector search (yams_scan_entity_topk_device) — the measurements of DESIGN 3.8:

  1. yardstick beside the new entry: yams_scan_doc_topk_device over the same 1 M x 768 rows, one query, k = 10,
     threshold -1, every row its own document, alternating with the unfiltered entity search in the same process
  2. filtered: embedding_type admitting about a quarter of randomly interleaved rows; document_hash admitting 0.1 %
  3. 8 and 64 queries per call (one filter, and eight different filters); a 10k x 384 corpus with one query
  4. the CPU side: the vectorised numpy restatement over 50 000 x 768 rows on one core (a restatement: the reference's own
     function also parses twelve text columns per row, which this figure leaves out)

    python scripts/entity_bench.py [--reps 50] [--out profiles/entity_search.json]

Device events around calls that end in a synchronise, warm-up first, each figure the median of --reps calls.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yams_amd import _lib  # noqa: E402
from yams_amd.accel import Accel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    L = acc.L
    n, d, k = a.rows, 768, 10
    rows = torch.empty((n, d), dtype=torch.float32, device="cuda")
    acc.synth_rows(5, 0, n, d, rows.data_ptr())
    queries = torch.empty((64, d), dtype=torch.float32, device="cuda")
    acc.synth_rows(5, 1 << 40, 64, d, queries.data_ptr())
    rng = np.random.default_rng(5)
    types = torch.from_numpy(rng.integers(0, 4, n).astype(np.uint8)).cuda()                 # a quarter per type, interleaved
    nodes = torch.from_numpy(rng.integers(0, 8, n).astype(np.int32)).cuda()
    docs = torch.from_numpy(rng.integers(0, 1000, n).astype(np.int32)).cuda()               # 0.1 % per document, interleaved
    own_doc = torch.arange(n, device="cuda", dtype=torch.int32)                             # the yardstick: every row its own document
    out_s = torch.empty(64 * k, dtype=torch.float32, device="cuda"); out_r = torch.empty(64 * k, dtype=torch.int64, device="cuda")
    out_d = torch.empty(64 * k, dtype=torch.int32, device="cuda"); out_n = torch.empty(64, dtype=torch.int32, device="cuda")
    out_m = torch.empty(64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    corpus = acc.corpus_view(rows.data_ptr(), n, d)
    ents = acc.entities_view(types.data_ptr(), nodes.data_ptr(), docs.data_ptr())
    dview = acc.docs_view(own_doc.data_ptr(), n)
    prm = _lib.ScanParams(k, -1.0, _lib.SCAN_COSINE, 0)
    diag = _lib.ScanDiag()

    def filt(items):
        arr = (_lib.EntityFilter * len(items))()
        for i, (t, nt, dc) in enumerate(items):
            arr[i] = _lib.EntityFilter((1 if t is not None else 0) | (2 if nt is not None else 0) | (4 if dc is not None else 0), t or 0, nt or 0, dc or 0)
        return arr

    def form(fl, cv=corpus):
        """The row walk entity_api.cpp takes for this call: the gathered list when a row mask or a filter on EVERY query
        restricts the rows, else every row."""
        return "compacted" if cv.row_mask or (fl is not None and all(f.fields for f in fl)) else "dense"

    def entity(nq, fl=None, cv=corpus, q=queries):
        acc._check(L.yams_scan_entity_topk_device(acc.ctx, C.byref(cv), C.byref(ents), q.data_ptr(), fl, nq, k, -1.0, out_s.data_ptr(),
                                                  out_r.data_ptr(), out_n.data_ptr(), out_m.data_ptr(), C.byref(diag)))

    def yardstick():
        acc._check(L.yams_scan_doc_topk_device(acc.ctx, C.byref(corpus), C.byref(dview), queries.data_ptr(), 1, C.byref(prm), out_s.data_ptr(),
                                               out_r.data_ptr(), out_d.data_ptr(), out_n.data_ptr(), out_m.data_ptr(), C.byref(diag)))

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    def median(fn, reps=a.reps):
        for _ in range(3):
            fn()
        return float(np.median([timed(fn) for _ in range(reps)]))

    row_bytes = n * d * 4
    info = acc.device_info()
    res = {"device": {k2: info[k2] for k2 in ("name", "arch", "compute_units") if k2 in info}, "shape": {"rows": n, "dim": d, "k": k, "threshold": -1.0}, "reps": a.reps, "row_bytes": row_bytes}
    # 1. yardstick and the new entry, alternating
    for _ in range(3):
        yardstick(); entity(1)
    ty, te = [], []
    for _ in range(a.reps):
        ty.append(timed(yardstick)); te.append(timed(lambda: entity(1)))
    my, me = float(np.median(ty)), float(np.median(te))
    res["unfiltered_one_query"] = {"doc_topk_yardstick_ms": my, "entity_ms": me, "ratio": me / my, "bar": 1.10, "form": form(None),
                                   "entity_row_TB_per_s": row_bytes / me / 1e9, "frac_of_8TBps_peak": row_bytes / me / 1e9 / 8.0,
                                   "frac_of_6.3TBps_achievable": row_bytes / me / 1e9 / 6.3}
    # 2. filtered
    for name, f in (("embedding_type_quarter", (1, None, None)), ("document_hash_0.1pct", (None, None, 7))):
        fl1 = filt([f])
        ms = median(lambda: entity(1, fl1))
        res[name] = {"ms": ms, "rows_admitted": int(diag.rows_visited), "bytes_admitted": int(diag.rows_visited) * d * 4, "form": form(fl1),
                     "admitted_TB_per_s": int(diag.rows_visited) * d * 4 / ms / 1e9}
    # 3. batches and the latency case
    res["q8_one_filter"] = {"ms": median(lambda: entity(8, filt([(1, None, None)] * 8)), max(10, a.reps // 5))}
    res["q8_eight_filters"] = {"ms": median(lambda: entity(8, filt([(i % 4, i % 8, None) for i in range(8)])), max(10, a.reps // 5))}
    res["q64_no_filter"] = {"ms": median(lambda: entity(64), max(5, a.reps // 10))}
    res["q64_one_filter"] = {"ms": median(lambda: entity(64, filt([(1, None, None)] * 64)), max(5, a.reps // 10))}
    small = acc.corpus_view(rows.data_ptr(), 10_000, 384)
    res["latency_10k_x_384_one_query"] = {"ms": median(lambda: entity(1, None, small))}
    # 4. the CPU side (one core): the restatement, 50 000 x 768
    h = rows[:50_000].cpu().numpy(); hq = queries[0].cpu().numpy()
    t0 = time.perf_counter()
    dot = np.zeros(len(h)); nb = np.zeros(len(h)); na = 0.0
    for i in range(d):                                          # fp64, one pass over the elements in order
        x = h[:, i].astype(np.float64); qa = float(hq[i])
        dot += qa * x; na += qa * qa; nb += x * x
    (dot / (np.sqrt(na) * np.sqrt(nb))).astype(np.float32)
    res["cpu_restatement_50k_x_768_s"] = time.perf_counter() - t0
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if me > 1.10 * my:
        sys.exit("the unfiltered entity search took %.3f ms, more than 1.10 x the yardstick beside it (%.3f ms)" % (me, my))


if __name__ == "__main__":
    main()
