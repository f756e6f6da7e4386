"""Document-level top-k (yams_scan_doc_topk_device / vector_doc_scan_v1) — the three measurements of DESIGN 3.7:

  1. one query over 1 M x 768 rows / 100 000 documents, every row a candidate: ms and effective GB/s of row bytes
  2. 64 queries on the same shape: ms and the fraction of the fp64 vector FMA peak the scoring reaches
  3. a 100 000-row candidate set through the plugin: the all-rows route the host used before (slices of YAMS_SCAN_MAX_K
     rows through search_batch_masked, every matching row handed back, best row per document on the host) against
     search_docs

    python scripts/doc_topk_bench.py [--reps 10] [--out FILE.json]

Wall-clock per call (each call synchronises its stream), median over --reps after one warm-up call.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from yams_amd import _lib  # noqa: E402
from yams_amd.accel import Accel  # noqa: E402

# MI355X fp64 vector peak (FMA counted as 2 flops): 78.6 TFLOP/s — AMD's published figure for the part, not measured here
FP64_VECTOR_PEAK = 78.6e12


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    import torch
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    L = acc.L
    n, d, n_docs, k = 1_000_000, 768, 100_000, 10
    rows = torch.empty((n, d), dtype=torch.float32, device="cuda")
    acc.synth_rows(5, 0, n, d, rows.data_ptr())
    row_doc = (torch.arange(n, device="cuda", dtype=torch.int64) * n_docs // n).to(torch.int32)   # contiguous documents
    rng = np.random.default_rng(5)
    doc_rank = torch.from_numpy(rng.permutation(n_docs).astype(np.int32)).cuda()
    queries = torch.empty((64, d), dtype=torch.float32, device="cuda")
    acc.synth_rows(5, 1 << 40, 64, d, queries.data_ptr())
    out_s = torch.empty(64 * k, dtype=torch.float32, device="cuda"); out_r = torch.empty(64 * k, dtype=torch.int64, device="cuda")
    out_d = torch.empty(64 * k, dtype=torch.int32, device="cuda"); out_n = torch.empty(64, dtype=torch.int32, device="cuda")
    out_m = torch.empty(64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    corpus = acc.corpus_view(rows.data_ptr(), n, d)
    docs = acc.docs_view(row_doc.data_ptr(), n_docs, doc_rank.data_ptr())
    prm = _lib.ScanParams(k, -1.0, _lib.SCAN_COSINE, 0)
    diag = _lib.ScanDiag()

    def call(nq):
        acc._check(L.yams_scan_doc_topk_device(acc.ctx, C.byref(corpus), C.byref(docs), queries.data_ptr(), nq, C.byref(prm),
                                               out_s.data_ptr(), out_r.data_ptr(), out_d.data_ptr(), out_n.data_ptr(),
                                               out_m.data_ptr(), C.byref(diag)))
    res = {"shape": {"rows": n, "dim": d, "docs": n_docs, "k": k}, "reps": a.reps,
           "fp64_vector_peak_tflops": FP64_VECTOR_PEAK / 1e12, "fp64_peak_source": "AMD published MI355X figure (not measured here)"}
    row_bytes = n * d * 4
    ms1 = median_ms(lambda: call(1), a.reps)
    res["single_query"] = {"ms": ms1, "row_GB_per_s": row_bytes / ms1 / 1e6, "hbm_floor_ms_at_8TBps": row_bytes / 8e12 * 1e3}
    ms64 = median_ms(lambda: call(64), a.reps)
    flops = 64 * n * d * 2 * (1 + 1 / 64)          # one fp64 FMA per element per query + the shared norm
    passes = (64 + 7) // 8                          # the rows are read once per group of 8 queries
    res["q64"] = {"ms": ms64, "fp64_tflops": flops / ms64 / 1e9, "frac_fp64_peak": flops / ms64 / 1e9 / (FP64_VECTOR_PEAK / 1e12),
                  "row_passes": passes, "row_GB_per_s": passes * row_bytes / ms64 / 1e6}

    # 3. the candidate-set case through the plugin boundary
    L.yams_plugin_shutdown()
    assert L.yams_plugin_init(b'{"device": 0}', None) == 0
    p = C.c_void_p(); pd = C.c_void_p()
    assert L.yams_plugin_get_interface(b"vector_scan_v1", 2, C.byref(p)) == 0
    assert L.yams_plugin_get_interface(b"vector_doc_scan_v1", 1, C.byref(pd)) == 0
    vs = C.cast(p, C.POINTER(_lib.VectorScanV1)).contents
    ds = C.cast(pd, C.POINTER(_lib.VectorDocScanV1)).contents
    nc, dc = 1_000_000, 768
    host_rows = rows.cpu().numpy()
    cid = C.c_uint64()
    assert vs.corpus_create(None, dc, C.byref(cid)) == 0
    assert vs.corpus_append(None, cid, host_rows.ctypes.data_as(_lib.f32p), nc) == 0
    h_doc = (np.arange(nc, dtype=np.int64) * n_docs // nc).astype(np.uint32)
    h_rank = doc_rank.cpu().numpy().astype(np.uint32)
    assert ds.corpus_set_documents(None, cid, h_doc.ctypes.data_as(_lib.u32p), nc, h_rank.ctypes.data_as(_lib.u32p), n_docs) == 0
    cand_docs = rng.choice(n_docs, 10_000, replace=False)                     # 10 rows per document: 100 000 rows
    cand = np.nonzero(np.isin(h_doc, cand_docs))[0]
    words = np.zeros((nc + 31) // 32, np.uint32)
    np.bitwise_or.at(words, cand >> 5, (np.uint32(1) << (cand & 31).astype(np.uint32)))
    q = np.ascontiguousarray(queries[:1].cpu().numpy())

    def new_route():
        hits = C.POINTER(_lib.ScanHit)(); counts = _lib.u32p(); m = np.zeros(1, np.uint64); dg = _lib.ScanDiag()
        assert ds.search_docs(None, cid, q.ctypes.data_as(_lib.f32p), 1, dc, k, -1.0, words.ctypes.data_as(_lib.u32p), C.byref(hits),
                              C.byref(counts), m.ctypes.data_as(_lib.u64p), C.byref(dg)) == 0
        out = [(hits[i].row, hits[i].similarity) for i in range(counts[0])]
        ds.free_doc_hits(None, hits, counts)
        return out

    def old_route():
        found = []
        for s0 in range(0, len(cand), 1024):                  # YAMS_SCAN_MAX_K rows per call
            part = cand[s0:s0 + 1024]
            w = np.zeros_like(words)
            np.bitwise_or.at(w, part >> 5, (np.uint32(1) << (part & 31).astype(np.uint32)))
            hits = C.POINTER(_lib.ScanHit)(); counts = _lib.u32p(); dg = _lib.ScanDiag()
            assert vs.search_batch_masked(None, cid, q.ctypes.data_as(_lib.f32p), 1, dc, len(part), -1.0, 0, w.ctypes.data_as(_lib.u32p),
                                          C.byref(hits), C.byref(counts), C.byref(dg)) == 0
            found += [(hits[i].row, hits[i].similarity) for i in range(counts[0])]
            vs.free_hits(None, hits, counts)
        best = {}
        for r, s in found:                                      # the host's reduction (records not materialised here)
            dd = h_doc[r]
            if dd not in best or s > best[dd][1] or (s == best[dd][1] and r < best[dd][0]):
                best[dd] = (r, s)
        top = sorted(best.items(), key=lambda t: (-t[1][1], h_rank[t[0]]))[:k]
        return [v for _, v in top]

    assert [r for r, _ in new_route()] == [r for r, _ in old_route()]
    ms_new = median_ms(new_route, a.reps)
    ms_old = median_ms(old_route, max(2, a.reps // 4))
    res["candidates_100k"] = {"rows": int(len(cand)), "search_docs_ms": ms_new, "old_route_ms": ms_old, "speedup": ms_old / ms_new,
                              "old_route_note": "98 device calls of <= 1024 rows + the best-row reduction; the host's VectorRecord "
                                                "copies (embeddings) of every matching row are not included: a lower bound"}
    assert vs.corpus_destroy(None, cid) == 0
    L.yams_plugin_shutdown()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
