"""The 25 orders of the product-quantised engine's ADC sum (YAMS_PQ_SUM_*: lanes | combine | tail) on the shape of bench.py's
PQ leg — 1M codes x 32 sub-quantisers, 256 queries per batch, top-100, rerank factor 2, index and tables resident — one
yams_scan_pq_topk_device call per step:

    python scripts/pq_sum_bench.py [--reps 3] [--m 32] [--out profiles/pq_sum_orders.json]
    python scripts/pq_sum_bench.py --m 40 ...          # a tail of 8 under 16 lanes: the scalar-tail epilogue does work
    python scripts/pq_sum_bench.py --flags 0,1,2,3 --key this1 ...   # the four orders the parent has: the script runs on the
                                                                      # parent's tree too (same C ABI), for an A/B per order
    python scripts/pq_sum_bench.py --ab-parent-ms 1,2,3 --ab-this-ms 1,2,3 --out profiles/pq_sum_orders.json

HIP events around calls that end in a synchronise, one warm-up call per definition first, each figure the median of --reps
calls; the ADC launches' own time (pq_adc_sample + pq_adc, the context's event pairs) beside it.  No pass mark: a first
measurement.  --ab-*: folds the pq.ms_per_step figures of `bench.py --only-pq` runs of the parent commit and of this one
(same box, same session, alternating) into the output file.  A run without a device fails; nothing is estimated."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yams_amd import _lib  # noqa: E402
from yams_amd.accel import Accel  # noqa: E402

LANES = {0: "seq", 1: "x4", 2: "x8", 3: "x16"}
COMBINE = {0: "", 4: "_halves", 8: "_pairs", 12: "_halves4_pairs"}


def definitions():
    out = [0]
    for l in (1, 2, 3):
        for c in (0, 4, 8, 12):
            for t in (0, 16):
                out.append(l | c | t)
    return out


def name(f):
    return "seq" if f & 3 == 0 else LANES[f & 3] + COMBINE[f & 12] + ("_tail" if f & 16 else "")


def fold_ab(a, res):
    parent = [float(x) for x in a.ab_parent_ms.split(",")]
    this = [float(x) for x in a.ab_this_ms.split(",")]
    spread = max(parent) - min(parent)
    res["bench_pq_leg_ab"] = {
        "what": "pq.ms_per_step of `bench.py --only-pq` (flag word 0: the sequential sum, 40 timed batches each), parent commit and this one, "
                "same box, same session, alternating",
        "parent_ms": parent, "this_ms": this, "parent_median_ms": float(np.median(parent)), "this_median_ms": float(np.median(this)),
        "parent_spread_ms": spread, "this_minus_parent_median_ms": float(np.median(this) - np.median(parent)),
        "within_the_parents_spread": bool(np.median(this) - np.median(parent) <= spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--flags", default=None, help="comma-separated flag words to time instead of all 25 (0,1,2,3: the orders the parent has)")
    ap.add_argument("--key", default=None, help="the section of the output file this run goes to (default: definitions / definitions_m<m>)")
    ap.add_argument("--ab-parent-ms", default=None)
    ap.add_argument("--ab-this-ms", default=None)
    a = ap.parse_args()
    res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    if a.ab_parent_ms and a.ab_this_ms:
        fold_ab(a, res)
    else:
        import torch
        acc = Accel(0, torch.cuda.current_stream().cuda_stream)
        n, d, m, nq, k, rf = 1_000_000, 384, a.m, 256, 100, 2
        g = torch.Generator(device="cuda"); g.manual_seed(73)
        tc = torch.empty((n, d), dtype=torch.float32, device="cuda")
        acc.synth_rows(73, 0, n, d, tc.data_ptr())
        codes = torch.randint(0, 256, (n, m), generator=g, device="cuda", dtype=torch.uint8)
        luts = (torch.randn((nq, m, 256), generator=g, device="cuda") * 0.05).contiguous()
        tq = torch.empty((nq, d), dtype=torch.float32, device="cuda")
        acc.synth_rows(73, 1 << 40, nq, d, tq.data_ptr())
        perm = torch.randperm(n, generator=g, device="cuda").to(torch.int32)
        key_row = torch.empty(n, dtype=torch.int32, device="cuda"); key_row[perm.long()] = torch.arange(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        view = acc.corpus_view(tc.data_ptr(), n, d)
        pq = _lib.ScanPqIndex(codes.data_ptr(), n, m, 0, perm.data_ptr(), key_row.data_ptr())
        o_s = torch.empty((nq, k), dtype=torch.float32, device="cuda"); o_r = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        o_c = torch.empty(nq, dtype=torch.int32, device="cuda")
        diag = _lib.ScanDiag()

        def step(flags, want_diag=False):
            prm = _lib.ScanPqParams(k, -1.0, rf, flags)
            acc._check(acc.L.yams_scan_pq_topk_device(acc.ctx, C.byref(view), C.byref(pq), tq.data_ptr(), luts.data_ptr(), nq, C.byref(prm), None, 0,
                                                      o_s.data_ptr(), o_r.data_ptr(), o_c.data_ptr(), C.byref(diag) if want_diag else None))

        step(0); step(0)                                           # workspace allocation, code objects
        rows = {}
        for f in ([int(x) for x in a.flags.split(",")] if a.flags else definitions()):
            step(f, want_diag=True)                                # this definition's kernels
            fallback = int(diag.as_dict()["exact_fallback_queries"])
            ts = []
            for _ in range(a.reps):
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record(); step(f); e1.record(); e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            acc.enable_timing(True)
            step(f); acc.synchronize()
            adc = sum(acc.kernel_ms(r)[0] or 0.0 for r in ("pq_adc", "pq_adc_sample"))
            acc.enable_timing(False)
            rows[name(f)] = {"flags": f, "ms_per_call": float(np.median(ts)), "ms_all_reps": ts, "adc_launches_ms": adc,
                             "queries_through_the_unfiltered_form": fallback}
        info = acc.device_info()
        key = a.key or ("definitions" if m == 32 else "definitions_m%d" % m)
        res["device"] = {k_: info[k_] for k_ in ("name", "arch", "compute_units") if k_ in info}
        res["shape"] = "1M codes, 256 queries per call, top-100, rerank factor 2; HIP events, median of %d after a warm-up" % a.reps
        res[key] = {"m": m, "per_definition": rows}
        acc.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
