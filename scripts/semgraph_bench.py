"""The device semantic-neighbour graph (yams_graph_semantic_neighbors_device) — the measurements of DESIGN 3.11:

  1. the full call (every row a source, K = 8, adaptive mode, with a tie_rank table) at 20 000 x 384 and at 54 000 x 1024
  2. the pairs kernel's share of it (the context's own event brackets) and its achieved fp64 multiply-add rate against
     N^2 * D and the 39.3 T FMA/s of the vendor sheet
  3. the CPU side: a plain C restatement of the reference-shaped loop, -O2, one core of the same machine, over a SAMPLE of
     sources of the same corpus, scaled to all of them (the loop's cost per source does not depend on the source)

    python scripts/semgraph_bench.py [--reps 3] [--out profiles/semantic_graph.json] [--only small] [--cpu-sources 16]
    python scripts/semgraph_bench.py --rocprof-stats kernel_stats.csv --out profiles/semantic_graph.json

HIP events around calls that end in a synchronise, one warm-up call first, each figure the median of --reps calls.  --only
small runs the first shape alone (the run to put under `rocprofv3 --kernel-trace --stats`, in a run of its own);
--rocprof-stats folds that run's kernel summary into an existing output file.  No pass mark is set for the rate: it is a
first measurement.  Figures that were not taken on a device are recorded as "not_run"."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yams_amd.accel import Accel  # noqa: E402

SHEET_TFMA = 39.3          # fp64 vector multiply-adds per second, vendor sheet (78.6 TFLOP/s)

CPU_LOOP = r'''
/* The reference-shaped pair loop restated in C: per source a scalar fp64 dot with every other row, float inverse norms, the
   min-replacement top-K.  Returns the number of pairs scored. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
uint64_t semgraph_cpu(const float* x, uint32_t n, uint32_t dim, const float* inv, const uint32_t* sources, uint32_t n_sources,
                      uint32_t k, uint32_t* out_rows, float* out_sims) {
    uint64_t scored = 0;
    for (uint32_t s = 0; s < n_sources; ++s) {
        const uint32_t src = sources[s];
        const float* a = x + (size_t)src * dim;
        uint32_t have = 0;
        uint32_t* rows = out_rows + (size_t)s * k; float* sims = out_sims + (size_t)s * k;
        for (uint32_t r = 0; r < n; ++r) {
            if (r == src) continue;
            const float* b = x + (size_t)r * dim;
            double dot = 0.0;
            for (uint32_t i = 0; i < dim; ++i) dot += (double)a[i] * (double)b[i];
            const float sim = (float)(dot * inv[src] * inv[r]);
            ++scored;
            if (sim <= 0.0f) continue;
            if (have < k) { rows[have] = r; sims[have] = sim; ++have; continue; }
            uint32_t w = 0;
            for (uint32_t j = 1; j < k; ++j) if (sims[j] < sims[w] || (sims[j] == sims[w] && rows[j] > rows[w])) w = j;
            if (sim > sims[w] || (sim == sims[w] && r < rows[w])) { rows[w] = r; sims[w] = sim; }
        }
    }
    return scored;
}
'''


def cpu_loop(rows, inv, sources, k):
    """Seconds the C restatement takes on one core for the given sources, and the best similarity per source."""
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "semgraph_cpu.c"); lib = os.path.join(tmp, "semgraph_cpu.so")
        open(src, "w").write(CPU_LOOP)
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", lib, src, "-lm"], check=True)
        L = C.CDLL(lib)
        L.semgraph_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.semgraph_cpu.restype = C.c_uint64
        o_r = np.zeros((len(sources), k), np.uint32); o_s = np.zeros((len(sources), k), np.float32)
        t0 = time.perf_counter()
        scored = L.semgraph_cpu(rows.ctypes.data, rows.shape[0], rows.shape[1], inv.ctypes.data, sources.ctypes.data, len(sources), k,
                                o_r.ctypes.data, o_s.ctypes.data)
        return time.perf_counter() - t0, scored, o_s.max(axis=1)


def rocprof_summary(path):
    """The per-kernel rows of a rocprofv3 --stats kernel summary (kernel_stats.csv)."""
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "semgraph" in name:
                out.append({"kernel": name.split("(")[0], "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                            "average_ns": float(r["AverageNs"]), "percent": float(r["Percentage"])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["all", "small"], default="all")
    ap.add_argument("--cpu-sources", type=int, default=16)
    ap.add_argument("--rocprof-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rocprof_stats and a.out and os.path.exists(a.out):       # fold a profiler summary into an existing result file
        res = json.load(open(a.out))
        res["rocprofv3_kernel_stats_20000x384"] = rocprof_summary(a.rocprof_stats)
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps(res["rocprofv3_kernel_stats_20000x384"]))
        return
    import torch
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    K = 8

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1), out

    def full_call(n, dim, reps, cpu_sources):
        rows = torch.empty((n, dim), dtype=torch.float32, device="cuda")
        acc.synth_rows(11, 0, n, dim, rows.data_ptr())
        rank = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n)).to(torch.int32)
        o_r = torch.empty((n, K), dtype=torch.int32, device="cuda"); o_s = torch.empty((n, K), dtype=torch.float32, device="cuda")
        o_c = torch.empty(n, dtype=torch.int32, device="cuda"); o_i = torch.empty(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        call = lambda: acc.semantic_neighbors_device(rows.data_ptr(), n, dim, K, o_r.data_ptr(), o_s.data_ptr(), o_c.data_ptr(),
                                                     tie_rank_ptr=rank.data_ptr(), out_inv_norm_ptr=o_i.data_ptr())
        call()                                                  # warm-up: workspace allocation, code objects
        acc.enable_timing(True)
        ts = []
        for _ in range(reps):
            ms, diag = timed(call)
            ts.append(ms)
        pairs_ms, _ = acc.kernel_ms("semgraph_pairs")
        norm_ms, _ = acc.kernel_ms("semgraph_norm")
        merge_ms, _ = acc.kernel_ms("semgraph_merge")
        acc.enable_timing(False)
        ms = float(np.median(ts))
        fma = n * n * dim
        out = {"rows": n, "dim": dim, "k": K, "ms": ms, "ms_all_reps": ts, "norm_ms": norm_ms, "pairs_ms": pairs_ms, "merge_ms": merge_ms, **diag,
               "fma_n2d": fma, "call_fp64_TFMA_per_s": fma / ms / 1e9, "pairs_kernel_fp64_TFMA_per_s": fma / pairs_ms / 1e9,
               "pairs_kernel_frac_of_39.3_TFMA_vendor_sheet": fma / pairs_ms / 1e9 / SHEET_TFMA,
               "projected_ms_at_vendor_sheet_rate": fma / SHEET_TFMA / 1e9}
        if cpu_sources:
            h = rows.cpu().numpy(); inv = o_i.cpu().numpy()
            sources = np.linspace(0, n - 1, cpu_sources).astype(np.uint32)
            sec, scored, best = cpu_loop(h, inv, sources, K)
            same = bool(np.array_equal(best.view(np.uint32), o_s.cpu().numpy()[sources, 0].view(np.uint32)))
            out["cpu_c_restatement"] = {"sampled_sources": int(cpu_sources), "seconds_for_the_sample": sec, "pairs_scored": int(scored), "flags": "-O2, one core",
                                        "seconds_scaled_to_all_sources": sec * n / cpu_sources, "best_similarity_bits_equal_the_device": same}
            out["device_over_cpu"] = {"cpu_s_scaled": sec * n / cpu_sources, "device_s": ms / 1e3, "ratio": sec * n / cpu_sources / (ms / 1e3)}
        return out

    info = acc.device_info()
    res = {"device": {k2: info[k2] for k2 in ("name", "arch", "compute_units") if k2 in info}, "reps": a.reps, "sheet_fp64_TFMA_per_s": SHEET_TFMA}
    res["full_20000x384"] = full_call(20_000, 384, a.reps, a.cpu_sources if a.only == "all" else 0)
    if a.only == "all":
        res["full_54000x1024"] = full_call(54_000, 1024, a.reps, a.cpu_sources)
        res["rocprofv3_kernel_stats_20000x384"] = "not_run"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
