"""Device k-means (yams_cluster_kmeans_device / yams_cluster_assign_device) — the measurements of DESIGN 3.9:

  1. the full call at 20 000 x 384, default configuration (k = 141, up to 10 iterations)
  2. the full call at 262 144 x 384 (k = 512)
  3. at 1 M x 768 (k = 1000): one assignment pass and the initialisation, from the context's own event brackets
  4. the CPU side: a C restatement of the reference-shaped loop, -O2, one core, 20 000 x 384, on the same machine

    python scripts/kmeans_bench.py [--reps 5] [--out profiles/kmeans.json] [--only small] [--rocprof-stats kernel_stats.csv]

HIP events around calls that end in a synchronise, warm-up first, each figure the median of --reps calls.  The fp64
multiply-add rate is N*K*D per assignment pass over the pass's time.  --only small runs the first call alone (the run to put
under `rocprofv3 --kernel-trace --stats`); --rocprof-stats folds that run's kernel summary into the output file.
"""
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

CPU_LOOP = r'''
/* The reference-shaped CPU loop (scalar fp64 distances evaluated N*K times per pass, fp32 means), restated in C. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
static double dist(const float* a, const float* b, uint32_t dim) {
    double dot = 0, na = 0, nb = 0;
    for (uint32_t i = 0; i < dim; ++i) { dot += (double)a[i] * b[i]; na += (double)a[i] * a[i]; nb += (double)b[i] * b[i]; }
    if (na <= 0 || nb <= 0) return 2.0;
    double c = dot / (sqrt(na) * sqrt(nb));
    return 1.0 - (c < -1.0 ? -1.0 : (1.0 < c ? 1.0 : c));
}
static void unit(float* v, uint32_t dim) {
    double n = 0;
    for (uint32_t i = 0; i < dim; ++i) n += (double)v[i] * v[i];
    if (n > 0) { float inv = (float)(1.0 / sqrt(n)); for (uint32_t i = 0; i < dim; ++i) v[i] *= inv; }
}
/* no repair path: random rows leave no cluster empty (checked: returns -1 if one is) */
int kmeans_cpu(const float* x, uint32_t n, uint32_t dim, uint32_t k, uint32_t iters, uint32_t* member) {
    float* cent = malloc((size_t)k * dim * 4); float* sum = malloc((size_t)k * dim * 4);
    double* md = malloc((size_t)n * 8); char* taken = calloc(n, 1); uint32_t* cnt = malloc((size_t)k * 4);
    memcpy(cent, x, dim * 4); unit(cent, dim); taken[0] = 1;
    for (uint32_t u = 0; u < n; ++u) md[u] = 1.7976931348623157e308;
    for (uint32_t s = 1; s < k; ++s) {
        uint32_t far = n; double fd = -1.0;
        for (uint32_t u = 0; u < n; ++u) {
            if (taken[u]) continue;
            double d = dist(x + (size_t)u * dim, cent + (size_t)(s - 1) * dim, dim);
            if (d < md[u]) md[u] = d;
            if (md[u] > fd) { fd = md[u]; far = u; }
        }
        taken[far] = 1; memcpy(cent + (size_t)s * dim, x + (size_t)far * dim, dim * 4); unit(cent + (size_t)s * dim, dim);
    }
    memset(member, 0, (size_t)n * 4);
    int ran = 0;
    for (uint32_t it = 0; it < iters; ++it) {
        int changed = 0; ++ran;
        for (uint32_t u = 0; u < n; ++u) {
            uint32_t best = 0; double bd = 1.7976931348623157e308;
            for (uint32_t c = 0; c < k; ++c) { double d = dist(x + (size_t)u * dim, cent + (size_t)c * dim, dim); if (d < bd) { bd = d; best = c; } }
            if (best != member[u]) { member[u] = best; changed = 1; }
        }
        memset(sum, 0, (size_t)k * dim * 4); memset(cnt, 0, (size_t)k * 4);
        for (uint32_t u = 0; u < n; ++u) { float* s = sum + (size_t)member[u] * dim; for (uint32_t d = 0; d < dim; ++d) s[d] += x[(size_t)u * dim + d]; ++cnt[member[u]]; }
        for (uint32_t c = 0; c < k; ++c) {
            if (!cnt[c]) return -1;
            for (uint32_t d = 0; d < dim; ++d) cent[(size_t)c * dim + d] = sum[(size_t)c * dim + d] / (float)cnt[c];
            unit(cent + (size_t)c * dim, dim);
        }
        if (!changed) break;
    }
    free(cent); free(sum); free(md); free(taken); free(cnt);
    return ran;
}
'''


def cpu_loop(rows, k, iters):
    """Seconds the C restatement takes on one core, its membership and the iterations it ran."""
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "kmeans_cpu.c"); lib = os.path.join(tmp, "kmeans_cpu.so")
        open(src, "w").write(CPU_LOOP)
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", lib, src, "-lm"], check=True)
        L = C.CDLL(lib)
        L.kmeans_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        member = np.zeros(len(rows), np.uint32)
        t0 = time.perf_counter()
        ran = L.kmeans_cpu(rows.ctypes.data, rows.shape[0], rows.shape[1], k, iters, member.ctypes.data)
        return time.perf_counter() - t0, member, ran


def rocprof_summary(path):
    """The per-kernel rows of a rocprofv3 --stats kernel summary (kernel_stats.csv)."""
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "kmeans" in name:
                out.append({"kernel": name.split("(")[0], "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                            "average_ns": float(r["AverageNs"]), "percent": float(r["Percentage"])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["all", "small"], default="all")
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

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1), out

    def full_call(n, dim, reps):
        rows = torch.empty((n, dim), dtype=torch.float32, device="cuda")
        acc.synth_rows(9, 0, n, dim, rows.data_ptr())
        mem = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        call = lambda: acc.cluster_kmeans_device(rows.data_ptr(), n, dim, 0, 0, mem.data_ptr(), None)
        call()                                                  # warm-up: workspace allocation, code objects
        acc.enable_timing(True)
        ts = []
        for _ in range(reps):
            ms, (k, iters) = timed(call)
            ts.append(ms)
        assign_ms, launches = acc.kernel_ms("kmeans_assign")
        init_ms, _ = acc.kernel_ms("kmeans_init")
        update_ms, _ = acc.kernel_ms("kmeans_update")
        acc.enable_timing(False)
        ms = float(np.median(ts))
        return rows, mem, {"rows": n, "dim": dim, "k": k, "iterations": iters, "ms": ms, "init_ms": init_ms, "assign_pass_ms": assign_ms,
                           "update_ms_per_iteration": update_ms, "fma_per_pass": n * k * dim,
                           "assign_pass_fp64_TFMA_per_s": n * k * dim / assign_ms / 1e9, "assign_pass_fp64_TFLOPs": 2 * n * k * dim / assign_ms / 1e9,
                           "frac_of_78.6_TF_vendor_sheet": 2 * n * k * dim / assign_ms / 1e9 / 78.6}

    info = acc.device_info()
    res = {"device": {k2: info[k2] for k2 in ("name", "arch", "compute_units") if k2 in info}, "reps": a.reps}
    rows, mem, res["full_20000x384"] = full_call(20_000, 384, a.reps)
    if a.only == "all":
        h = rows.cpu().numpy()
        sec, member, ran = cpu_loop(h, res["full_20000x384"]["k"], 10)
        same = bool(np.array_equal(member, mem.cpu().numpy().view(np.uint32)))
        res["cpu_c_restatement_20000x384"] = {"seconds": sec, "iterations": ran, "flags": "-O2, one core", "same_membership_as_device": same}
        res["device_over_cpu_20000x384"] = {"cpu_s": sec, "device_s": res["full_20000x384"]["ms"] / 1e3, "ratio": sec / (res["full_20000x384"]["ms"] / 1e3)}
        del rows, mem
        _, _, res["full_262144x384"] = full_call(262_144, 384, max(1, a.reps // 2))
        # 1 M x 768: the initialisation and ONE assignment pass (max_iterations = 1)
        n, dim = 1_000_000, 768
        big = torch.empty((n, dim), dtype=torch.float32, device="cuda")
        acc.synth_rows(9, 1 << 40, n, dim, big.data_ptr())
        bm = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        acc.enable_timing(True)
        ms, (k, iters) = timed(lambda: acc.cluster_kmeans_device(big.data_ptr(), n, dim, 0, 1, bm.data_ptr(), None))
        assign_ms, _ = acc.kernel_ms("kmeans_assign"); init_ms, _ = acc.kernel_ms("kmeans_init"); update_ms, _ = acc.kernel_ms("kmeans_update")
        acc.enable_timing(False)
        res["one_pass_1Mx768"] = {"rows": n, "dim": dim, "k": k, "call_ms_first_run": ms, "init_ms": init_ms, "assign_pass_ms": assign_ms, "update_ms": update_ms,
                                  "fma_per_pass": n * k * dim, "assign_pass_fp64_TFLOPs": 2 * n * k * dim / assign_ms / 1e9,
                                  "frac_of_78.6_TF_vendor_sheet": 2 * n * k * dim / assign_ms / 1e9 / 78.6,
                                  "init_row_TB_per_s": (k - 1) * n * dim * 4 / init_ms / 1e9}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if a.only == "all" and res["device_over_cpu_20000x384"]["ratio"] <= 1.0:
        sys.exit("the device call at 20 000 x 384 did not beat the CPU loop on the same machine")


if __name__ == "__main__":
    main()
