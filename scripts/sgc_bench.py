"""SGC smoothing on the device (yams_graph_sgc_smooth_device) — the measurements of DESIGN 3.13:

  1. the full call at 54 000 x 1024, lists from an 8-neighbour graph (every row names 8 others, symmetrised: about 16 edges a
     row), 2 hops: time per call and per hop (the context's own event brackets around the hop launches)
  2. GB/s of the hops against the algorithmic bytes (nnz + 2n) * dim * 4 + nnz * 8 per hop (every neighbour row read once per
     edge, the row itself read and written, a column and a weight per edge)
  3. the CPU side: a plain C restatement of the loop, -O2, one core of the same machine, on the same input

    python scripts/sgc_bench.py [--reps 3] [--out profiles/sgc.json] [--rows 54000] [--dim 1024] [--no-cpu]
    python scripts/sgc_bench.py --not-run --out profiles/sgc.json

HIP events around calls that end in a synchronise, one warm-up call first, each figure the median of --reps calls.  No time
is fixed in advance and no test gates on one.  --not-run writes the file with every figure "not_run" (what is committed until
the script has run on a device)."""
from __future__ import annotations

import argparse
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

CPU_LOOP = r'''
/* The hop loop restated in C: per row the self term, then the row's edges in list order; fp64 products, fp32 adds. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
int sgc_cpu(const float* x, uint64_t n, uint32_t dim, const uint64_t* off, const uint32_t* cols, const float* w, uint32_t hops, float* out) {
    double* inv = malloc(n * sizeof(double));
    float* a = malloc(n * dim * sizeof(float)); float* b = malloc(n * dim * sizeof(float));
    if (!inv || !a || !b) return 1;
    memcpy(a, x, n * dim * sizeof(float));
    for (uint64_t i = 0; i < n; ++i) {
        double deg = 1.0;
        for (uint64_t e = off[i]; e < off[i + 1]; ++e) deg += (double)w[e];
        inv[i] = deg > 0.0 ? 1.0 / sqrt(deg) : 0.0;
    }
    for (uint32_t h = 0; h < hops; ++h) {
        for (uint64_t i = 0; i < n; ++i) {
            float* row = b + i * dim; const float* self = a + i * dim;
            const double ss = inv[i] * inv[i];
            for (uint32_t d = 0; d < dim; ++d) row[d] = (float)(ss * (double)self[d]);
            for (uint64_t e = off[i]; e < off[i + 1]; ++e) {
                const double s = (double)w[e] * inv[i] * inv[cols[e]];
                if (s == 0.0) continue;
                const float* src = a + (uint64_t)cols[e] * dim;
                for (uint32_t d = 0; d < dim; ++d) row[d] += (float)(s * (double)src[d]);
            }
        }
        float* t = a; a = b; b = t;
    }
    memcpy(out, a, n * dim * sizeof(float));
    free(inv); free(a); free(b);
    return 0;
}
'''
FIGURES = ["ms_per_call", "ms_all_reps", "check_ms", "scale_ms", "hops_ms", "ms_per_hop", "algorithmic_bytes_per_hop", "hop_GB_per_s", "diag",
           "cpu_c_restatement", "device_over_cpu"]


def cpu_loop(x, off, cols, w, hops):
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "sgc_cpu.c"); lib = os.path.join(tmp, "sgc_cpu.so")
        open(src, "w").write(CPU_LOOP)
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src, "-lm"], check=True)
        L = C.CDLL(lib)
        L.sgc_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        out = np.empty_like(x)
        t0 = time.perf_counter()
        rc = L.sgc_cpu(x.ctypes.data, x.shape[0], x.shape[1], off.ctypes.data, cols.ctypes.data, w.ctypes.data, hops, out.ctypes.data)
        assert rc == 0
        return time.perf_counter() - t0, out


def neighbour_lists(n, k, seed):
    """Every row names k other rows with a weight in (0, 1]; symmetrised with the larger weight.  Each row's list is then
    shuffled: the order a hash map would leave is no sorted one."""
    rng = np.random.default_rng(seed)
    a = np.repeat(np.arange(n, dtype=np.int64), k)
    b = (a + rng.integers(1, n, n * k)) % n
    wt = (1.0 - rng.random(n * k)).astype(np.float32)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = hi * n + lo
    order = np.lexsort((-wt, key))
    key, wt = key[order], wt[order]
    first = np.concatenate(([True], key[1:] != key[:-1]))
    key, wt = key[first], wt[first]
    lo, hi = key % n, key // n
    rows = np.concatenate((lo, hi)); cols = np.concatenate((hi, lo)); ws = np.concatenate((wt, wt))
    perm = rng.permutation(len(rows))
    rows, cols, ws = rows[perm], cols[perm], ws[perm]
    order = np.argsort(rows, kind="stable")
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return off, cols[order].astype(np.uint32), ws[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=54_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--neighbours", type=int, default=8)
    ap.add_argument("--hops", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--not-run", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, dim, hops = a.rows, a.dim, a.hops
    shape = {"rows": n, "dim": dim, "neighbours_named_per_row": a.neighbours, "hops": hops}
    if a.not_run:
        res = {"device": "not_run", "reps": "not_run", "shape": shape, **{f: "not_run" for f in FIGURES}}
    else:
        import torch
        from yams_amd.accel import Accel
        acc = Accel(0, torch.cuda.current_stream().cuda_stream)
        off, cols, w = neighbour_lists(n, a.neighbours, 7)
        nnz = int(off[n])
        rows = torch.empty((n, dim), dtype=torch.float32, device="cuda")
        acc.synth_rows(13, 0, n, dim, rows.data_ptr())
        out = torch.empty((n, dim), dtype=torch.float32, device="cuda")
        d_off = torch.from_numpy(off.view(np.int64)).cuda(); d_cols = torch.from_numpy(cols.view(np.int32)).cuda(); d_w = torch.from_numpy(w).cuda()
        torch.cuda.synchronize()
        call = lambda: acc.sgc_smooth_device(rows.data_ptr(), n, dim, d_off.data_ptr(), d_cols.data_ptr(), d_w.data_ptr(), hops, out.data_ptr())
        call()                                                  # warm-up: workspace allocation, code objects
        acc.enable_timing(True)
        ts = []
        for _ in range(a.reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); diag = call(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        check_ms, _ = acc.kernel_ms("sgc_check"); scale_ms, _ = acc.kernel_ms("sgc_scale"); hops_ms, _ = acc.kernel_ms("sgc_hops")
        acc.enable_timing(False)
        per_hop = hops_ms / hops
        bytes_per_hop = (nnz + 2 * n) * dim * 4 + nnz * 8
        info = acc.device_info()
        res = {"device": {k2: info[k2] for k2 in ("name", "arch", "compute_units") if k2 in info}, "reps": a.reps, "shape": {**shape, "nnz": nnz},
               "ms_per_call": float(np.median(ts)), "ms_all_reps": ts, "check_ms": check_ms, "scale_ms": scale_ms, "hops_ms": hops_ms,
               "ms_per_hop": per_hop, "algorithmic_bytes_per_hop": bytes_per_hop, "hop_GB_per_s": bytes_per_hop / per_hop / 1e6, "diag": diag,
               "cpu_c_restatement": "not_run", "device_over_cpu": "not_run"}
        if not a.no_cpu:
            h = rows.cpu().numpy()
            sec, want = cpu_loop(h, off, cols, w, hops)
            same = bool(np.array_equal(want.view(np.uint32), out.cpu().numpy().view(np.uint32)))
            res["cpu_c_restatement"] = {"seconds": sec, "seconds_per_hop": sec / hops, "flags": "-O2 -ffp-contract=off, one core", "bits_equal_the_device": same}
            res["device_over_cpu"] = {"cpu_s": sec, "device_s": res["ms_per_call"] / 1e3, "ratio": sec / (res["ms_per_call"] / 1e3)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
