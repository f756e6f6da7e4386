"""The cluster artifacts on the device (yams_cluster_centroids / _representatives / _residuals _device) — the measurements of
DESIGN 3.14, at the project's topology shape: 54 000 x 1024 Philox rows and the 232 clusters the device k-means gives them.

  steps      centroids | representatives (n_extra = 3) | residuals_dense_separate | residuals_dense_fused | residuals_lists
             (32-entry lists, SEPARATE) | assign (yams_cluster_assign_device on the same rows and centroids: the nearest
             existing yardstick, the same N*K*D fp64 pairs)
  each step  runs in a process of its own under its own time limit (the parent never opens the device, and stops at the first
             step that fails): the median of --reps calls between HIP events, one warm-up call first; then the plain C
             restatement of the same step, -O2 -ffp-contract=off, one core of the same machine, on the same input, and the two
             outputs compared on bits.

    python scripts/artifacts_bench.py [--reps 5] [--rows 54000] [--dim 1024] [--out profiles/cluster_artifacts.json] [--no-cpu]

No time is fixed in advance and no test gates on one."""
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
STEPS = ["centroids", "representatives", "residuals_dense_separate", "residuals_dense_fused", "residuals_lists", "assign"]
STEP_TIMEOUT = {"centroids": 120, "representatives": 120, "residuals_dense_separate": 300, "residuals_dense_fused": 300, "residuals_lists": 150,
                "assign": 120}

CPU_LOOPS = r'''
/* The three contracts restated in C, scalar, in the reference's order.  FUSED is set by the build: fma() per `+=`, or a rounded
   multiply and a rounded add (the file is built with -ffp-contract=off). */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#ifdef FUSED
#define MADD(acc, a, b) (acc) = __builtin_fma((a), (b), (acc))
#else
#define MADD(acc, a, b) (acc) += (a) * (b)
#endif
void centroids_cpu(const float* x, uint32_t dim, const uint64_t* off, const uint32_t* mem, uint32_t c, float* out) {
    for (uint32_t k = 0; k < c; ++k) {
        float* o = out + (uint64_t)k * dim;
        for (uint32_t d = 0; d < dim; ++d) o[d] = 0.0f;
        const uint64_t cnt = off[k + 1] - off[k];
        for (uint64_t m = off[k]; m < off[k + 1]; ++m) { const float* r = x + (uint64_t)mem[m] * dim; for (uint32_t d = 0; d < dim; ++d) o[d] += r[d]; }
        if (cnt) for (uint32_t d = 0; d < dim; ++d) o[d] /= (float)cnt;
    }
}
static double cosine_distance(const float* a, const float* b, uint32_t dim) {
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (uint32_t i = 0; i < dim; ++i) { dot += (double)a[i] * (double)b[i]; na += (double)a[i] * (double)a[i]; nb += (double)b[i] * (double)b[i]; }
    if (na <= 0.0 || nb <= 0.0) return 2.0;
    double c = dot / (sqrt(na) * sqrt(nb));
    c = c < -1.0 ? -1.0 : (1.0 < c ? 1.0 : c);
    return 1.0 - c;
}
void representatives_cpu(const float* x, uint32_t dim, const uint64_t* off, const uint32_t* cand, const float* cents, uint32_t c,
                         uint32_t n_extra, uint32_t* sel) {
    for (uint32_t k = 0; k < c; ++k) {
        const uint64_t m = off[k + 1] - off[k];
        const uint32_t* list = cand + off[k];
        const uint64_t limit = m < n_extra ? m : n_extra;
        unsigned char* used = calloc(m ? m : 1, 1);
        double* md = malloc((m ? m : 1) * sizeof(double));
        for (uint64_t i = 0; i < m; ++i) md[i] = DBL_MAX;
        for (uint32_t s = 0; s < n_extra; ++s) sel[(uint64_t)k * n_extra + s] = 0xffffffffu;
        uint64_t last = 0;
        for (uint64_t s = 0; s < limit; ++s) {
            const float* target = s == 0 ? cents + (uint64_t)k * dim : x + (uint64_t)list[last] * dim;
            uint64_t best = m; double best_d = -1.0;
            for (uint64_t i = 0; i < m; ++i) {
                if (used[i]) continue;
                const double d = cosine_distance(x + (uint64_t)list[i] * dim, target, dim);
                md[i] = d < md[i] ? d : md[i];
                if (md[i] > best_d) { best_d = md[i]; best = i; }
            }
            if (best == m) break;
            used[best] = 1; last = best; sel[(uint64_t)k * n_extra + s] = (uint32_t)best;
        }
        free(used); free(md);
    }
}
/* pairs of documents [lo, hi): dense (off == NULL: every cluster) or listed */
void residuals_cpu(const float* x, uint64_t lo, uint64_t hi, uint32_t dim, const float* cents, uint32_t c, const uint32_t* primary,
                   const uint64_t* off, const uint32_t* cand, double* pn, double* cn, double* rd) {
    double* pr = malloc(dim * sizeof(double));
    for (uint64_t u = lo; u < hi; ++u) {
        const float* e = x + u * dim; const float* pc = cents + (uint64_t)primary[u] * dim;
        double s = 0.0;
        for (uint32_t d = 0; d < dim; ++d) { pr[d] = (double)e[d] - pc[d]; MADD(s, pr[d], pr[d]); }
        pn[u] = s;
        const uint64_t b = off ? off[u] : u * c, m = off ? off[u + 1] - off[u] : c;
        for (uint64_t j = 0; j < m; ++j) {
            const float* cc = cents + (uint64_t)(off ? cand[b + j] : j) * dim;
            double a = 0.0, q = 0.0;
            for (uint32_t d = 0; d < dim; ++d) { const double r = (double)e[d] - cc[d]; MADD(a, r, r); MADD(q, pr[d], r); }
            cn[b + j] = a; rd[b + j] = q;
        }
    }
    free(pr);
}
'''


def cpu_lib(tmp, fused, hardware_fma=True):
    src = os.path.join(tmp, "artifacts_cpu.c")
    lib = os.path.join(tmp, "artifacts_cpu_fused.so" if fused else "artifacts_cpu.so")
    open(src, "w").write(CPU_LOOPS)
    flags = ["-O2", "-ffp-contract=off"] + ((["-DFUSED"] + (["-mfma"] if hardware_fma else [])) if fused else [])
    subprocess.run([os.environ.get("CC", "cc"), *flags, "-shared", "-fPIC", "-o", lib, src, "-lm"], check=True)
    L = C.CDLL(lib)
    vp = C.c_void_p
    L.centroids_cpu.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.representatives_cpu.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, vp]
    L.residuals_cpu.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
    return L, " ".join(flags) + ", one core"


def host_has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return False


def timed(call, reps):
    import torch
    call()      # warm-up: workspace allocation, code objects
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), ts


def run_step(step, n, dim, reps, with_cpu):
    import torch
    from yams_amd import _lib
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    L, ctx = acc.L, acc.ctx
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rows = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    acc.synth_rows(13, 0, n, dim, rows.data_ptr())
    # the clusters of the device k-means (k = round(sqrt(n))), each member list in a scrambled order (as a sort by hash leaves it)
    mem_d = torch.empty(n, dtype=torch.int32, device="cuda")
    k_out, it_out = C.c_uint32(0), C.c_uint32(0)
    acc._check(L.yams_cluster_kmeans_device(ctx, rows.data_ptr(), n, dim, 0, 10, mem_d.data_ptr(), None, C.byref(k_out), C.byref(it_out)))
    c = k_out.value
    membership = mem_d.cpu().numpy().astype(np.int64)
    rng = np.random.default_rng(5)
    perm = rng.permutation(n)
    members = perm[np.argsort(membership[perm], kind="stable")].astype(np.uint32)
    off = np.zeros(c + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(membership, minlength=c))
    d_off, d_mem, d_pri = dev(off.view(np.int64)), dev(members.view(np.int32)), dev(membership.astype(np.uint32).view(np.int32))
    cents = torch.empty((c, dim), dtype=torch.float32, device="cuda")
    counts = torch.empty(c, dtype=torch.int32, device="cuda")
    centroids = lambda: acc._check(L.yams_cluster_centroids_device(ctx, rows.data_ptr(), n, dim, d_off.data_ptr(), d_mem.data_ptr(), c,
                                                                    cents.data_ptr(), counts.data_ptr()))
    centroids()
    res = {"clusters": c, "kmeans_iterations": it_out.value, "largest_cluster": int(np.diff(off.astype(np.int64)).max())}
    h_rows = rows.cpu().numpy() if with_cpu else None
    h_cents = cents.cpu().numpy()
    same, cpu_s, cpu_note = "not_run", "not_run", None
    with tempfile.TemporaryDirectory() as tmp:
        if step == "centroids":
            ms, all_ms = timed(centroids, reps)
            if with_cpu:
                lib, cpu_note = cpu_lib(tmp, False)
                want = np.empty_like(h_cents)
                t0 = time.perf_counter(); lib.centroids_cpu(h_rows.ctypes.data, dim, off.ctypes.data, members.ctypes.data, c, want.ctypes.data)
                cpu_s = time.perf_counter() - t0
                same = bool(np.array_equal(want.view(np.uint32), h_cents.view(np.uint32)))
        elif step == "representatives":
            n_extra = 3
            sel = torch.empty((c, n_extra), dtype=torch.int32, device="cuda")
            call = lambda: acc._check(L.yams_cluster_representatives_device(ctx, rows.data_ptr(), n, dim, d_off.data_ptr(), d_mem.data_ptr(),
                                                                             cents.data_ptr(), None, c, n_extra, sel.data_ptr(), counts.data_ptr()))
            ms, all_ms = timed(call, reps)
            if with_cpu:
                lib, cpu_note = cpu_lib(tmp, False)
                want = np.empty((c, n_extra), np.uint32)
                t0 = time.perf_counter()
                lib.representatives_cpu(h_rows.ctypes.data, dim, off.ctypes.data, members.ctypes.data, h_cents.ctypes.data, c, n_extra, want.ctypes.data)
                cpu_s = time.perf_counter() - t0
                same = bool(np.array_equal(want, sel.cpu().numpy().view(np.uint32)))
        elif step == "assign":
            asg = torch.empty(n, dtype=torch.int32, device="cuda")
            dist = torch.empty(n, dtype=torch.float64, device="cuda")
            call = lambda: acc._check(L.yams_cluster_assign_device(ctx, rows.data_ptr(), n, dim, cents.data_ptr(), c, None, asg.data_ptr(), dist.data_ptr()))
            ms, all_ms = timed(call, reps)
        else:
            fused = step == "residuals_dense_fused"
            lists = step == "residuals_lists"
            if lists:
                per = 32
                cand = rng.integers(0, c, n * per).astype(np.uint32)
                coff = (np.arange(n + 1, dtype=np.uint64) * per)
                d_coff, d_cand = dev(coff.view(np.int64)), dev(cand.view(np.int32))
                pairs = n * per
            else:
                pairs = n * c
            pn = torch.empty(n, dtype=torch.float64, device="cuda")
            cn = torch.empty(pairs, dtype=torch.float64, device="cuda")
            rd = torch.empty(pairs, dtype=torch.float64, device="cuda")
            form = _lib.RESIDUAL_FUSED if fused else _lib.RESIDUAL_SEPARATE
            call = lambda: acc._check(L.yams_cluster_residuals_device(ctx, rows.data_ptr(), n, dim, cents.data_ptr(), c, d_pri.data_ptr(),
                                                                       d_coff.data_ptr() if lists else None, d_cand.data_ptr() if lists else None, form,
                                                                       pn.data_ptr(), cn.data_ptr(), rd.data_ptr()))
            ms, all_ms = timed(call, reps)
            res["pairs"] = pairs
            if with_cpu:
                # the fused loop needs the host's fma instruction to run at the speed of a compiled host; without one only a
                # tenth of the documents is computed (and compared), and the time is scaled
                slow = fused and not host_has_fma()
                docs = n // 10 if slow else n
                lib, cpu_note = cpu_lib(tmp, fused, hardware_fma=not slow)
                if slow:
                    cpu_note += "; no fma instruction on this host: the C library's fma(), a tenth of the documents, time scaled by 10"
                pri = membership.astype(np.uint32)
                w_pn, w_cn, w_rd = np.empty(n), np.empty(pairs), np.empty(pairs)
                t0 = time.perf_counter()
                lib.residuals_cpu(h_rows.ctypes.data, 0, docs, dim, h_cents.ctypes.data, c, pri.ctypes.data, coff.ctypes.data if lists else None,
                                  cand.ctypes.data if lists else None, w_pn.ctypes.data, w_cn.ctypes.data, w_rd.ctypes.data)
                cpu_s = (time.perf_counter() - t0) * (n / docs)
                m = docs * (per if lists else c)
                eq = lambda a, b: bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
                same = eq(w_pn[:docs], pn.cpu().numpy()[:docs]) and eq(w_cn[:m], cn.cpu().numpy()[:m]) and eq(w_rd[:m], rd.cpu().numpy()[:m])
    res.update({"ms": ms, "ms_all_reps": all_ms, "cpu_c_restatement": {"seconds": cpu_s, "flags": cpu_note, "bits_equal_the_device": same},
                "cpu_over_device": (cpu_s / (ms / 1e3)) if isinstance(cpu_s, float) else "not_run"})
    info = acc.device_info()
    res["device"] = {k2: info[k2] for k2 in ("name", "arch", "compute_units") if k2 in info}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=54_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        print("STEP_RESULT " + json.dumps(run_step(a.step, a.rows, a.dim, a.reps, not a.no_cpu)), flush=True)
        return
    out = {"shape": {"rows": a.rows, "dim": a.dim}, "reps": a.reps, "steps": {},
           "not_measured": ["hardware counters", "the HBM share against the Infinity Cache (the 221 MB matrix fits the cache)"]}
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rows", str(a.rows), "--dim", str(a.dim), "--reps", str(a.reps)]
        if a.no_cpu:
            cmd.append("--no-cpu")
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT[step])
        except subprocess.TimeoutExpired:
            out["steps"][step] = {"error": f"time limit of {STEP_TIMEOUT[step]} s"}
            print(step, "hit its time limit: stopping", flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not line:
            out["steps"][step] = {"error": f"exit status {r.returncode}", "tail": (r.stdout + r.stderr)[-600:]}
            print(step, "failed: stopping\n", (r.stdout + r.stderr)[-600:], flush=True)
            break
        out["steps"][step] = json.loads(line[0][len("STEP_RESULT "):])
        print(step, json.dumps(out["steps"][step]), flush=True)
    s = out["steps"]
    if "assign" in s and "ms" in s["assign"]:
        out["ratio_to_assign"] = {k: v["ms"] / s["assign"]["ms"] for k, v in s.items() if k != "assign" and "ms" in v}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
