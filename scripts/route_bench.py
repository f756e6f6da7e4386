"""The cluster router's dense signal on the device (yams_route_dense_device over a resident index) — the measurements of
DESIGN 3.15.

  shapes     snapshot: 232 clusters x (centroid + 3 representatives) = 928 rows of dim 1024 (the cluster count DESIGN 3.14's
             54 000 x 1024 snapshot gives), at 1, 8 and 256 queries; large: 16 384 clusters x 4 = 65 536 rows of dim 1024, at 1
             and 1024 queries.  Rows and queries are Philox rows (yams_synth_rows_device): no time here depends on values.
  each step  runs in a process of its own under its own time limit (the parent never opens the device, and stops at the first
             step that fails): the median of --reps calls between HIP events, one warm-up call first.
  yardsticks (never the code under test)
    (i)   a plain C loop of the contract, -O2 -ffp-contract=off, one core of the same machine, on the same input, outputs
          compared on bits (at 256 and 1024 queries the loop runs the first 8 queries and its time is scaled)
    (ii)  more than 8 queries: yams_cluster_assign_device on the same Q x V x dim in the same process (rows = the table,
          centroids = the queries: the same fp64 tile with one fma per pair); the bar is 1.10 x that time
    (iii) one query: yams_scan_entity_topk_device over the same rows (the same row-chain core plus a selection), a ratio, no bar

    python scripts/route_bench.py [--reps 9] [--out profiles/cluster_route.json] [--no-cpu]

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
SHAPES = {"snapshot": (232, 3), "large": (16384, 3)}
STEPS = [("snapshot", 1), ("snapshot", 8), ("snapshot", 256), ("large", 1), ("large", 1024)]
STEP_TIMEOUT = 240
CPU_QUERIES = 8

CPU_LOOP = r'''
/* The contract of yams_route_dense restated in C, scalar, in the reference's order (built with -ffp-contract=off). */
#include <math.h>
#include <stdint.h>
static float norm(const float* v, uint32_t dim) {
    double acc = 0.0;
    for (uint32_t i = 0; i < dim; ++i) acc += (double)v[i] * (double)v[i];
    return (float)sqrt(acc);
}
void norms_cpu(const float* x, uint64_t n, uint32_t dim, float* out) { for (uint64_t r = 0; r < n; ++r) out[r] = norm(x + r * dim, dim); }
void route_cpu(const float* vec, const float* vnorm, const uint32_t* off, const uint8_t* has, const uint16_t* pos, uint32_t c, uint32_t dim,
               const float* queries, uint32_t nq, uint32_t rep_limit, float* dense, uint8_t* observed, uint32_t* evals) {
    for (uint32_t q = 0; q < nq; ++q) {
        const float* x = queries + (uint64_t)q * dim;
        const float qn = norm(x, dim);
        evals[q] = 0;
        for (uint32_t k = 0; k < c; ++k) {
            float cur = 0.0f; uint8_t obs = 0;
            for (uint32_t r = off[k]; r < off[k + 1]; ++r) {
                const int centroid = has[k] && r == off[k];
                const float vn = vnorm[r];
                if (centroid) { if (!(qn > 0.0f && vn > 0.0f)) continue; }
                else if ((rep_limit && pos[r] >= rep_limit - 1) || qn <= 0.0f || vn <= 0.0f) continue;
                const float* v = vec + (uint64_t)r * dim;
                double acc = 0.0;
                for (uint32_t i = 0; i < dim; ++i) acc += (double)x[i] * (double)v[i];
                const float cosine = (float)acc / (qn * vn);
                float d = (cosine + 1.0f) * 0.5f;
                d = d < 0.0f ? 0.0f : (1.0f < d ? 1.0f : d);
                cur = centroid ? d : (cur < d ? d : cur);
                obs = 1; ++evals[q];
            }
            dense[(uint64_t)q * c + k] = cur; observed[(uint64_t)q * c + k] = obs;
        }
    }
}
'''


def cpu_lib(tmp):
    src, lib = os.path.join(tmp, "route_cpu.c"), os.path.join(tmp, "route_cpu.so")
    open(src, "w").write(CPU_LOOP)
    subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src, "-lm"], check=True)
    L = C.CDLL(lib)
    vp = C.c_void_p
    L.norms_cpu.argtypes = [vp, C.c_uint64, C.c_uint32, vp]
    L.route_cpu.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    return L


def timed(call, reps):
    import torch
    call()      # warm-up: workspace allocation, code objects
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), ts


def run_step(shape, nq, dim, reps, with_cpu):
    import torch
    from yams_amd import _lib
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    L, ctx = acc.L, acc.ctx
    c, r = SHAPES[shape]
    v = c * (1 + r)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    table = torch.empty((v, dim), dtype=torch.float32, device="cuda")
    queries = torch.empty((nq, dim), dtype=torch.float32, device="cuda")
    acc.synth_rows(21, 0, v, dim, table.data_ptr())
    acc.synth_rows(22, 0, nq, dim, queries.data_ptr())
    off = (np.arange(c + 1, dtype=np.uint32) * (1 + r))
    has = np.ones(c, np.uint8)
    pos = np.tile(np.concatenate([[0], np.arange(r)]).astype(np.uint16), c)
    d_off, d_has, d_pos = dev(off.view(np.int32)), dev(has), dev(pos.view(np.int16))
    norms = torch.empty(v, dtype=torch.float32, device="cuda")
    index = C.c_void_p()
    t0 = time.perf_counter()
    acc._check(L.yams_route_index_create_device(ctx, table.data_ptr(), v, dim, d_off.data_ptr(), d_has.data_ptr(), d_pos.data_ptr(), c,
                                                C.byref(index), norms.data_ptr()))
    create_s = time.perf_counter() - t0
    dense = torch.empty((nq, c), dtype=torch.float32, device="cuda")
    obs = torch.empty((nq, c), dtype=torch.uint8, device="cuda")
    evals = torch.empty(nq, dtype=torch.int32, device="cuda")
    diag = _lib.RouteDiag()
    call = lambda: acc._check(L.yams_route_dense_device(index, queries.data_ptr(), nq, 0, None, dense.data_ptr(), obs.data_ptr(), evals.data_ptr(),
                                                        C.byref(diag)))
    ms, all_ms = timed(call, reps)
    res = {"clusters": c, "rows": v, "dim": dim, "queries": nq, "ms": ms, "ms_all_reps": all_ms, "form": "rows" if diag.form == 0 else "tile",
           "slices": diag.slices, "index_create_s_first_call": create_s, "pair_gfma_per_s": nq * v * dim / (ms * 1e-3) / 1e9}
    # (ii) / (iii): the yardstick of this form, in the same process
    if nq > 8:
        asg = torch.empty(v, dtype=torch.int32, device="cuda")
        dist = torch.empty(v, dtype=torch.float64, device="cuda")
        ycall = lambda: acc._check(L.yams_cluster_assign_device(ctx, table.data_ptr(), v, dim, queries.data_ptr(), nq, None, asg.data_ptr(), dist.data_ptr()))
        yms, yall = timed(ycall, reps)
        res["yardstick_assign"] = {"ms": yms, "ms_all_reps": yall, "ratio": ms / yms, "bar": 1.10, "within_bar": bool(ms <= 1.10 * yms)}
    elif nq == 1:
        corpus = acc.corpus_view(table.data_ptr(), v, dim)
        ents = acc.entities_view()
        k = 8
        s = torch.empty(k, dtype=torch.float32, device="cuda"); rws = torch.empty(k, dtype=torch.int64, device="cuda")
        n_ = torch.empty(1, dtype=torch.int32, device="cuda"); m_ = torch.empty(1, dtype=torch.int64, device="cuda")
        sd = _lib.ScanDiag()
        ycall = lambda: acc._check(L.yams_scan_entity_topk_device(ctx, C.byref(corpus), C.byref(ents), queries.data_ptr(), None, 1, k, C.c_float(-2.0),
                                                                  s.data_ptr(), rws.data_ptr(), n_.data_ptr(), m_.data_ptr(), C.byref(sd)))
        yms, yall = timed(ycall, reps)
        res["yardstick_entity_topk"] = {"ms": yms, "ms_all_reps": yall, "ratio": ms / yms}
    # (i): the C loop, one core
    if with_cpu:
        with tempfile.TemporaryDirectory() as tmp:
            lib = cpu_lib(tmp)
            h_table, h_q = table.cpu().numpy(), queries.cpu().numpy()
            m = min(nq, CPU_QUERIES)
            h_norm = np.empty(v, np.float32)
            lib.norms_cpu(h_table.ctypes.data, v, dim, h_norm.ctypes.data)
            w_d, w_o, w_e = np.empty((m, c), np.float32), np.empty((m, c), np.uint8), np.empty(m, np.uint32)
            t0 = time.perf_counter()
            lib.route_cpu(h_table.ctypes.data, h_norm.ctypes.data, off.ctypes.data, has.ctypes.data, pos.ctypes.data, c, dim, h_q.ctypes.data, m, 0,
                          w_d.ctypes.data, w_o.ctypes.data, w_e.ctypes.data)
            cpu_s = (time.perf_counter() - t0) * (nq / m)
            same = bool(np.array_equal(h_norm.view(np.uint32), norms.cpu().numpy().view(np.uint32)) and
                        np.array_equal(w_d.view(np.uint32), dense.cpu().numpy()[:m].view(np.uint32)) and
                        np.array_equal(w_o, obs.cpu().numpy()[:m]) and np.array_equal(w_e, evals.cpu().numpy()[:m].view(np.uint32)))
            res["cpu_c_restatement"] = {"seconds": cpu_s, "flags": "-O2 -ffp-contract=off, one core", "queries_run": m,
                                        "scaled": m != nq, "bits_equal_the_device": same}
            res["cpu_over_device"] = cpu_s / (ms / 1e3)
    L.yams_route_index_destroy(index)
    info = acc.device_info()
    res["device"] = {k2: info[k2] for k2 in ("name", "arch", "compute_units") if k2 in info}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--step", default=None, help="internal: run one step (shape:queries) in this process and print its JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        shape, nq = a.step.split(":")
        print("STEP_RESULT " + json.dumps(run_step(shape, int(nq), a.dim, a.reps, not a.no_cpu)), flush=True)
        return
    out = {"reps": a.reps, "steps": {},
           "not_measured": ["hardware counters", "candidate masks and representative limits (every row is scored here)", "the _host entries and topology_route_v1",
                            "dimensions other than %d" % a.dim, "query counts between 9 and 255 (where the tile's 64-query side is partly idle)"]}
    for shape, nq in STEPS:
        name = "%s_q%d" % (shape, nq)
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%d" % (shape, nq), "--dim", str(a.dim), "--reps", str(a.reps)]
        if a.no_cpu:
            cmd.append("--no-cpu")
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            out["steps"][name] = {"error": f"time limit of {STEP_TIMEOUT} s"}
            print(name, "hit its time limit: stopping", flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not line:
            out["steps"][name] = {"error": f"exit status {r.returncode}", "tail": (r.stdout + r.stderr)[-600:]}
            print(name, "failed: stopping\n", (r.stdout + r.stderr)[-600:], flush=True)
            break
        out["steps"][name] = json.loads(line[0][len("STEP_RESULT "):])
        print(name, json.dumps(out["steps"][name]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
