"""computePersistenceH0 on the device (yams_quality_persistence_h0_device) — the measurements of DESIGN 3.16.

  shapes     (m, dim) = (232, 1024): the centroid cloud of DESIGN 3.14's 54 000 x 1024 snapshot; (2048, 1024); (8192, 1024): a
             512 MiB matrix.  Rows are Philox rows (yams_synth_rows_device): no stage's work depends on the values (the select
             always runs its 8 passes, the tree its m - 1 steps).  Both chain forms.
  each step  runs in a process of its own under its own time limit (the parent never opens the device, and stops at the first
             step that fails): one warm-up call (workspace allocation, code objects), then --reps calls; the call time is taken
             between HIP events around the call (it synchronises), the per-stage times are the entry's own out_stage_ms (HIP
             events around the pair kernel, the 16 launches of the select, the tree kernel).  Median, minimum and maximum.
  yardsticks (never the code under test)
    (i)   a plain C++ restatement of the contract (CPU_LOOP below: the reference's algorithm, Kruskal over a stable sort),
          -O2 -ffp-contract=off, one core of the same machine, on the same input, at the first two shapes; value, percentile,
          index and merge weights compared on bits
    (ii)  yams_graph_semantic_neighbors_device over the same rows in the same process: its semgraph_pairs_kernel has the same
          128 x 64 tile and ONE fma per element (no subtract, an exact product), and scores all m^2 ordered pairs where the pair
          stage here computes the tiles that touch the upper triangle.  Reported: both times, both pair counts, and the ratio
          per pair; the call also holds a norm pass, a check and the top-K merge, so the ratio flatters the pair stage a little.

    python scripts/persistence_bench.py [--reps 9] [--out profiles/persistence_h0.json] [--no-cpu]

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
STEPS = [(232, 1024), (2048, 1024), (8192, 1024)]
CPU_STEPS = {(232, 1024), (2048, 1024)}
STEP_TIMEOUT = 280
TILE_A, TILE_B = 128, 64


CPU_LOOP = r'''
// The contract of yams_quality_persistence_h0 restated in C++, scalar, in the reference's order (built with -ffp-contract=off).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>
struct Edge { uint32_t i, j; double d; };
extern "C" double persistence_cpu(const float* x, uint64_t m, uint32_t dim, int fused, double* weights, double* out_norm, uint64_t* out_index) {
    std::vector<Edge> edges; std::vector<double> all;
    edges.reserve(m * (m - 1) / 2); all.reserve(m * (m - 1) / 2);
    for (uint64_t i = 0; i < m; ++i)
        for (uint64_t j = i + 1; j < m; ++j) {
            const float* a = x + i * dim; const float* b = x + j * dim;
            double acc = 0.0;
            for (uint32_t k = 0; k < dim; ++k) {
                const double d = double(a[k]) - double(b[k]);
                if (fused) acc = std::fma(d, d, acc); else { const double p = d * d; acc = acc + p; }
            }
            edges.push_back(Edge{uint32_t(i), uint32_t(j), std::sqrt(acc)}); all.push_back(edges.back().d);
        }
    std::stable_sort(edges.begin(), edges.end(), [](const Edge& a, const Edge& b) { return a.d < b.d; });
    const size_t idx = size_t(std::clamp(0.95 * double(all.size() - 1), 0.0, double(all.size() - 1)));
    std::nth_element(all.begin(), all.begin() + idx, all.end());
    const double norm = all[idx];
    *out_norm = norm; *out_index = idx;
    std::vector<size_t> parent(m), rank(m, 0);
    std::iota(parent.begin(), parent.end(), size_t{0});
    auto find = [&](size_t v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; };
    double total = 0.0; uint64_t merges = 0;
    for (const Edge& e : edges) {
        if (merges + 1 >= m) break;
        size_t ra = find(e.i), rb = find(e.j);
        if (ra == rb) continue;
        if (rank[ra] < rank[rb]) std::swap(ra, rb);
        parent[rb] = ra;
        if (rank[ra] == rank[rb]) ++rank[ra];
        weights[merges] = e.d;
        if (merges + 2 < m && norm > 0.0) total += e.d / norm;
        ++merges;
    }
    return norm > 0.0 ? total : 0.0;
}
'''


def cpu_lib(tmp):
    src, lib = os.path.join(tmp, "persistence_cpu.cpp"), os.path.join(tmp, "persistence_cpu.so")
    open(src, "w").write(CPU_LOOP)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src], check=True)
    L = C.CDLL(lib)
    L.persistence_cpu.restype = C.c_double
    L.persistence_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    return L


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def spread(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def computed_pairs(m):
    """Pairs inside the tiles the pair kernel computes (those that touch the upper triangle), padding included."""
    tiles = sum(1 for bx in range((m + TILE_A - 1) // TILE_A) for by in range((m + TILE_B - 1) // TILE_B) if bx * TILE_A <= by * TILE_B + TILE_B - 1)
    return tiles * TILE_A * TILE_B


def run_step(m, dim, reps, with_cpu):
    import torch
    from yams_amd import _lib
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    L, ctx = acc.L, acc.ctx
    rows = torch.empty((m, dim), dtype=torch.float32, device="cuda")
    acc.synth_rows(31, 0, m, dim, rows.data_ptr())
    weights = torch.empty(m, dtype=torch.float64, device="cuda")
    res = {"m": m, "dim": dim, "edges": m * (m - 1) // 2, "matrix_bytes": m * m * 8, "forms": {}}
    outs = {}
    for form, name in ((_lib.RESIDUAL_SEPARATE, "separate"), (_lib.RESIDUAL_FUSED, "fused")):
        out, stage = _lib.PersistenceH0(), np.zeros(3, np.float32)
        call = lambda: acc._check(L.yams_quality_persistence_h0_device(ctx, rows.data_ptr(), m, dim, None, 0, form, C.byref(out), None,
                                                                       weights.data_ptr(), stage.ctypes.data))
        call()      # warm-up
        total, stages = [], []
        for _ in range(reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); e1.synchronize()
            total.append(e0.elapsed_time(e1)); stages.append(stage.copy())
        stages = np.array(stages, np.float64)
        med = np.median(stages, 0)
        res["forms"][name] = {"call_ms": spread(total), "call_ms_all_reps": [float(t) for t in total],
                              "stage_ms": {k: spread(stages[:, i]) for i, k in enumerate(("pairs", "select", "tree"))},
                              "stage_share_of_the_three": {k: float(med[i] / med.sum()) for i, k in enumerate(("pairs", "select", "tree"))},
                              "outside_the_stages_ms": float(np.median(total) - med.sum()),
                              "pair_chain_steps_per_s": computed_pairs(m) * dim / (med[0] * 1e-3),
                              "tree_us_per_step": float(med[2] * 1e3 / max(m - 1, 1)), "value": out.value, "norm": out.norm}
        outs[form] = (out.value, out.norm, out.norm_index, weights[:m - 1].cpu().numpy().copy())
    # (ii) the semantic-neighbour graph's entry over the same rows
    k = 8
    o_r = torch.empty((m, k), dtype=torch.int32, device="cuda"); o_s = torch.empty((m, k), dtype=torch.float32, device="cuda")
    o_c = torch.empty(m, dtype=torch.int32, device="cuda")
    diag = {}
    ycall = lambda: diag.update(acc.semantic_neighbors_device(rows.data_ptr(), m, dim, k, o_r.data_ptr(), o_s.data_ptr(), o_c.data_ptr()))
    ycall()
    ys = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); ycall(); e1.record(); e1.synchronize()
        ys.append(e0.elapsed_time(e1))
    scored = int(diag.get("pairs_scored", m * m))
    res["yardstick_semantic_graph"] = {"call_ms": spread(ys), "pairs_scored": scored, "pairs_computed_here": computed_pairs(m)}
    for name in ("separate", "fused"):
        p = res["forms"][name]["stage_ms"]["pairs"]["median"]
        res["forms"][name]["pairs_over_semgraph_per_pair"] = (p / computed_pairs(m)) / (float(np.median(ys)) / scored)
    # (i) the C++ restatement on one core
    if with_cpu and (m, dim) in CPU_STEPS:
        x = rows.cpu().numpy()
        res["cpu_cpp_restatement"] = {"flags": "-O2 -ffp-contract=off, one core"}
        with tempfile.TemporaryDirectory() as tmp:
            lib = cpu_lib(tmp)
            for form, name in ((_lib.RESIDUAL_SEPARATE, "separate"), (_lib.RESIDUAL_FUSED, "fused")):
                w, nrm, idx = np.zeros(m - 1), C.c_double(), C.c_uint64()
                t0 = time.perf_counter()
                value = lib.persistence_cpu(x.ctypes.data, m, dim, form, w.ctypes.data, C.byref(nrm), C.byref(idx))
                s = time.perf_counter() - t0
                d_value, d_norm, d_index, d_w = outs[form]
                same = bool((bits(d_value) == bits(value)).all() and (bits(d_norm) == bits(nrm.value)).all() and d_index == idx.value and
                            (bits(d_w) == bits(w)).all())
                res["cpu_cpp_restatement"][name] = {"seconds": s, "bits_equal_the_device": same,
                                                    "over_device_call": s / (res["forms"][name]["call_ms"]["median"] / 1e3)}
    info = acc.device_info()
    res["device"] = {k2: info[k2] for k2 in ("name", "arch", "compute_units") if k2 in info}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--step", default=None, help="internal: run one step (m:dim) in this process and print its JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        m, dim = a.step.split(":")
        print("STEP_RESULT " + json.dumps(run_step(int(m), int(dim), a.reps, not a.no_cpu)), flush=True)
        return
    out = {"reps": a.reps, "steps": {},
           "not_measured": ["hardware counters and the HBM share of any stage", "the _host entry and topology_quality_v1 (uploads and the matrix's way back)",
                            "a select list", "dimensions other than 1024", "the reference's own translation unit (it is not on the device's machine)"]}
    for m, dim in STEPS:
        name = "m%d_d%d" % (m, dim)
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "%d:%d" % (m, dim), "--reps", str(a.reps)] + (["--no-cpu"] if a.no_cpu else [])
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
