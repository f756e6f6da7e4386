"""The topology build's input features on the device (yams_features_aggregate / _variance / _compose) — the measurements of
DESIGN 3.17.

  shape      54 000 documents x 1024 dimensions (the reference's own size, topology_sgc.cpp:127-129), 8 chunk records per
             document (432 000 x 1024 record rows), a variance sample of 4096 rows, target 256 kept dimensions, K = 16 entity
             dimensions, sketch_dim 64, sig_len 256, every part on for every row.  Rows are Philox rows
             (yams_synth_rows_device): no kernel's work depends on the values.
  each step  (aggregate, variance, compose) runs in a process of its own under its own time limit (the parent never opens the
             device, and stops at the first step that fails): one warm-up call, then --reps calls of the _device entry timed
             between HIP events around the call (it synchronises), then --reps calls of the _host entry timed with
             perf_counter (uploads and the way back included).  Median, minimum and maximum.
  yardstick  (never the code under test) a plain C++ restatement of the contract (CPU_LOOP below), -O2 -ffp-contract=off, one
             core of the same machine, on the same input; its output is compared with the device's on bits.
  bandwidth  aggregate and compose: the bytes the contract has to move (every record row read once, every output written once;
             compose reads the kept columns' sectors: counted as whole rows) over the median device time, and that as a fraction of
             --hbm-gbs (8000 GB/s, the MI355X's peak).
  variance   a latency chain of 2 m dependent fp64 steps per dimension: reported as nanoseconds per step.

    python scripts/features_bench.py [--reps 9] [--out profiles/features.json] [--no-cpu]

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
N_DOCS, DIM, PER_DOC, SAMPLE, TARGET, K, SKETCH_DIM, SIG_LEN = 54000, 1024, 8, 4096, 256, 16, 64, 256
STEPS = ["aggregate", "variance", "compose"]
STEP_TIMEOUT = 280

CPU_LOOP = r'''
// The contracts of yams_features_aggregate / _variance / _compose restated in C++, scalar (built with -ffp-contract=off).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
extern "C" void aggregate_cpu(const float* rows, uint32_t dim, const uint64_t* off, const uint32_t* rec, uint64_t n_docs, float* out) {
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t lo = off[d], cnt = off[d + 1] - lo;
        float* o = out + d * dim;
        if (!cnt) { std::fill(o, o + dim, 0.0f); continue; }
        std::memcpy(o, rows + uint64_t(rec[lo]) * dim, size_t(dim) * 4);
        for (uint64_t m = 1; m < cnt; ++m) { const float* r = rows + uint64_t(rec[lo + m]) * dim; for (uint32_t i = 0; i < dim; ++i) o[i] += r[i]; }
        if (cnt > 1) for (uint32_t i = 0; i < dim; ++i) o[i] /= float(cnt);
    }
}
extern "C" void variance_cpu(const float* rows, uint32_t dim, uint64_t m, int fused, double* mean, double* var) {
    std::fill(mean, mean + dim, 0.0); std::fill(var, var + dim, 0.0);
    for (uint64_t k = 0; k < m; ++k) for (uint32_t i = 0; i < dim; ++i) mean[i] += double(rows[k * dim + i]);
    for (uint32_t i = 0; i < dim; ++i) mean[i] /= double(m);
    for (uint64_t k = 0; k < m; ++k) for (uint32_t i = 0; i < dim; ++i) {
        const double d = double(rows[k * dim + i]) - mean[i];
        if (fused) var[i] = std::fma(d, d, var[i]); else { const double p = d * d; var[i] = var[i] + p; }
    }
    for (uint32_t i = 0; i < dim; ++i) var[i] /= double(m);
}
static void normalize(float* v, size_t n) {
    double s = 0.0;
    for (size_t i = 0; i < n; ++i) s += double(v[i]) * double(v[i]);
    if (s <= 0.0) return;
    const float norm = float(std::sqrt(s));
    for (size_t i = 0; i < n; ++i) v[i] /= norm;
}
// every part on for every row
extern "C" void compose_cpu(const float* dense, uint64_t n, uint32_t dim, const float* w, const float* ent, uint32_t k, const uint32_t* sig,
                            uint32_t sig_len, uint32_t sd, float ae, float am, float* out, uint32_t stride) {
    std::vector<uint32_t> kept;
    for (uint32_t i = 0; i < dim; ++i) if (w[i] > 0.0f) kept.push_back(i);
    const uint32_t kc = uint32_t(kept.size());
    const float t = (1.0f - ae) - am, ad = (0.0f < t) ? t : 0.0f;
    std::vector<float> sk(sd);
    for (uint64_t r = 0; r < n; ++r) {
        float* o = out + r * stride;
        for (uint32_t j = 0; j < kc; ++j) o[j] = dense[r * dim + kept[j]] * w[kept[j]];
        normalize(o, kc);
        for (uint32_t j = 0; j < kc; ++j) o[j] = o[j] * ad;
        for (uint32_t j = 0; j < k; ++j) o[kc + j] = ent[r * k + j] * ae;
        std::fill(sk.begin(), sk.end(), 0.0f);
        for (uint32_t i = 0; i < sig_len; ++i) sk[sig[r * sig_len + i] % sd] += 1.0f;
        normalize(sk.data(), sd);
        for (uint32_t j = 0; j < sd; ++j) o[kc + k + j] = sk[j] * am;
    }
}
'''


def cpu_lib(tmp):
    src, lib = os.path.join(tmp, "features_cpu.cpp"), os.path.join(tmp, "features_cpu.so")
    open(src, "w").write(CPU_LOOP)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src], check=True)
    L = C.CDLL(lib)
    for f in (L.aggregate_cpu, L.variance_cpu, L.compose_cpu):
        f.restype = None
    vp = C.c_void_p
    L.aggregate_cpu.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint64, vp]
    L.variance_cpu.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_int, vp, vp]
    L.compose_cpu.argtypes = [vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_float, C.c_float, vp, C.c_uint32]
    return L


def spread(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


def timed_device(torch, call, reps):
    call()      # warm-up: workspace, code objects
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def timed_host(call, reps):
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def run_step(step, reps, with_cpu, hbm_gbs):
    import torch
    from yams_amd import _lib
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    L, ctx = acc.L, acc.ctx
    res = {"step": step}
    dev = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")      # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        cpu = cpu_lib(tmp) if with_cpu else None
        if step == "aggregate":
            n_rec = N_DOCS * PER_DOC
            rows = dev((n_rec, DIM), torch.float32)
            acc.synth_rows(31, 0, n_rec, DIM, rows.data_ptr())
            off = np.arange(N_DOCS + 1, dtype=np.uint64) * PER_DOC
            rec = np.random.default_rng(1).permutation(n_rec).astype(np.uint32)      # a document's chunks lie anywhere in the mirror
            d_off, d_rec = torch.from_numpy(off.view(np.int64)).cuda(), torch.from_numpy(rec.view(np.int32)).cuda()
            out, cnt = dev((N_DOCS, DIM), torch.float32), dev((N_DOCS,), torch.int32)
            ts = timed_device(torch, lambda: acc._check(L.yams_features_aggregate_device(
                ctx, rows.data_ptr(), n_rec, DIM, d_off.data_ptr(), d_rec.data_ptr(), N_DOCS, out.data_ptr(), cnt.data_ptr())), reps)
            moved = (n_rec + N_DOCS) * DIM * 4 + n_rec * 4 + N_DOCS * 12
            res.update(shape={"n_docs": N_DOCS, "records": n_rec, "dim": DIM}, device_ms=spread(ts), bytes_moved=moved)
            h_rows = rows.cpu().numpy()
            h_out, h_cnt = np.empty((N_DOCS, DIM), np.float32), np.empty(N_DOCS, np.uint32)
            res["host_entry_ms"] = spread(timed_host(lambda: acc._check(L.yams_features_aggregate_host(
                ctx, h_rows.ctypes.data, n_rec, DIM, off.ctypes.data, rec.ctypes.data, N_DOCS, h_out.ctypes.data, h_cnt.ctypes.data)), reps))
            res["host_entry_equals_device"] = same(h_out, out.cpu().numpy())
            if cpu:
                c_out = np.empty((N_DOCS, DIM), np.float32)
                t0 = time.perf_counter()
                cpu.aggregate_cpu(h_rows.ctypes.data, DIM, off.ctypes.data, rec.ctypes.data, N_DOCS, c_out.ctypes.data)
                res["cpu_cpp_restatement"] = {"seconds": time.perf_counter() - t0, "bits_equal_the_device": same(c_out, h_out)}
        elif step == "variance":
            rows = dev((N_DOCS, DIM), torch.float32)
            acc.synth_rows(32, 0, N_DOCS, DIM, rows.data_ptr())
            sel = np.arange(SAMPLE, dtype=np.uint32)      # the first 4096 documents with an embedding, as :596-606 takes them
            d_sel = torch.from_numpy(sel.view(np.int32)).cuda()
            mv = dev((2, DIM), torch.float64)
            h_rows = rows[:SAMPLE].cpu().numpy()
            res.update(shape={"m": SAMPLE, "dim": DIM}, forms={})
            for form, name in ((_lib.RESIDUAL_SEPARATE, "separate"), (_lib.RESIDUAL_FUSED, "fused")):
                ts = timed_device(torch, lambda: acc._check(L.yams_features_variance_device(
                    ctx, rows.data_ptr(), N_DOCS, DIM, d_sel.data_ptr(), SAMPLE, form, mv[0].data_ptr(), mv[1].data_ptr())), reps)
                got = mv.cpu().numpy()
                h_mean, h_var = np.empty(DIM), np.empty(DIM)
                hs = timed_host(lambda: acc._check(L.yams_features_variance_host(
                    ctx, h_rows.ctypes.data, SAMPLE, DIM, None, 0, form, h_mean.ctypes.data, h_var.ctypes.data)), reps)
                f = {"device_ms": spread(ts), "host_entry_ms": spread(hs), "chain_steps_per_dimension": 2 * SAMPLE,
                     "ns_per_chain_step": float(np.median(ts)) * 1e6 / (2 * SAMPLE), "host_entry_equals_device": same(h_var, got[1])}
                if cpu:
                    c_mean, c_var = np.empty(DIM), np.empty(DIM)
                    t0 = time.perf_counter()
                    cpu.variance_cpu(h_rows.ctypes.data, DIM, SAMPLE, form, c_mean.ctypes.data, c_var.ctypes.data)
                    f["cpu_cpp_restatement"] = {"seconds": time.perf_counter() - t0,
                                                "bits_equal_the_device": same(c_mean, got[0]) and same(c_var, got[1])}
                res["forms"][name] = f
        else:
            rows = dev((N_DOCS, DIM), torch.float32)
            acc.synth_rows(33, 0, N_DOCS, DIM, rows.data_ptr())
            rng = np.random.default_rng(2)
            w = np.zeros(DIM, np.float32)
            w[rng.permutation(DIM)[:TARGET]] = rng.random(TARGET).astype(np.float32) + 0.5
            ent = rng.random((N_DOCS, K)).astype(np.float32)
            sig = rng.integers(0, 1 << 32, (N_DOCS, SIG_LEN), dtype=np.uint64).astype(np.uint32)
            on = np.ones(N_DOCS, np.uint8)
            d_ent, d_sig, d_on = torch.from_numpy(ent).cuda(), torch.from_numpy(sig.view(np.int32)).cuda(), torch.from_numpy(on).cuda()
            stride = TARGET + K + SKETCH_DIM
            out, dims = dev((N_DOCS, stride), torch.float32), dev((N_DOCS,), torch.int32)
            ae, am = C.c_float(0.25), C.c_float(0.1)
            ts = timed_device(torch, lambda: acc._check(L.yams_features_compose_device(
                ctx, rows.data_ptr(), N_DOCS, DIM, w.ctypes.data, d_ent.data_ptr(), K, d_on.data_ptr(), d_sig.data_ptr(), SIG_LEN,
                d_on.data_ptr(), SKETCH_DIM, ae, am, out.data_ptr(), stride, dims.data_ptr())), reps)
            # the dense rows are read twice (the norm pass, the store pass); every kept column's 32-byte sector counts as a row read
            moved = N_DOCS * (2 * DIM * 4 + K * 4 + 2 * SIG_LEN * 4 + stride * 4 + 8 + 12)
            res.update(shape={"n": N_DOCS, "dim": DIM, "kept": TARGET, "k": K, "sketch_dim": SKETCH_DIM, "sig_len": SIG_LEN},
                       device_ms=spread(ts), bytes_moved=moved)
            h_rows = rows.cpu().numpy()
            h_out, h_dims = np.empty((N_DOCS, stride), np.float32), np.empty(N_DOCS, np.uint32)
            res["host_entry_ms"] = spread(timed_host(lambda: acc._check(L.yams_features_compose_host(
                ctx, h_rows.ctypes.data, N_DOCS, DIM, w.ctypes.data, ent.ctypes.data, K, on.ctypes.data, sig.ctypes.data, SIG_LEN, on.ctypes.data,
                SKETCH_DIM, ae, am, h_out.ctypes.data, stride, h_dims.ctypes.data)), reps))
            res["host_entry_equals_device"] = same(h_out, out.cpu().numpy())
            if cpu:
                c_out = np.empty((N_DOCS, stride), np.float32)
                t0 = time.perf_counter()
                cpu.compose_cpu(h_rows.ctypes.data, N_DOCS, DIM, w.ctypes.data, ent.ctypes.data, K, sig.ctypes.data, SIG_LEN, SKETCH_DIM, ae, am,
                                c_out.ctypes.data, stride)
                res["cpu_cpp_restatement"] = {"seconds": time.perf_counter() - t0, "bits_equal_the_device": same(c_out, h_out)}
    if "bytes_moved" in res:
        gbs = res["bytes_moved"] / (res["device_ms"]["median"] * 1e-3) / 1e9
        res["achieved_gb_per_s"] = gbs
        res["fraction_of_hbm_peak"] = gbs / hbm_gbs
    if "cpu_cpp_restatement" in res:
        res["cpu_cpp_restatement"]["over_device_call"] = res["cpu_cpp_restatement"]["seconds"] / (res["device_ms"]["median"] / 1e3)
    for f in res.get("forms", {}).values():
        if "cpu_cpp_restatement" in f:
            f["cpu_cpp_restatement"]["over_device_call"] = f["cpu_cpp_restatement"]["seconds"] / (f["device_ms"]["median"] / 1e3)
    info = acc.device_info()
    res["device"] = {k2: info[k2] for k2 in ("name", "arch", "compute_units") if k2 in info}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        print("STEP_RESULT " + json.dumps(run_step(a.step, a.reps, not a.no_cpu, a.hbm_gbs)), flush=True)
        return
    out = {"reps": a.reps, "hbm_peak_gb_per_s_assumed": a.hbm_gbs, "steps": {},
           "not_measured": ["hardware counters (the HBM traffic is the contract's byte count, not a counter)", "topology_features_v1 through the plugin",
                            "dimensions other than 1024 and documents with other than 8 records", "rows with a part switched off",
                            "the reference's own translation unit (it is not on the device's machine)"]}
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--hbm-gbs", str(a.hbm_gbs)] + (["--no-cpu"] if a.no_cpu else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            out["steps"][step] = {"error": f"time limit of {STEP_TIMEOUT} s"}
            print(step, "hit its time limit: stopping", flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not line:
            out["steps"][step] = {"error": f"exit status {r.returncode}", "tail": (r.stdout + r.stderr)[-600:]}
            print(step, "failed: stopping\n", (r.stdout + r.stderr)[-600:], flush=True)
            break
        out["steps"][step] = json.loads(line[0][len("STEP_RESULT "):])
        print(step, json.dumps(out["steps"][step]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
