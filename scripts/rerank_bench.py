"""The late-interaction rerank on the device (yams_rerank_maxsim) — the measurements of DESIGN 3.18.

  shapes     the reference's padded shape: documents of 512 tokens (encode() pads to maxSequenceLength_) at token_dim 48, a
             window of 100 and of 300 documents, against a 512-token query (the reference pads the query alike) and against a
             32-token query; and the same at dim 128, 100 documents.  Values are mixed-exponent floats: no kernel's work depends
             on them.
  each shape runs in a process of its own under its own time limit (the parent never opens the device, and stops at the first
             shape that fails): per form two warm-up calls, then --reps (>= 20) calls of the _device entry timed between HIP
             events around the call (it synchronises; the offsets' check and the score launch are inside), then --reps calls of
             the _host entry timed with perf_counter (uploads and the way back included).  Median, minimum and maximum.
  yardstick  (never the code under test) a plain C++ restatement of the contract (CPU_LOOP below), -O2 -ffp-contract=off, ONE
             core of the same machine, on the same input, in each form; its scores are compared with the device's on bits.
  rate       chain steps (n_docs x tokens x query tokens x dim) per second of the median device call, and two FLOP per step
             against the fp32 vector / matrix peak (157.3 TF); which path served the fused form (the diag).

    python scripts/rerank_bench.py [--reps 20] [--out profiles/rerank_maxsim.json] [--no-cpu]

No time is fixed in advance and no test gates on one: the parent commit has no device path, the comparison is one host core."""
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
TOKENS = 512
SHAPES = [(48, 100, 512), (48, 300, 512), (48, 100, 32), (48, 300, 32), (128, 100, 512), (128, 100, 32)]      # dim, documents, query tokens
PEAK_TF = 157.3
SHAPE_TIMEOUT = 280


CPU_LOOP = r'''
// The contract of yams_rerank_maxsim restated in C++, scalar (built with -ffp-contract=off: form 0 multiplies, then adds).
#include <cmath>
#include <cstdint>
#include <limits>
extern "C" void maxsim_cpu(const float* query, uint32_t tq, uint32_t dim, const float* rows, const uint64_t* off, uint64_t n_docs, int fused,
                           float* scores) {
    for (uint64_t d = 0; d < n_docs; ++d) {
        float score = 0.0f;
        for (uint32_t q = 0; q < tq; ++q) {
            const float* a = query + uint64_t(q) * dim;
            float best = -std::numeric_limits<float>::infinity();
            for (uint64_t r = off[d]; r < off[d + 1]; ++r) {
                const float* b = rows + r * dim;
                float sum = 0.0f;
                if (fused) for (uint32_t i = 0; i < dim; ++i) sum = std::fmaf(a[i], b[i], sum);
                else for (uint32_t i = 0; i < dim; ++i) { const float p = a[i] * b[i]; sum = sum + p; }
                if (sum > best) best = sum;
            }
            score = score + best;
        }
        scores[d] = score;
    }
}
'''


def cpu_lib(tmp):
    src, lib = os.path.join(tmp, "rerank_cpu.cpp"), os.path.join(tmp, "rerank_cpu.so")
    open(src, "w").write(CPU_LOOP)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src], check=True)
    L = C.CDLL(lib)
    L.maxsim_cpu.restype = None
    L.maxsim_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    return L


def mixed(rng, shape, lo, hi):
    """Floats of mixed exponents 2^lo .. 2^hi and both signs, full mantissas."""
    return (rng.uniform(1.0, 2.0, shape) * np.exp2(rng.integers(lo, hi + 1, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def same(a, b):
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def spread(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def run_shape(dim, n_docs, tq, reps, with_cpu):
    import torch
    from yams_amd import _lib
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    L, ctx = acc.L, acc.ctx
    rng = np.random.default_rng(dim * 1000 + n_docs + tq)
    q, x = mixed(rng, (tq, dim), -3, 3), mixed(rng, (n_docs * TOKENS, dim), -3, 3)
    off = np.arange(n_docs + 1, dtype=np.uint64) * TOKENS
    d_q, d_x, d_off = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
    d_sc = torch.empty(n_docs, dtype=torch.float32, device="cuda")
    h_sc = np.empty(n_docs, np.float32)
    steps = n_docs * TOKENS * tq * dim
    res = {"shape": {"dim": dim, "n_docs": n_docs, "doc_tokens": TOKENS, "query_tokens": tq}, "chain_steps": steps, "forms": {}}
    for form, name in ((_lib.RESIDUAL_SEPARATE, "separate"), (_lib.RESIDUAL_FUSED, "fused")):
        dg = _lib.RerankDiag()

        def dev():
            acc._check(L.yams_rerank_maxsim_device(ctx, d_q.data_ptr(), tq, dim, d_x.data_ptr(), d_off.data_ptr(), n_docs, form, d_sc.data_ptr(),
                                                   None, None, dg))

        def host():
            acc._check(L.yams_rerank_maxsim_host(ctx, q.ctypes.data, tq, dim, x.ctypes.data, off.ctypes.data, n_docs, form, h_sc.ctypes.data,
                                                 None, None, None))
        dev(); dev()
        ts = []
        for _ in range(reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); dev(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        got = d_sc.cpu().numpy()
        host()
        hs = []
        for _ in range(reps):
            t0 = time.perf_counter(); host(); hs.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(ts)) * 1e-3
        f = {"device_ms": spread(ts), "host_entry_ms": spread(hs), "host_entry_equals_device": same(h_sc, got),
             "path": {_lib.RERANK_PATH_VALU: "valu", _lib.RERANK_PATH_MFMA: "mfma"}[dg.path],
             "chain_steps_per_second": steps / med, "tflops": 2 * steps / med / 1e12, "fraction_of_fp32_peak": 2 * steps / med / 1e12 / PEAK_TF}
        if with_cpu:
            with tempfile.TemporaryDirectory() as tmp:
                cpu = cpu_lib(tmp)
                want = np.empty(n_docs, np.float32)
                t0 = time.perf_counter()
                cpu.maxsim_cpu(q.ctypes.data, tq, dim, x.ctypes.data, off.ctypes.data, n_docs, form, want.ctypes.data)
                sec = time.perf_counter() - t0
            f["cpu_cpp_restatement_one_core"] = {"seconds": sec, "chain_steps_per_second": steps / sec, "bits_equal_the_device": same(want, got),
                                                 "over_device_call": sec / med, "over_host_entry_call": sec / (float(np.median(hs)) * 1e-3)}
        res["forms"][name] = f
    info = acc.device_info()
    res["device"] = {k: info[k] for k in ("name", "arch", "compute_units") if k in info}
    acc.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--shape", default=None, help="internal: dim,n_docs,tq — run one shape in this process and print its JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 repetitions"
    if a.shape:
        dim, n_docs, tq = (int(v) for v in a.shape.split(","))
        print("SHAPE_RESULT " + json.dumps(run_shape(dim, n_docs, tq, a.reps, not a.no_cpu)), flush=True)
        return
    out = {"reps": a.reps, "warm_up_calls": 2, "fp32_peak_tflops_assumed": PEAK_TF, "shapes": [],
           "not_measured": ["hardware counters", "late_interaction_rerank_v1 through the plugin door and the shell's flattening",
                            "documents of unequal lengths", "the pooling entry", "the reference's own translation unit (it needs ONNX Runtime)"]}
    for dim, n_docs, tq in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{dim},{n_docs},{tq}", "--reps", str(a.reps)] + (["--no-cpu"] if a.no_cpu else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=SHAPE_TIMEOUT)
        except subprocess.TimeoutExpired:
            out["shapes"].append({"shape": [dim, n_docs, tq], "error": f"time limit of {SHAPE_TIMEOUT} s"})
            print((dim, n_docs, tq), "hit its time limit: stopping", flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("SHAPE_RESULT ")]
        if r.returncode != 0 or not line:
            out["shapes"].append({"shape": [dim, n_docs, tq], "error": f"exit status {r.returncode}", "tail": (r.stdout + r.stderr)[-600:]})
            print((dim, n_docs, tq), "failed: stopping\n", (r.stdout + r.stderr)[-600:], flush=True)
            break
        out["shapes"].append(json.loads(line[0][len("SHAPE_RESULT "):]))
        print(json.dumps(out["shapes"][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(1 if any("error" in s for s in out["shapes"]) else 0)


if __name__ == "__main__":
    main()
