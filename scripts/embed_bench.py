"""The embedding model's pooling head on the device (yams_embed_pool) — the measurements of DESIGN 3.19.

  shapes     1 x 512 x 768 (the query), 64 x 512 x 768 with a realistic share of padding (text lengths drawn evenly from 32 to
             512 tokens, padded at the tail) and 256 x 512 x 1024 fully active; MEAN and MAX, normalised.  Values are
             mixed-exponent floats: no kernel's work depends on them.
  each shape runs in a process of its own under its own time limit (the parent never opens the device, and stops at the first
             shape that fails): per mode three warm-up calls, then --reps (>= 20) calls of the _device entry over device-resident
             hidden states, masks and output, timed between HIP events around the call (it synchronises; the mask check, its
             read-back and the finish launch are inside), then --reps calls of the _host entry timed with perf_counter (the
             upload of the hidden states and the way back included).  Median, minimum and maximum.
  cache      a call re-reading the input of the call before it may be served by the 256 MiB Infinity Cache, not by HBM.  A shape
             whose hidden states are larger than that cache alternates between TWO copies of them (a call then reads 512 MiB the
             previous call did not touch): its rate is an HBM rate, "input_rotated": true.  The smaller shapes fit the cache
             whole and are not rotated: their rate is reported as what it is, bytes over time, "input_rotated": false.
  yardstick  (never the code under test) a plain C++ restatement of the contract (CPU_LOOP below), -O2 -ffp-contract=off, ONE
             core of the same machine, on the same input, median of seven runs after one; its rows are compared with the
             device's on bits.
  rate       the bytes of the ACTIVE rows (active tokens x dim x 4) over the median device call, and that rate over the 8 TB/s
             HBM peak (a fraction of the HBM roof only where the input is rotated); the slab width the host chose (the diag).

    python scripts/embed_bench.py [--reps 20] [--out profiles/embed_pool.json] [--no-cpu]

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
SHAPES = [(1, 512, 768, "full"), (64, 512, 768, "padded"), (256, 512, 1024, "full")]      # batch, seq, dim, mask
HBM_PEAK = 8.0e12
CACHE_BYTES = 256 << 20      # the Infinity Cache
SHAPE_TIMEOUT = 280


CPU_LOOP = r'''
// The contract of yams_embed_pool restated in C++, scalar (built with -ffp-contract=off).  mode 1 MAX, 2 MEAN; normalised.
#include <algorithm>
#include <cmath>
#include <cstdint>
extern "C" void pool_cpu(const float* hidden, uint64_t batch, uint32_t seq, uint32_t dim, const int32_t* mask, uint32_t mask_len, int mode,
                         float* out) {
    for (uint64_t b = 0; b < batch; ++b) {
        float* emb = out + b * dim;
        for (uint32_t d = 0; d < dim; ++d) emb[d] = 0.0f;
        float total = 0.0f;
        for (uint32_t i = 0; i < std::min(seq, mask_len); ++i) {
            const float w = static_cast<float>(mask[b * mask_len + i]);
            if (w <= 0.0f) continue;
            const float* x = hidden + (b * seq + i) * dim;
            total = total + w;
            if (mode == 1) for (uint32_t d = 0; d < dim; ++d) emb[d] = std::max(emb[d], x[d]);
            else for (uint32_t d = 0; d < dim; ++d) { const float p = x[d] * w; emb[d] = emb[d] + p; }
        }
        if (mode == 2 && total > 0.0f) for (uint32_t d = 0; d < dim; ++d) emb[d] = emb[d] / total;
        double norm = 0.0;
        for (uint32_t d = 0; d < dim; ++d) norm += double(emb[d]) * double(emb[d]);
        norm = std::sqrt(norm);
        for (uint32_t d = 0; d < dim; ++d) emb[d] = norm > 1e-8 ? float(double(emb[d]) / norm) : 0.0f;
    }
}
'''


def cpu_lib(tmp):
    src, lib = os.path.join(tmp, "embed_cpu.cpp"), os.path.join(tmp, "embed_cpu.so")
    open(src, "w").write(CPU_LOOP)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src], check=True)
    L = C.CDLL(lib)
    L.pool_cpu.restype = None
    L.pool_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
    return L


def mixed(rng, shape, lo, hi):
    """Floats of mixed exponents 2^lo .. 2^hi and both signs, full mantissas."""
    x = rng.uniform(1.0, 2.0, shape).astype(np.float32)
    x *= np.exp2(rng.integers(lo, hi + 1, shape)).astype(np.float32)
    x *= rng.choice(np.array([-1.0, 1.0], np.float32), shape)
    return x


def same(a, b):
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def spread(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def run_shape(batch, seq, dim, kind, reps, with_cpu):
    import torch
    from yams_amd import _lib
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    L, ctx = acc.L, acc.ctx
    rng = np.random.default_rng(batch * 1000 + dim)
    x = mixed(rng, (batch, seq, dim), -3, 3)
    m = np.ones((batch, seq), np.int32)
    if kind == "padded":
        for b, n in enumerate(rng.integers(32, seq + 1, batch)):
            m[b, n:] = 0
    active = int(m.sum())
    d_x, d_m = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
    rotated = x.nbytes > CACHE_BYTES
    d_xs = [d_x, d_x.clone()] if rotated else [d_x]
    turn = [0]
    d_out = torch.empty((batch, dim), dtype=torch.float32, device="cuda")
    h_out = np.empty((batch, dim), np.float32)
    res = {"shape": {"batch": batch, "seq": seq, "dim": dim, "mask": kind}, "active_tokens": active, "active_bytes": active * dim * 4,
           "hidden_bytes": x.nbytes, "input_rotated": rotated, "modes": {}}
    for mode, name in ((_lib.EMBED_POOL_MEAN, "mean"), (_lib.EMBED_POOL_MAX, "max")):
        dg = _lib.EmbedDiag()

        def dev():
            turn[0] += 1
            acc._check(L.yams_embed_pool_device(ctx, d_xs[turn[0] % len(d_xs)].data_ptr(), batch, seq, dim, d_m.data_ptr(), seq, mode, _lib.EMBED_NORMALIZE, d_out.data_ptr(), dg))

        def host():
            acc._check(L.yams_embed_pool_host(ctx, x.ctypes.data, batch, seq, dim, m.ctypes.data, seq, mode, _lib.EMBED_NORMALIZE, h_out.ctypes.data, None))
        dev(); dev(); dev()
        ts = []
        for _ in range(reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); dev(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        got = d_out.cpu().numpy()
        host()
        hs = []
        for _ in range(reps):
            t0 = time.perf_counter(); host(); hs.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(ts)) * 1e-3
        f = {"device_ms": spread(ts), "host_entry_ms": spread(hs), "host_entry_equals_device": same(h_out, got), "slab_dims": dg.slab_dims,
             "active_bytes_per_second": active * dim * 4 / med, "active_bytes_per_second_over_hbm_peak": active * dim * 4 / med / HBM_PEAK}
        if with_cpu:
            with tempfile.TemporaryDirectory() as tmp:
                cpu = cpu_lib(tmp)
                want = np.empty((batch, dim), np.float32)
                cs = []
                for run in range(8):
                    t0 = time.perf_counter()
                    cpu.pool_cpu(x.ctypes.data, batch, seq, dim, m.ctypes.data, seq, mode, want.ctypes.data)
                    cs.append(time.perf_counter() - t0)
                cs = cs[1:]
            sec = float(np.median(cs))
            f["cpu_cpp_restatement_one_core"] = {"seconds": spread(cs), "bits_equal_the_device": same(want, got), "over_device_call": sec / med,
                                                 "over_host_entry_call": sec / (float(np.median(hs)) * 1e-3)}
        res["modes"][name] = f
    info = acc.device_info()
    res["device"] = {k: info[k] for k in ("name", "arch", "compute_units") if k in info}
    acc.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--shape", default=None, help="internal: batch,seq,dim,mask — run one shape in this process and print its JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 repetitions"
    if a.shape:
        batch, seq, dim, kind = a.shape.split(",")
        print("SHAPE_RESULT " + json.dumps(run_shape(int(batch), int(seq), int(dim), kind, a.reps, not a.no_cpu)), flush=True)
        return
    out = {"reps": a.reps, "warm_up_calls": 3, "hbm_peak_bytes_per_second_assumed": HBM_PEAK, "shapes": [],
           "not_measured": ["hardware counters", "embedding_pool_v1 through the plugin door and the shell's flattening", "CLS", "the rank-2 entry",
                            "an encoder writing the hidden states on the same device", "the reference's own translation unit (it needs ONNX Runtime)"]}
    for batch, seq, dim, kind in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{batch},{seq},{dim},{kind}", "--reps", str(a.reps)] + (["--no-cpu"] if a.no_cpu else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=SHAPE_TIMEOUT)
        except subprocess.TimeoutExpired:
            out["shapes"].append({"shape": [batch, seq, dim, kind], "error": f"time limit of {SHAPE_TIMEOUT} s"})
            print((batch, seq, dim), "hit its time limit: stopping", flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("SHAPE_RESULT ")]
        if r.returncode != 0 or not line:
            out["shapes"].append({"shape": [batch, seq, dim, kind], "error": f"exit status {r.returncode}", "tail": (r.stdout + r.stderr)[-600:]})
            print((batch, seq, dim), "failed: stopping\n", (r.stdout + r.stderr)[-600:], flush=True)
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
