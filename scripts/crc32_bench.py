"""The batched CRC-32 on the device (yams_crc32_*) — the measurements of DESIGN 3.12:

  (a) 8 GiB resident as 2048 x 4 MiB Philox blobs, chunked with the default configuration: the CRC pass over the chunk
      table (yams_crc32_batch_device and the fused yams_crc32_chunks_device) in GB/s and as a fraction of 8 TB/s, and IN THE
      SAME RUN yams_sha256_batch_device over the same table.  The pass mark is relative to that existing code: the CRC pass
      is at least as fast as the SHA-256 pass.
  (b) one 1 GiB message
  (c) 2^20 messages of 64 bytes
  (d) yams_crc32_many_host over 8 GiB of host memory (2048 x 4 MiB)

    python scripts/crc32_bench.py [--reps 3] [--only all|a] [--gib 8] [--out profiles/crc32.json]
    python scripts/crc32_bench.py --rocprof-stats kernel_stats.csv --out profiles/crc32.json

HIP events around calls that end in a synchronise, one warm-up call first, each figure the median of --reps calls.  A sample
of the results is checked against zlib.crc32 before anything is timed.  --only a runs shape (a) alone (the run to put under
`rocprofv3 --kernel-trace --stats`, in a run of its own); --rocprof-stats folds that run's kernel summary into an existing
output file.  Figures that were not taken on a device are recorded as "not_run"."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yams_amd.accel import Accel, cdc_config  # noqa: E402

HBM_TBS = 8.0
CPU_RATES = {"note": "restated loops on one core of a development machine (not the GPU box), g++ -O2, 64 MiB of random bytes",
             "bit_at_a_time_MBps": 76, "byte_table_MBps": 271}


def rocprof_summary(path):
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "crc32" in name or "sha256" in name:
                out.append({"kernel": name.split("(")[0], "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                            "average_ns": float(r["AverageNs"]), "percent": float(r["Percentage"])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["all", "a"], default="all")
    ap.add_argument("--gib", type=int, default=8)
    ap.add_argument("--rocprof-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rocprof_stats and a.out and os.path.exists(a.out):
        res = json.load(open(a.out))
        res["rocprofv3_kernel_stats_shape_a"] = rocprof_summary(a.rocprof_stats)
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps(res["rocprofv3_kernel_stats_shape_a"]))
        return
    import torch
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        fn()                                                    # warm-up: workspace allocation, code objects
        ts = []
        for _ in range(a.reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), ts

    def rate(nbytes, ms):
        return {"ms": ms, "GBps": nbytes / ms / 1e6, "frac_of_8TBps": nbytes / ms / 1e6 / (HBM_TBS * 1e3)}

    blob_len, n_blobs = 4 << 20, a.gib * 256
    total = blob_len * n_blobs
    data = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    acc.synth_bytes(7, 0, n_blobs, blob_len, data.data_ptr())
    offs = np.arange(n_blobs, dtype=np.uint64) * blob_len
    res_ing = acc.ingest_device(data.data_ptr(), offs, np.full(n_blobs, blob_len, np.uint64), cdc_config("streaming"), flags=0)
    tab = acc.fetch_ingest(res_ing, n_blobs)
    n = int(tab["n_chunks"])
    m_off = offs[tab["chunk_blob"]] + tab["chunk_offset"]
    m_len = tab["chunk_size"]
    d_off = torch.from_numpy(m_off.view(np.int64)).cuda(); d_len = torch.from_numpy(m_len.view(np.int64)).cuda()
    d_crc = torch.empty(n, dtype=torch.int32, device="cuda"); d_dg = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    # a sample against zlib before anything is timed
    acc.crc32_chunks_device(data.data_ptr(), offs, res_ing, d_crc.data_ptr())
    got = d_crc.cpu().numpy().view(np.uint32)
    for i in np.linspace(0, n - 1, 24).astype(int):
        b = data[int(m_off[i]):int(m_off[i] + m_len[i])].cpu().numpy().tobytes()
        assert zlib.crc32(b) & 0xFFFFFFFF == int(got[i]), ("chunk", int(i))
    info = acc.device_info()
    res = {"device": {k: info[k] for k in ("name", "arch", "compute_units") if k in info}, "reps": a.reps, "cpu_loops": CPU_RATES,
           "segment_bytes": 4096}
    crc_ms, crc_all = timed(lambda: acc.crc32_batch_device(data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, d_crc.data_ptr()))
    fused_ms, _ = timed(lambda: acc.crc32_chunks_device(data.data_ptr(), offs, res_ing, d_crc.data_ptr()))
    sha_ms, sha_all = timed(lambda: (acc.sha256_batch_device(data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, d_dg.data_ptr()), acc.synchronize()))
    acc.enable_timing(True)
    acc.crc32_batch_device(data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, d_crc.data_ptr())
    parts = {k: acc.kernel_ms(k)[0] for k in ("crc32_plan", "crc32_segments", "crc32_fold")}
    acc.enable_timing(False)
    res["a_chunk_table"] = {"bytes": total, "chunks": n, "crc32_batch_device": {**rate(total, crc_ms), "ms_all_reps": crc_all, "kernel_ms": parts},
                            "crc32_chunks_device": rate(total, fused_ms), "sha256_batch_device": {**rate(total, sha_ms), "ms_all_reps": sha_all},
                            "crc_over_sha_speed": sha_ms / crc_ms, "pass_mark_crc_at_least_as_fast_as_sha256": bool(crc_ms <= sha_ms)}
    if a.only == "all":
        one = 1 << 30
        o1 = torch.tensor([3], dtype=torch.int64, device="cuda"); l1 = torch.tensor([one], dtype=torch.int64, device="cuda")
        ms, _ = timed(lambda: acc.crc32_batch_device(data.data_ptr(), o1.data_ptr(), l1.data_ptr(), 1, d_crc.data_ptr()))
        res["b_one_1GiB_message"] = rate(one, ms)
        k = 1 << 20
        os_ = torch.arange(k, dtype=torch.int64, device="cuda") * 64; ls = torch.full((k,), 64, dtype=torch.int64, device="cuda")
        dk = torch.empty(k, dtype=torch.int32, device="cuda")
        ms, _ = timed(lambda: acc.crc32_batch_device(data.data_ptr(), os_.data_ptr(), ls.data_ptr(), k, dk.data_ptr()))
        res["c_2^20_messages_of_64_bytes"] = {**rate(64 * k, ms), "messages_per_s": k / ms * 1e3}
        host = data[:total].cpu().numpy()
        ptrs = (C.c_void_p * n_blobs)(*[host.ctypes.data + i * blob_len for i in range(n_blobs)])
        lens = (C.c_size_t * n_blobs)(*([blob_len] * n_blobs))
        out = np.zeros(n_blobs, np.uint32)
        ms, _ = timed(lambda: acc._check(acc.L.yams_crc32_many_host(acc.ctx, ptrs, lens, n_blobs, out.ctypes.data_as(C.POINTER(C.c_uint32)))))
        assert int(out[5]) == zlib.crc32(host[5 * blob_len:6 * blob_len].tobytes()) & 0xFFFFFFFF
        res["d_many_host"] = {**rate(total, ms), "memory": "pageable", "messages": n_blobs}
        res["rocprofv3_kernel_stats_shape_a"] = "not_run"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
