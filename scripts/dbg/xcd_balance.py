"""When does each XCD finish its share of the resident-query filter launch?  (measurement build, 100 MHz ticks)

The deal of 512-row units to the row streams is static: the launch ends with its slowest stream.  This script runs the bench shape
(ROWS x DIM, Q queries, LANES search lanes behind one sweep gate, four query batches in rotation), lets the measurement build append
the per-wave begin / end ticks of LAUNCHES filter launches (YAMS_ACCEL_DUMP_SYNC_LOG) and reduces every launch to the end of each XCD
(the latest wave of its streams) relative to the launch's last end.  The figure that matters is `idle_mean_us`: the launch's last end
minus the mean of the eight XCD ends — what a perfect deal could give back.  Also: the shader clock every XCD's waves ran at (the
kernel's own clock64 / wall_clock64), amdsmi's per-XCD clocks over the same window, and whether the ranking of the XCDs holds from
launch to launch and from lane to lane.

    python scripts/dbg/xcd_balance.py [out.json]          (YAMS_ACCEL_XCD_WEIGHTS=w0,...,w7 forces the deal's weights)
"""
import json, os, sys, tempfile, threading, time
os.environ["YAMS_ACCEL_MEASURE_LIB"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from yams_amd.accel import Accel, SweepGate
from yams_amd._lib import SCAN_COSINE
from yams_amd import telemetry as ytel

n, d, nq, k = int(os.environ.get("ROWS", 12_500_000)), int(os.environ.get("DIM", 768)), int(os.environ.get("Q", 1024)), 100
lanes, launches = int(os.environ.get("LANES", 2)), int(os.environ.get("LAUNCHES", 24))
acc0 = Accel(0, torch.cuda.current_stream().cuda_stream)
tc = torch.empty((n, d), dtype=torch.float32, device="cuda"); acc0.synth_rows(42, 0, n, d, tc.data_ptr())
tqs = []
for b in range(4):
    tq = torch.empty((nq, d), dtype=torch.float32, device="cuda"); acc0.synth_rows(42, (1 << 40) + b * nq, nq, d, tq.data_ptr()); tqs.append(tq)
tb = torch.empty((n, d), dtype=torch.bfloat16, device="cuda"); tn = torch.empty(n, dtype=torch.float32, device="cuda")
acc0.build_shadow_device(tc.data_ptr(), n, d, tb.data_ptr(), tn.data_ptr())
t8 = torch.empty(((n + 63) // 64 * 64, d), dtype=torch.int8, device="cuda"); tm8 = torch.empty(((n + 15) // 16, 2), dtype=torch.float32, device="cuda")
acc0.build_shadow_i8_device(tc.data_ptr(), n, d, t8.data_ptr(), tm8.data_ptr()); acc0.synchronize()
view = acc0.corpus_view(tc.data_ptr(), n, d, rows_bf16_ptr=tb.data_ptr(), rows_nsq_ptr=tn.data_ptr(), rows_i8_ptr=t8.data_ptr(), rows_i8_meta_ptr=tm8.data_ptr())
streams = [None] + [torch.cuda.Stream() for _ in range(lanes - 1)]
accs = [acc0] + [Accel(0, s.cuda_stream) for s in streams[1:]]
outs = [(torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"),
         torch.zeros(nq, dtype=torch.int32, device="cuda")) for _ in range(lanes)]
gate = SweepGate(0) if lanes > 1 else None
for c in accs:
    c.set_gate(gate)
torch.cuda.synchronize()


def run(count):
    errs = []

    def lane_fn(lane):
        try:
            torch.cuda.set_device(0)
            o = outs[lane]
            for i in range(lane, count, lanes):
                accs[lane].scan_topk_device(view, tqs[i % 4].data_ptr(), nq, k, -1.0, SCAN_COSINE, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                            flags=0, want_diag=False)
        except BaseException as e:       # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=lane_fn, args=(l,)) for l in range(lanes)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]


run(8 * lanes)                                         # warm-up: workspaces, clocks settled under the power cap
for c in accs:
    c.enable_timing(True)
torch.cuda.synchronize(); t0 = time.perf_counter()
run(40)
torch.cuda.synchronize(); step_ms = (time.perf_counter() - t0) / 40 * 1e3
filt = [c.kernel_ms("scan_filter") for c in accs]
for c in accs:
    c.enable_timing(False)

# amdsmi's per-XCD clocks while the dumped launches run
thr = None; clk = []; stop = False
try:
    thr = ytel.Throttle(ytel.hip_pci_bus(0))
except Exception:       # noqa: BLE001
    thr = None


def clock_fn():
    while not stop and thr is not None and thr.h is not None:
        s = thr.snapshot()
        if s and s.get("current_gfxclks_MHz"):
            clk.append(s["current_gfxclks_MHz"][:8])
        time.sleep(0.01)


log = os.path.join(tempfile.mkdtemp(), "sync_log.bin")
os.environ["YAMS_ACCEL_DUMP_SYNC_LOG"] = log
ct = threading.Thread(target=clock_fn); ct.start()
run(launches)
stop = True; ct.join()
del os.environ["YAMS_ACCEL_DUMP_SYNC_LOG"]
torch.cuda.synchronize()

w = np.fromfile(log, dtype=np.uint32)
n_qt = (nq + 127) // 128
recs, p = [], 0
while p + 4 <= w.size:
    assert w[p] == 0x58434442, hex(int(w[p]))
    ctx, words, ns = int(w[p + 1]), int(w[p + 2]), int(w[p + 3])
    body = w[p + 4:p + 4 + words][: words // 2]          # the filter launch's half
    dbg = body[ns * 4 * 32:].reshape(ns, 8, 32)            # [stream][wave][32]
    recs.append((ctx, ns, dbg))
    p += 4 + words
lane_of = {c: i for i, c in enumerate(sorted({r[0] for r in recs}))}
rows = []
for ctx, ns, dbg in recs:
    tb_ = dbg[:, :, 8:8 + n_qt].astype(np.int64); te = dbg[:, :, 16:16 + n_qt].astype(np.int64); un = dbg[:, :, 24:24 + n_qt].astype(np.int64)
    mhz = dbg[:, :, 0:n_qt].astype(np.float64)
    t_first = tb_.min()
    xcd = np.arange(ns) % 8                                # stream = st * 8 + xcd
    end_x = np.array([te[xcd == x].max() for x in range(8)]) - t_first
    beg_x = np.array([tb_[xcd == x].min() for x in range(8)]) - t_first
    end_s = te.max(axis=(1, 2)) - t_first                  # per stream
    last = end_x.max()
    rows.append({"lane": lane_of[ctx], "launch_us": last / 100.0,
                 "xcd_end_behind_last_us": [float(last - e) / 100.0 for e in end_x],
                 "xcd_begin_us": [float(b) / 100.0 for b in beg_x],
                 "idle_mean_us": float(last - end_x.mean()) / 100.0,
                 "stream_end_spread_us": float(end_s.max() - end_s.min()) / 100.0,
                 "xcd_MHz": [float(mhz[xcd == x].mean()) for x in range(8)],
                 "units_per_xcd": [int(un[xcd == x].sum()) // (8 * n_qt) for x in range(8)],
                 "rank_slowest_first": [int(x) for x in np.argsort(-end_x)]})
behind = np.array([r["xcd_end_behind_last_us"] for r in rows])
mhz = np.array([r["xcd_MHz"] for r in rows])
rank_corr = []
for a in range(len(rows)):
    for b in range(a + 1, len(rows)):
        ra, rb = np.argsort(np.argsort(behind[a])), np.argsort(np.argsort(behind[b]))
        rank_corr.append(float(np.corrcoef(ra, rb)[0, 1]))
by_lane = {}
for l in sorted(set(r["lane"] for r in rows)):
    sel = np.array([r["lane"] == l for r in rows])
    by_lane[str(l)] = {"launches": int(sel.sum()), "mean_behind_last_us": behind[sel].mean(axis=0).round(2).tolist(), "mean_MHz": mhz[sel].mean(axis=0).round(1).tolist()}
out = {"shape": {"rows": n, "dim": d, "queries": nq, "lanes": lanes}, "weights_forced": os.environ.get("YAMS_ACCEL_XCD_WEIGHTS"),
       "step_ms": step_ms, "scan_filter_ms": [f[0] for f in filt], "launches": len(rows),
       "idle_mean_us": {"mean": float(np.mean([r["idle_mean_us"] for r in rows])), "min": float(np.min([r["idle_mean_us"] for r in rows])),
                        "max": float(np.max([r["idle_mean_us"] for r in rows]))},
       "launch_us_mean": float(np.mean([r["launch_us"] for r in rows])),
       "xcd_end_behind_last_us_mean": behind.mean(axis=0).round(2).tolist(), "xcd_end_behind_last_us_std": behind.std(axis=0).round(2).tolist(),
       "xcd_MHz_in_kernel_mean": mhz.mean(axis=0).round(1).tolist(),
       "xcd_MHz_amdsmi_mean": (np.array(clk, dtype=np.float64).mean(axis=0).round(1).tolist() if clk and len({len(c) for c in clk}) == 1 else None),
       "amdsmi_samples": len(clk),
       "rank_correlation_between_launches": {"mean": float(np.mean(rank_corr)) if rank_corr else None, "min": float(np.min(rank_corr)) if rank_corr else None},
       "slowest_xcd_histogram": np.bincount([r["rank_slowest_first"][0] for r in rows], minlength=8).tolist(),
       "by_lane": by_lane, "per_launch": rows}
dst = sys.argv[1] if len(sys.argv) > 1 else None
if dst:
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
out.pop("per_launch")
print(json.dumps(out))
