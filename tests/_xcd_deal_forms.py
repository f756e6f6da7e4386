"""Run as a subprocess by test_xcd_deal_gpu.py with YAMS_ACCEL_MEASURE_LIB=1 (the measurement library is chosen at import; its
YAMS_ACCEL_XCD_WEIGHTS knob forces the weights of the int8 sweep's deal of units to the XCDs): every shape with the weights
forced to equal, to both clamps alternating and to one XCD at the minimum, against the CPU oracle and against the equal-weight
run; then three calls in a row on one context with the feedback on.  Prints one JSON line: a record per shape."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import _oracle
from yams_amd.accel import Accel
from yams_amd import _lib
from yams_amd._lib import SCAN_COSINE, SCAN_L2, FLAG_RESIDENT_QUERIES

WEIGHTS = {"equal": "1,1,1,1,1,1,1,1", "clamps": "0.92,1.08,0.92,1.08,0.92,1.08,0.92,1.08", "one_min": "1,1,1,0.92,1,1,1,1"}
SHAPES = json.loads(os.environ["XCD_SHAPES"])          # [[rows, dim, queries, metric], ...]
K = 10
o = _oracle.oracle()
acc = Accel(0, torch.cuda.current_stream().cuda_stream)
shards = {}


def shard(n, d):
    if (n, d) not in shards:
        c = o.synth_rows(91, 0, n, d)
        tc = torch.from_numpy(c).cuda()
        tb = torch.empty((n, d), dtype=torch.bfloat16, device="cuda"); tn = torch.empty(n, dtype=torch.float32, device="cuda")
        acc.build_shadow_device(tc.data_ptr(), n, d, tb.data_ptr(), tn.data_ptr())
        t8 = torch.empty((_lib.i8_shadow_rows(n), d), dtype=torch.int8, device="cuda"); tm = torch.empty(((n + 63) // 64, 2), dtype=torch.float32, device="cuda")
        acc.build_shadow_i8_device(tc.data_ptr(), n, d, t8.data_ptr(), tm.data_ptr()); acc.synchronize()
        view = acc.corpus_view(tc.data_ptr(), n, d, rows_bf16_ptr=tb.data_ptr(), rows_nsq_ptr=tn.data_ptr(), rows_i8_ptr=t8.data_ptr(), rows_i8_meta_ptr=tm.data_ptr())
        shards[(n, d)] = (c, view, (tc, tb, tn, t8, tm))
    return shards[(n, d)]


def same(a, b, l2):
    return bool(np.array_equal(a.rows, b.rows) and np.array_equal(a.scores.view(np.uint32), b.scores.view(np.uint32)) and np.array_equal(a.counts, b.counts)
                and (not l2 or np.array_equal(a.dist.view(np.uint32), b.dist.view(np.uint32))))


out = []
for (n, d, nq, metric) in SHAPES:
    l2 = metric == "l2"
    c, view, _ = shard(n, d)
    q = o.synth_rows(91, (1 << 40) + nq, nq, d)
    ref = _oracle.scan_threaded(lambda lo, hi: c[lo:hi], n, q, K, metric=metric, thr=-1.0, slice_rows=8192)
    rec = {"shape": [n, d, nq, metric], "runs": {}}
    res = {}
    for name, w in WEIGHTS.items():
        os.environ["YAMS_ACCEL_XCD_WEIGHTS"] = w
        r = acc.scan_topk(view, q, K, -1.0, SCAN_L2 if l2 else SCAN_COSINE, flags=FLAG_RESIDENT_QUERIES)
        res[name] = r
        info = acc.device_info().get("xcd_deal") or {}
        ok = True
        for qi in range(nq):
            t = ref[qi]
            cnt = int(r.counts[qi])
            ok &= cnt == len(t[0]) and np.array_equal(r.rows[qi, :cnt], t[0]) and np.array_equal(r.scores[qi, :cnt].view(np.uint32), t[1].view(np.uint32))
            if l2:
                ok &= np.array_equal(r.dist[qi, :cnt].view(np.uint32), t[2].view(np.uint32))
        rec["runs"][name] = {"tier": r.diag["filter_tier"], "oracle": bool(ok), "fallback": r.diag["exact_fallback_queries"], "candidates": r.diag["filter_candidates"],
                             "widened": r.diag["widened_queries"], "escalated": r.diag["escalated_queries"], "weights": info.get("weights"), "off": info.get("off"),
                             "units": info.get("units"), "same_as_equal": same(r, res["equal"], l2)}
    del os.environ["YAMS_ACCEL_XCD_WEIGHTS"]
    out.append(rec)

# feedback on (no knob): three calls in a row on one context of its own
n, d, nq = 66000, 768, 1024
c, view, _ = shard(n, d)
q = o.synth_rows(91, (1 << 40) + nq, nq, d)
acc2 = Accel(0, torch.cuda.current_stream().cuda_stream)
calls = []
first = None
for i in range(3):
    r = acc2.scan_topk(view, q, K, -1.0, SCAN_COSINE, flags=FLAG_RESIDENT_QUERIES)
    first = first or r
    info = acc2.device_info().get("xcd_deal") or {}
    calls.append({"weights": info.get("weights"), "off": info.get("off"), "units": info.get("units"), "same_as_first": same(r, first, False),
                  "fallback": r.diag["exact_fallback_queries"], "tier": r.diag["filter_tier"]})
os.environ["YAMS_ACCEL_XCD_WEIGHTS"] = WEIGHTS["equal"]
r = acc2.scan_topk(view, q, K, -1.0, SCAN_COSINE, flags=FLAG_RESIDENT_QUERIES)
print(json.dumps({"shapes": out, "feedback": {"calls": calls, "same_as_equal": same(first, r, False)}}))
