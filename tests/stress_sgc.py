"""Seeded randomised stress of SGC smoothing on the device (yams_graph_sgc_smooth_device / _host) against the restatement of
tests/_sgc_oracle.py, on ONE context (so the workspace is reused across shapes): dims that are and are not a multiple of four,
up to 4096; rows without edges; zero weights (the skip at scale 0.0); self-loops and repeated columns; -0.0f, denormal and
+-FLT_MAX / 4 elements; a hub row past YAMS_SGC_HUB_DEGREE in every tenth case; 1 to 4 hops; every fifth case through the host
entry.  Every case has nnz * dim * hops <= 4e7, so the numpy oracle stays the slower side.  Every case is held to the oracle bit
for bit (a NaN matches any NaN), with nnz, max_degree, edges_skipped_zero_scale and hub_rows.

    python tests/stress_sgc.py [--cases 60] [--seed 1] [--dry-run] [--self-test]

The harness stops at the first failing case, never retries and skips no case.  --dry-run draws the cases and runs the oracle
without touching the device.  --self-test checks the comparison itself: a result with one bit flipped must be reported as
different, the two zeros are different bits, and two NaNs of different payloads are the same.  The last line is
{"mode", "cases", "skipped", "paths"}."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _sgc_oracle as sg

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--dry-run", action="store_true")
ap.add_argument("--self-test", action="store_true")
a = ap.parse_args()
rng = np.random.default_rng(a.seed)
WORK_CAP = 4 * 10 ** 7

PATHS = ["vec4", "scalar", "empty_rows", "zero_scale", "self_loop", "repeated_column", "hub_row", "one_hop", "even_hops", "odd_hops",
         "host_entry", "several_workgroups", "wide_dim", "negative_zero_kept"]
hits = {p: 0 for p in PATHS}


def draw(case):
    dim = int(rng.choice([1, 3, 4, 5, 8, 37, 64, 100, 384])) if rng.random() < 0.8 else int(rng.choice([1024, 1025, 4095, 4096]))
    n = int(rng.choice([2, 3, 63, 64, 65, 255, 257])) if rng.random() < 0.4 else int(np.exp(rng.uniform(np.log(2), np.log(1500))))
    hops = int(rng.choice([1, 1, 2, 2, 3, 4]))
    deg = int(rng.choice([1, 4, 8, 16]))
    hub = None
    if case % 10 == 3:
        hub = (int(rng.integers(n)), int(rng.choice([sg.HUB_DEGREE - 1, sg.HUB_DEGREE, sg.HUB_DEGREE + 1, 1500])))
    while (n * deg + (hub[1] if hub else 0)) * dim * hops > WORK_CAP and n > 2:
        n //= 2
        if hub:
            hub = (hub[0] % n, hub[1])
    s = int(rng.integers(1 << 30))
    x, off, cols, w = sg.seeded_case(s, n, dim, deg, hub=hub)
    return x, off, cols, w, hops, case % 5 == 4


def differs(got, want):
    out, diag = got
    y, wd = want
    bad = [] if sg.same_bits(out, y) else ["out"]
    return bad + [k for k in ("nnz", "max_degree", "edges_skipped_zero_scale", "hops", "hub_rows") if diag[k] != wd[k]]


if a.self_test:
    x, off, cols, w = sg.seeded_case(3, 90, 5, 6)
    want = sg.smooth(x, off, cols, w, 2, with_diag=True)
    exact = lambda: (want[0].copy(), dict(want[1]))
    assert differs(exact(), want) == []
    g = exact(); g[0].reshape(-1).view(np.uint32)[7] ^= 1
    assert differs(g, want) == ["out"]
    for name in ("nnz", "max_degree", "edges_skipped_zero_scale", "hops", "hub_rows"):
        g = exact(); g[1][name] += 1
        assert differs(g, want) == [name], name
    z = exact(); z[0][0, 0] = np.float32(-0.0); w2 = (want[0].copy(), want[1]); w2[0][0, 0] = np.float32(0.0)
    assert differs(z, w2) == ["out"]                          # the two zeros are different bits to the comparison
    z[0].view(np.uint32)[0, 0] = 0x7fc00001; w2[0].view(np.uint32)[0, 0] = 0xffc00000
    assert differs(z, w2) == []                               # a NaN matches any NaN
    print(json.dumps({"mode": "self-test", "ok": True}))
    sys.exit(0)

acc = None
if not a.dry_run:
    import torch
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)

checked = 0
for case in range(a.cases):
    x, off, cols, w, hops, host_entry = draw(case)
    n, dim = x.shape
    want = sg.smooth(x, off, cols, w, hops, with_diag=True)
    cnt = np.diff(off.astype(np.int64))
    row_of_edge = np.repeat(np.arange(n), cnt)
    hits["vec4" if dim % 4 == 0 else "scalar"] += 1
    hits["empty_rows"] += bool((cnt == 0).any())
    hits["zero_scale"] += want[1]["edges_skipped_zero_scale"] > 0
    hits["self_loop"] += bool((cols == row_of_edge).any())
    hits["repeated_column"] += bool(len(np.unique(row_of_edge.astype(np.int64) * n + cols)) < len(cols))
    hits["hub_row"] += want[1]["hub_rows"] > 0
    hits["one_hop" if hops == 1 else "even_hops" if hops % 2 == 0 else "odd_hops"] += 1
    hits["host_entry"] += host_entry
    hits["several_workgroups"] += n * ((dim + 3) // 4) > 256
    hits["wide_dim"] += dim >= 1024
    hits["negative_zero_kept"] += bool((sg.bits(want[0]) == 0x80000000).any())
    if acc is not None:
        got = acc.sgc_smooth(x, off, cols, w, hops, host_entry=host_entry)
        bad = differs(got, want)
        if bad:
            print(json.dumps({"failed_case": case, "seed": a.seed, "n": n, "dim": dim, "hops": hops, "host_entry": host_entry, "differs": bad,
                              "diag": got[1], "want_diag": want[1],
                              "first": np.argwhere(~((sg.bits(got[0]) == sg.bits(want[0])) | (np.isnan(got[0]) & np.isnan(want[0]))))[:4].tolist()}))
            sys.exit(1)
    checked += 1
print(json.dumps({"mode": "dry-run" if a.dry_run else "device", "seed": a.seed, "cases": checked, "skipped": a.cases - checked,
                  "paths": {p: int(v) for p, v in hits.items()}}))
