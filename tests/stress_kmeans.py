"""Seeded randomised stress of the device k-means (yams_cluster_kmeans_device, yams_cluster_assign_device) against the
restatement of tests/_kmeans_oracle.py: shapes (dims that are not a multiple of four, rows around the tile edges of the
assignment kernel), k (default, explicit, above n), iteration caps, duplicate density (ties, duplicate centroids, the repair
path), zero rows, and four rare bands drawn by case number: more than 65536 rows (a thread of kmeans_pick_kernel strides over
the block partials), k_eff above 256 (kmeans_scan_kernel sums several clusters per thread), dim from 4000 to the limit of 4096,
-0.0f elements.  The rare bands keep dim or n small so that the oracle stays quick.  Every case is held to the oracle bit for bit: membership, centroid bits, effective k, iterations run; every
third case also checks yams_cluster_assign_device (skipped centroids, fp64 distance bits) over the case's centroids.

    python tests/stress_kmeans.py [--cases 60] [--seed 1] [--dry-run]

The harness stops at the first failing case and never retries.  --dry-run draws the cases and runs the oracle without touching
the device: the coverage counters the last line reports ({"mode", "cases", "paths"}) are then the oracle's alone.
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _kmeans_oracle as ko

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--dry-run", action="store_true")
a = ap.parse_args()
rng = np.random.default_rng(a.seed)
acc = None
if not a.dry_run:
    import torch
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)

PATHS = ["vec4", "scalar", "default_k", "explicit_k", "k_above_n", "iteration_cap", "converged", "duplicates", "zero_rows",
         "several_centroid_tiles", "several_row_tiles", "empty_cluster", "assign_skip", "strided_partials", "scan_segments",
         "max_dim_band", "negative_zero"]
hits = {p: 0 for p in PATHS}


def draw(case):
    dim = int(rng.choice([1, 2, 3, 5, 8, 16, 33, 50, 64, 96])) if rng.random() < 0.8 else int(rng.integers(1, 140))
    n = int(rng.choice([2, 3, 127, 128, 129, 256, 257])) if rng.random() < 0.25 else int(np.exp(rng.uniform(np.log(2), np.log(1500))))
    band = {5: "strided", 11: "segments", 17: "max_dim"}.get(case % 20)
    if band == "strided":                                    # more than 256 block partials of 256 rows
        n, dim = int(rng.choice([65537, 65792, 65793, 70000, 131073])), int(rng.choice([2, 3, 4, 8]))
    elif band == "segments":                                 # room for more than 256 clusters
        n, dim = int(rng.integers(300, 1300)), int(rng.choice([3, 4, 6, 9]))
    elif band == "max_dim":
        n, dim = int(rng.integers(20, 200)), int(rng.choice([4000, 4093, 4095, 4096]))
    groups = max(1, int(rng.integers(1, 12)))
    centres = rng.standard_normal((groups, dim)).astype(np.float32)
    rows = (centres[rng.integers(0, groups, n)] + np.float32(rng.choice([0.05, 0.3, 1.0])) * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)
    dup = float(rng.choice([0.0, 0.0, 0.2, 0.6, 0.95]))
    if dup and n > 3:
        src = rng.integers(0, max(1, n // 8), n)
        take = rng.random(n) < dup
        rows[take] = rows[src[take]]
        hits["duplicates"] += 1
    if rng.random() < 0.3:
        rows[rng.random(n) < 0.05] = 0.0
        if rng.random() < 0.5:
            rows[0] = 0.0
    if rng.random() < 0.25:                                  # -0.0f elements, and a row of nothing else
        rows[rng.random(rows.shape) < 0.1] = -0.0
        if rng.random() < 0.5:
            rows[int(rng.integers(0, n))] = -0.0
    mode = case % 4
    k = 0 if mode == 0 else int(rng.integers(2, 2 * n + 3)) if mode == 1 else int(rng.integers(2, max(3, min(n, 200))))
    if case % 7 == 3:
        k = int(rng.integers(65, 150))                       # more than one centroid tile (64), when n allows
    iters = int(rng.choice([0, 0, 1, 2, 3, 25]))
    if band == "strided":
        k, iters = int(rng.integers(2, 9)), int(rng.choice([1, 2]))
    elif band == "segments":
        k, iters = int(rng.integers(257, n + 40)), int(rng.choice([1, 2]))
    elif band == "max_dim":
        k, iters = min(k, 12), min(iters or 10, 3)
    return rows, k, iters


checked = 0
for case in range(a.cases):
    rows, k, iters = draw(case)
    n, dim = rows.shape
    repairs = ko.REPAIRS[0]
    mem, cent, ke, ran = ko.kmeans(rows, k, iters)
    hits["vec4" if dim % 4 == 0 else "scalar"] += 1
    hits["default_k" if k == 0 else "k_above_n" if k > n else "explicit_k"] += 1
    hits["iteration_cap" if ran == (iters or 10) else "converged"] += 1
    hits["zero_rows"] += bool((~rows.any(axis=1)).any())
    hits["several_centroid_tiles"] += ke > 64
    hits["several_row_tiles"] += n > 128
    hits["empty_cluster"] += ko.REPAIRS[0] > repairs                    # the repair path moved a row
    hits["strided_partials"] += n > 65536
    hits["scan_segments"] += ke > 256
    hits["max_dim_band"] += dim >= 4000
    hits["negative_zero"] += bool(((rows == 0) & np.signbit(rows)).any())
    want_assign = None
    if case % 3 == 0:
        empty = (rng.random(ke) < 0.3).astype(np.uint8)
        want_assign = (empty,) + ko.nearest(rows, cent, empty)
        hits["assign_skip"] += bool(empty.any())
    if acc is not None:
        gm, gc, gk, gr = acc.cluster_kmeans(rows, k, iters)
        ok = gk == ke and gr == ran and np.array_equal(gm, mem) and ko.same_f32(gc, cent)
        if ok and want_assign is not None:
            ga, gd = acc.cluster_assign(rows, cent, want_assign[0])
            ok = np.array_equal(ga, want_assign[1]) and ko.same_f64(gd, want_assign[2])
        if not ok:
            print(json.dumps({"failed_case": case, "seed": a.seed, "n": n, "dim": dim, "k": k, "iters": iters, "k_eff": [int(gk), int(ke)],
                              "ran": [int(gr), int(ran)], "membership_differs": int((gm != mem).sum()) if gm.shape == mem.shape else -1}))
            sys.exit(1)
    checked += 1
print(json.dumps({"mode": "dry-run" if a.dry_run else "device", "seed": a.seed, "cases": checked, "paths": {p: int(v) for p, v in hits.items()}}))
