"""Seeded randomised stress of the device semantic-neighbour graph (yams_graph_semantic_neighbors_device / _host) against the
restatement of tests/_semgraph_oracle.py, on ONE context: shapes around the tile edges (128 sources, 64 candidates, 8
dimensions per stage) and dims that are no multiple of four; uniform, clustered and duplicate-heavy rows (plateaus the tie rank
has to cut); zero rows; both admission modes; K from 1 to 64; with and without tie_rank and source_rows (unordered, repeated);
every fifth case through the host entry; every twentieth a shape the stripe rule splits.  Every case has
n * n_sources * dim <= 2e8, so the numpy oracle stays the slower side.  Every case is held to the oracle bit for bit: rows,
similarity bits, counts, inverse-norm bits, pairs_scored, pairs_admitted.

    python tests/stress_semgraph.py [--cases 150] [--seed 1] [--dry-run] [--self-test]

The harness stops at the first failing case, never retries and skips no case.  --dry-run draws the cases and runs the oracle
without touching the device.  --self-test checks the comparison itself: a result with one bit flipped in each output in turn
must be reported as different.  The last line is {"mode", "cases", "skipped", "paths"}."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _semgraph_oracle as so

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=150)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--dry-run", action="store_true")
ap.add_argument("--self-test", action="store_true")
a = ap.parse_args()
rng = np.random.default_rng(a.seed)
WORK_CAP = 2 * 10 ** 8

PATHS = ["vec4", "scalar", "uniform", "clustered", "duplicate_heavy", "zero_rows", "adaptive", "explicit", "tie_rank", "row_order",
         "source_rows", "all_sources", "host_entry", "several_source_tiles", "several_candidate_tiles", "stripes", "short_lists",
         "full_lists", "k_max", "plateau_cut"]
hits = {p: 0 for p in PATHS}


def draw(case):
    dim = int(rng.choice([1, 2, 3, 5, 7, 8, 9, 16, 33, 64, 96])) if rng.random() < 0.8 else int(rng.integers(1, 400))
    n = int(rng.choice([2, 3, 63, 64, 65, 127, 128, 129, 191, 193, 257])) if rng.random() < 0.35 else int(np.exp(rng.uniform(np.log(2), np.log(1200))))
    sources = None
    if case % 20 == 7:                                        # few sources over many candidates: the stripe rule splits
        n, dim = int(rng.integers(2000, 7000)), int(rng.choice([4, 8, 13, 32]))
        sources = rng.integers(0, n, int(rng.integers(1, 130))).astype(np.uint32)
    elif rng.random() < 0.4:
        sources = rng.integers(0, n, int(rng.choice([1, 2, 127, 129, max(1, n // 3), 2 * n]))).astype(np.uint32)
    kind = ["uniform", "clustered", "duplicate_heavy"][case % 3]
    s = int(rng.integers(1 << 30))
    rows = so.uniform_rows(s, n, dim) if kind == "uniform" else so.clustered_rows(s, n, dim, int(rng.integers(1, 9)), float(rng.choice([0.02, 0.3]))) \
        if kind == "clustered" else so.duplicate_rows(s, n, dim, int(rng.integers(1, 7)))
    if rng.random() < 0.3:
        rows[rng.random(n) < 0.05] = 0.0
    S = n if sources is None else len(sources)
    while n * S * dim > WORK_CAP:                             # the stated bound: halve the sources until the case fits
        sources = sources[:len(sources) // 2] if sources is not None else np.arange(n // 2, dtype=np.uint32)
        S = len(sources)
    k = int(rng.choice([1, 2, 8, 8, 16, 63, 64])) if rng.random() < 0.7 else int(rng.integers(1, 65))
    threshold = None if case % 2 == 0 else float(rng.choice([-1.0, 0.0, 0.25, 0.5, 0.9, 1.0]))
    rank = so.shuffled_rank(s + 1, n) if rng.random() < 0.6 else None
    return kind, rows, k, rank, sources, threshold, case % 5 == 4


def differs(got, want):
    g_rows, g_sims, g_counts, g_inv, diag = got
    return [name for name, x, y in (("rows", g_rows, want["rows"]), ("sims", so.bits(g_sims), so.bits(want["sims"])), ("counts", g_counts, want["counts"]),
                                    ("inv", so.bits(g_inv), so.bits(want["inv"])),
                                    ("pairs_scored", diag["pairs_scored"], want["pairs_scored"]),
                                    ("pairs_admitted", diag["pairs_admitted"], want["pairs_admitted"])) if not np.array_equal(x, y)]


if a.self_test:
    rows = so.duplicate_rows(3, 90, 5, 4)
    want = so.neighbors(rows, 8, so.shuffled_rank(4, 90))
    exact = lambda: (want["rows"].copy(), want["sims"].copy(), want["counts"].copy(), want["inv"].copy(),
                     dict(pairs_scored=want["pairs_scored"], pairs_admitted=want["pairs_admitted"]))
    assert differs(exact(), want) == []
    for i, name in enumerate(["rows", "sims", "counts", "inv"]):
        g = exact()
        g[i].reshape(-1).view(np.uint32)[5] ^= 1
        assert differs(g, want) == [name], name
    for name in ("pairs_scored", "pairs_admitted"):
        g = exact(); g[4][name] += 1
        assert differs(g, want) == [name], name
    z = exact(); z[1][0, 0] = np.float32(-0.0); w2 = dict(want); w2["sims"] = want["sims"].copy(); w2["sims"][0, 0] = np.float32(0.0)
    assert differs(z, w2) == ["sims"]                         # the two zeros are different bits to the comparison
    print(json.dumps({"mode": "self-test", "ok": True}))
    sys.exit(0)

acc = None
if not a.dry_run:
    import torch
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)

checked = 0
for case in range(a.cases):
    kind, rows, k, rank, sources, threshold, host_entry = draw(case)
    n, dim = rows.shape
    S = n if sources is None else len(sources)
    assert n * S * dim <= WORK_CAP
    want = so.neighbors(rows, k, rank, sources, threshold)
    hits["vec4" if dim % 4 == 0 else "scalar"] += 1
    hits[kind] += 1
    hits["zero_rows"] += bool((want["inv"] == 0).any())
    hits["adaptive" if threshold is None else "explicit"] += 1
    hits["tie_rank" if rank is not None else "row_order"] += 1
    hits["source_rows" if sources is not None else "all_sources"] += 1
    hits["host_entry"] += host_entry
    hits["several_source_tiles"] += S > 128
    hits["several_candidate_tiles"] += n > 64
    split = (S + 127) // 128 < 512 and (n + 63) // 64 >= 8                # semgraph_geometry: CUs to spare, four tiles a stripe
    hits["stripes"] += split
    hits["short_lists"] += bool((want["counts"] < k).any())
    hits["full_lists"] += bool((want["counts"] == k).any())
    hits["k_max"] += k >= 63
    full = want["counts"] == k
    if full.any() and n - 1 > k:
        deeper = so.neighbors(rows, k + 1, rank, sources, threshold) if n * S * dim <= WORK_CAP // 8 else None
        if deeper is not None:
            both = full & (deeper["counts"] == k + 1)
            hits["plateau_cut"] += bool((so.bits(deeper["sims"][both, k - 1]) == so.bits(deeper["sims"][both, k])).any())
    if acc is not None:
        got = acc.semantic_neighbors(rows, k, tie_rank=rank, source_rows=sources, threshold=threshold, host_entry=host_entry)
        bad = differs(got, want)
        if (got[4]["stripes"] > 1) != split:                   # the path this case is counted under is the one it took
            bad.append("stripes")
        if bad:
            print(json.dumps({"failed_case": case, "seed": a.seed, "n": n, "dim": dim, "k": k, "sources": S, "threshold": threshold,
                              "tie_rank": rank is not None, "host_entry": host_entry, "differs": bad, "diag": got[4]}))
            sys.exit(1)
    checked += 1
print(json.dumps({"mode": "dry-run" if a.dry_run else "device", "seed": a.seed, "cases": checked, "skipped": a.cases - checked,
                  "paths": {p: int(v) for p, v in hits.items()}}))
