"""Stress of the cluster router's dense signal against tests/_route_oracle.py: seeded cases on ONE context, each a random
index (mixed segment sizes, special values, positions with gaps) created, queried a few times (query counts on both sides of
the kernels' thresholds, candidate masks, representative limits, device or host entry, aligned or not) and destroyed; every
comparison on bits.

    python tests/stress_route.py [--cases 60] [--seed 1]
    python tests/stress_route.py --dry-run      draws the cases and computes their oracle, no device
    python tests/stress_route.py --self-test    the comparison tells a flipped bit, no device
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _route_oracle as ro  # noqa: E402

DIMS = [1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 64, 100, 257]
QUERIES = [1, 2, 4, 5, 8, 9, 17, 63, 64, 65, 70]
F32 = np.float32


def draw(seed):
    rng = np.random.default_rng(seed)
    dim = int(rng.choice(DIMS))
    c = int(rng.integers(1, 8)) if rng.random() < 0.6 else int(rng.integers(30, 300))
    big = [0, 1, 2, 5, 64, 65] if c < 8 else [0, 1, 2, 3, 5]
    sizes = [int(rng.choice(big)) if rng.random() < 0.5 else int(rng.integers(0, 7)) for _ in range(c)]
    table = ro.random_table(rng, dim, sizes, centroid_prob=float(rng.choice([0.0, 0.5, 0.9, 1.0])), special=bool(rng.random() < 0.6))
    calls = []
    for _ in range(int(rng.integers(1, 4))):
        nq = int(rng.choice(QUERIES))
        q = rng.standard_normal((nq, dim)).astype(F32)
        if rng.random() < 0.4:
            kind = rng.integers(0, 4)
            q[rng.integers(0, nq)] = [0.0, np.nan, np.inf, 1e-30][kind] if kind != 3 else q[0] * F32(1e-30)
        mask = None
        if rng.random() < 0.5:
            mask = rng.random((nq, c)) < float(rng.choice([0.0, 0.1, 0.5, 1.0]))
        top = int(table.position.max()) + 1 if table.position.size else 1
        calls.append({"queries": q, "rep_limit": int(rng.choice([0, 1, 2, top, top + 1])), "mask": mask, "host": bool(rng.random() < 0.3),
                      "misalign": 4 if rng.random() < 0.3 else 0})
    return {"seed": seed, "dim": dim, "table": table, "calls": calls, "host": bool(rng.random() < 0.3), "misalign": 4 if rng.random() < 0.3 else 0}


def oracle(case):
    t = case["table"]
    return {"norms": t.norms, "calls": [ro.dense_signal(t, c["queries"], c["rep_limit"], c["mask"]) for c in case["calls"]]}


def device(acc, case):
    t = case["table"]
    index = acc.route_index(t.vectors, t.offsets, t.has_centroid, t.position, host_entry=case["host"], misalign=case["misalign"])
    try:
        calls = [acc.route_dense(index, c["queries"], c["rep_limit"], c["mask"], host_entry=c["host"], misalign=c["misalign"])[:3] for c in case["calls"]]
        return {"norms": index.norms, "calls": calls}
    finally:
        index.close()


def differs(got, want):
    bad = []
    if not ro.same_bits(got["norms"], want["norms"]):
        bad.append("norms")
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        if not ro.same_bits(g[0], w[0]):
            bad.append("dense[%d]" % i)
        if not np.array_equal(np.asarray(g[1], bool), w[1]):
            bad.append("observed[%d]" % i)
        if not np.array_equal(np.asarray(g[2], np.uint32), w[2]):
            bad.append("evals[%d]" % i)
    return bad


def self_test():
    case = draw(4)
    want = oracle(case)
    copy = lambda: {"norms": want["norms"].copy(), "calls": [tuple(a.copy() for a in c) for c in want["calls"]]}  # noqa: E731
    assert differs(copy(), want) == []
    got = copy()
    got["norms"].view(np.uint32)[got["norms"].size // 2] ^= 1
    assert differs(got, want) == ["norms"]
    for part, name in ((0, "dense[0]"), (1, "observed[0]"), (2, "evals[0]")):
        got = copy()
        a = got["calls"][0][part].reshape(-1)
        if a.dtype == bool:
            a[a.size // 2] ^= True
        else:
            a.view(np.uint32)[a.size // 2] ^= 1
        assert differs(got, want) == [name], name
    print("self-test OK")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=60)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--self-test", action="store_true")
    a = ap.parse_args()
    if a.self_test:
        return self_test()
    cases = [draw(a.seed * 1000 + i) for i in range(a.cases)]
    if a.dry_run:
        wants = [oracle(c) for c in cases[:8]]
        assert all(len(w["calls"]) >= 1 for w in wants)
        calls = [c for case in cases for c in case["calls"]]
        assert {c["host"] for c in calls} == {False, True} and {c["mask"] is None for c in calls} == {False, True}
        assert {c["queries"].shape[0] <= 8 for c in calls} == {False, True} and {case["host"] for case in cases} == {False, True}
        print(f"dry run OK: {len(cases)} cases drawn, dims {sorted({c['dim'] for c in cases})}, {len(calls)} calls")
        return
    import torch
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    failed = 0
    for case in cases:
        bad = differs(device(acc, case), oracle(case))
        if bad:
            failed += 1
            print("FAIL seed", case["seed"], "dim", case["dim"], "host", case["host"], bad)
    acc.close()
    print(f"{len(cases)} cases, {failed} failures" + (" OK" if not failed else ""))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
