"""Stress of computePersistenceH0 on the device against tests/_persistence_oracle.py: seeded cases on ONE context over the
lattice of point counts and dimensions of tests/test_persistence_gpu.py, each a random cloud (mixed exponents, an integer
lattice, duplicated points or separated clusters), with or without a select list (reordered, with repeats), in either chain
form, through the device or the host entry, aligned or not; every comparison on bits, of every output.

    python tests/stress_persistence.py [--cases 60] [--seed 1]
    python tests/stress_persistence.py --dry-run      draws the cases and computes their oracle, no device
    python tests/stress_persistence.py --self-test    the comparison tells a flipped bit, no device
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _persistence_oracle as po  # noqa: E402

POINTS = [1, 2, 3, 5, 17, 63, 64, 65, 127, 128, 129, 193, 257, 400, 1023, 1024, 1025]
DIMS = [1, 2, 3, 7, 8, 9, 16, 33, 100, 768]
KINDS = ["mixed", "lattice", "duplicates", "clusters"]


def draw(seed):
    rng = np.random.default_rng(seed)
    m, dim, kind = int(rng.choice(POINTS)), int(rng.choice(DIMS)), str(rng.choice(KINDS))
    if m > 300 and dim > 33:
        dim = 33                                     # (keeps the oracle of a case well under a second)
    if kind == "mixed":
        x = po.mixed_points(seed, m, dim)
    elif kind == "lattice":
        x = po.lattice_points(seed, m, dim, side=int(rng.integers(2, 6)))
    elif kind == "duplicates":
        others = int(rng.integers(0, max(m // 4, 1) + 1))
        x = po.duplicated_points(seed, max(m - others, 1), others, dim)[:m]
    else:
        k = int(rng.integers(1, 6))
        x = po.cluster_points(seed, k, (m + k - 1) // k, dim)[:m]
    select = None
    if rng.random() < 0.4:
        select = rng.integers(0, len(x), int(rng.choice([1, 2, 3, len(x), len(x) + 7]))).astype(np.uint32)
    return {"seed": seed, "kind": kind, "x": np.ascontiguousarray(x, np.float32), "select": select, "form": int(rng.integers(0, 2)),
            "host": bool(rng.random() < 0.3), "misalign": 4 if rng.random() < 0.3 else 0}


def oracle(case):
    x = case["x"] if case["select"] is None else case["x"][case["select"].astype(np.int64)]
    return po.persistence_cpp(x, case["form"])


def device(acc, case):
    return acc.persistence_h0(case["x"], select=case["select"], form=case["form"], host_entry=case["host"], want_distances=True,
                              want_weights=True, misalign=case["misalign"])


def differs(got, want):
    bad = [k for k in ("norm_index", "n_edges", "n_points", "n_merges") if int(got[k]) != int(want[k])]
    bad += [k for k in ("norm", "value") if po.hex64(got[k]) != po.hex64(want[k])]
    bad += [k for k in ("distances", "weights") if got[k].shape != want[k].shape or not (po.bits64(got[k]) == po.bits64(want[k])).all()]
    return bad


def self_test():
    case = draw(1003)
    want = oracle(case)
    assert want["n_points"] >= 3
    copy = lambda: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}  # noqa: E731
    assert differs(copy(), want) == []
    for k in ("distances", "weights"):
        got = copy()
        got[k].reshape(-1).view(np.uint64)[got[k].size // 2] ^= 1
        assert differs(got, want) == [k], k
    for k in ("norm", "value"):
        got = copy()
        got[k] = float((np.float64(want[k]).view(np.uint64) ^ np.uint64(1)).view(np.float64))
        assert differs(got, want) == [k], k
    got = copy()
    got["norm_index"] += 1
    assert differs(got, want) == ["norm_index"]
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
        assert all(w["n_points"] == (len(c["x"]) if c["select"] is None else len(c["select"])) for w, c in zip(wants, cases))
        assert {c["host"] for c in cases} == {False, True} and {c["form"] for c in cases} == {0, 1}
        assert {c["select"] is None for c in cases} == {False, True} and {c["kind"] for c in cases} == set(KINDS)
        print(f"dry run OK: {len(cases)} cases drawn, points {sorted({len(c['x']) for c in cases})}, dims {sorted({c['x'].shape[1] for c in cases})}")
        return
    import torch
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    failed = 0
    for case in cases:
        bad = differs(device(acc, case), oracle(case))
        if bad:
            failed += 1
            print("FAIL seed", case["seed"], case["kind"], case["x"].shape, "form", case["form"], "host", case["host"], bad)
    acc.close()
    print(f"{len(cases)} cases, {failed} failures" + (" OK" if not failed else ""))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
