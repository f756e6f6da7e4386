"""Stress of the topology build's input features on the device (yams_features_aggregate / _variance / _compose) against
tests/_features_oracle.py: seeded cases on ONE context, each one of the three entries on a random shape from the lattice of
tests/test_features_gpu.py (mixed exponents, signed zeros, a few non-finite values), with or without a select list / weights /
either part, in either variance form, through the device or the host entry, aligned or not; every comparison on bits, of
every output element.

    python tests/stress_features.py [--cases 60] [--seed 1]
    python tests/stress_features.py --dry-run      draws the cases and computes their oracle, no device
    python tests/stress_features.py --self-test    the comparison tells a flipped bit, no device
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _features_oracle as fo  # noqa: E402

DIMS = [1, 3, 4, 5, 63, 64, 65, 257, 1024]
ROWS = [1, 2, 17, 255, 256, 257, 600]
KINDS = ["aggregate", "variance", "compose"]


def specials(rng, x, share=0.02):
    """Signed zeros and, rarely, a non-finite value: served as IEEE gives them."""
    flat = x.reshape(-1)
    if flat.size:
        k = max(1, int(flat.size * share))
        flat[rng.integers(0, flat.size, k)] = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, np.inf, np.nan, 1e-42, 3e38], np.float32), k)
    return x


def draw(seed):
    rng = np.random.default_rng(seed)
    kind = KINDS[seed % 3]
    dim, n = int(rng.choice(DIMS)), int(rng.choice(ROWS))
    if n > 300 and dim > 257:
        dim = 257
    case = {"seed": seed, "kind": kind, "host": bool(rng.random() < 0.3), "misalign": 4 if rng.random() < 0.3 else 0}
    x = fo.mixed(rng, (n, dim), -6, 6)
    if rng.random() < 0.5:
        x = specials(rng, x)
    case["x"] = x
    if kind == "aggregate":
        n_docs = int(rng.choice([1, 2, 40, 300]))
        lengths = rng.choice([0, 1, 2, 3, 17], n_docs)
        case["off"] = fo.csr(lengths)
        case["records"] = rng.integers(0, n, int(lengths.sum())).astype(np.uint32)
    elif kind == "variance":
        case["select"] = rng.integers(0, n, int(rng.choice([1, 2, 9, n + 5]))).astype(np.uint32) if rng.random() < 0.5 else None
        case["form"] = int(rng.integers(0, 2))
    else:
        case["weights"] = None
        if rng.random() < 0.5:
            w = np.abs(fo.mixed(rng, dim, -3, 3))
            w[rng.random(dim) < 0.5] = 0.0
            case["weights"] = w
        k = int(rng.choice([1, 3, 16]))
        sl, sd = int(rng.choice([1, 7, 256])), int(rng.choice([1, 7, 64]))
        case["entity"] = fo.mixed(rng, (n, k), -2, 2) if rng.random() < 0.7 else None
        case["sig"] = rng.integers(0, 1 << 32, (n, sl), dtype=np.uint64).astype(np.uint32) if rng.random() < 0.7 else None
        case["entity_on"] = (rng.random(n) < 0.5).astype(np.uint8)
        case["sketch_on"] = (rng.random(n) < 0.5).astype(np.uint8)
        case["sketch_dim"] = sd
        case["alpha"] = (float(rng.choice([0.25, 0.75, np.nan, 0.0])), float(rng.choice([0.125, 0.5, 0.0])))
        case["pad"] = int(rng.choice([0, 0, 5]))
    return case


def _compose_args(c):
    return (c["x"], c["weights"], c["entity"], c["entity_on"], c["sig"], c["sketch_on"], c["sketch_dim"], c["alpha"][0], c["alpha"][1])


def _stride(c):
    k = 0 if c["entity"] is None else c["entity"].shape[1]
    sl = 0 if c["sig"] is None else c["sig"].shape[1]
    return fo.longest_row(c["x"].shape[1], c["weights"], c["entity"], k, c["sig"], sl, c["sketch_dim"]) + c["pad"]


def oracle(c):
    if c["kind"] == "aggregate":
        return fo.aggregate_cpp(c["x"], c["off"], c["records"])
    if c["kind"] == "variance":
        return fo.variance_cpp(c["x"], c["select"], c["form"])
    return fo.compose_cpp(*_compose_args(c), out_stride=_stride(c))


def device(acc, c):
    kw = dict(host_entry=c["host"], misalign=c["misalign"])
    if c["kind"] == "aggregate":
        return acc.features_aggregate(c["x"], c["off"], c["records"], **kw)
    if c["kind"] == "variance":
        return acc.features_variance(c["x"], select=c["select"], form=c["form"], **kw)
    x, w, ent, eon, sig, son, sd, ae, am = _compose_args(c)
    return acc.features_compose(x, w, ent, eon, sig, son, sd, ae, am, out_stride=_stride(c), **kw)


def differs(got, want):
    """The outputs whose bits differ (a NaN the arithmetic made may be any NaN; one that was only copied keeps its bits —
    the aggregate of a single record — which the GPU tests pin; here NaNs are compared as NaNs)."""
    bad = []
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append(i)
            continue
        if g.dtype.kind == "f":
            u = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
            same = (g.view(u) == w.view(u)) | (np.isnan(g) & np.isnan(w))
        else:
            same = g == w
        if not same.all():
            bad.append(i)
    return bad


def self_test():
    for seed in (1000, 1001, 1002):
        c = draw(seed)
        want = oracle(c)
        copy = [np.array(v, copy=True) for v in want]
        assert differs(copy, want) == []
        for i in range(len(want)):
            got = [np.array(v, copy=True) for v in want]
            flat = got[i].reshape(-1)
            if flat.size == 0:
                continue
            at = int(np.flatnonzero(~np.isnan(flat.astype(np.float64)))[0])
            flat.view({4: np.uint32, 8: np.uint64}[flat.dtype.itemsize])[at] ^= 1
            assert differs(got, want) == [i], (seed, i)
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
        for c in cases[:9]:
            oracle(c)
        assert {c["kind"] for c in cases} == set(KINDS) and {c["host"] for c in cases} == {False, True}
        assert {c["form"] for c in cases if c["kind"] == "variance"} == {0, 1}
        assert {c["weights"] is None for c in cases if c["kind"] == "compose"} == {False, True}
        print(f"dry run OK: {len(cases)} cases drawn, rows {sorted({len(c['x']) for c in cases})}, dims {sorted({c['x'].shape[1] for c in cases})}")
        return
    import torch
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    failed = 0
    for c in cases:
        bad = differs(device(acc, c), oracle(c))
        if bad:
            failed += 1
            print("FAIL seed", c["seed"], c["kind"], c["x"].shape, "host", c["host"], "misalign", c["misalign"], "outputs", bad)
    acc.close()
    print(f"{len(cases)} cases, {failed} failures" + (" OK" if not failed else ""))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
