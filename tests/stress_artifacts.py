"""Stress of the cluster artifacts against tests/_artifacts_oracle.py: seeded cases on ONE context, each a random shape
through centroids -> representatives -> residuals (dense or lists, either form, device or host entry, aligned or not), every
comparison on bits.

    python tests/stress_artifacts.py [--cases 60] [--seed 1]
    python tests/stress_artifacts.py --dry-run      draws the cases and computes their oracle, no device
    python tests/stress_artifacts.py --self-test    the comparison tells a flipped bit, no device
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _artifacts_oracle as ao  # noqa: E402

DIMS = [1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 33, 64, 100, 257]


def draw(seed):
    rng = np.random.default_rng(seed)
    form = int(rng.integers(0, 2))
    # the FUSED restatement is exact integer arithmetic, one Python call per multiply-add: those cases stay small (the wide and
    # many-cluster shapes come with SEPARATE here, and with both forms in tests/test_artifacts_gpu.py)
    small = form == ao.FUSED
    dim = int(rng.choice(DIMS[:9] if small else DIMS))
    c = int(rng.integers(1, 8)) if (small or rng.random() < 0.7) else int(rng.integers(60, 72))
    sizes = [int(rng.choice([0, 1, 2, 5, 63, 64, 65, 130])) if (not small and rng.random() < 0.5) else int(rng.integers(0, 12)) for _ in range(c)]
    if sum(sizes) == 0:
        sizes[0] = 3
    x, off, mem = ao.clustered_case(seed * 7 + 1, sizes, dim, order=str(rng.choice(["scrambled", "descending", "ascending"])))
    n = len(x)
    pri = np.full(n, ao.NONE, np.uint32)
    for k in range(c):
        pri[mem[int(off[k]):int(off[k + 1])].astype(np.int64)] = k
    pri[rng.random(n) < 0.05] = ao.NONE
    lists = bool(rng.random() < 0.5)
    coff = cand = None
    if lists:
        lens = rng.integers(0, 9 if small else 33, n)
        coff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        cand = rng.integers(0, c, int(coff[-1])).astype(np.uint32)
    return {"seed": seed, "dim": dim, "x": x, "off": off, "mem": mem, "n_extra": int(rng.choice([1, 2, 3, 4, 64])), "pri": pri if rng.random() < 0.8 else None,
            "coff": coff, "cand": cand, "form": form, "host": bool(rng.random() < 0.3), "misalign": 4 if rng.random() < 0.3 else 0}


def oracle(case):
    cent, cnt = ao.centroids(case["x"], case["off"], case["mem"])
    sel, scnt = ao.representatives(case["x"], case["off"], case["mem"], cent, case["n_extra"])
    pn, cn, rd = ao.residuals(case["x"], cent, case["pri"], case["coff"], case["cand"], case["form"])
    return {"centroids": cent, "counts": cnt, "selected": sel, "selected_counts": scnt, "primary_norm_sq": pn, "cand_norm_sq": cn, "residual_dot": rd}


def device(acc, case, cent):
    kw = {"host_entry": case["host"], "misalign": case["misalign"]}
    c2, cnt = acc.cluster_centroids(case["x"], case["off"], case["mem"], **kw)
    sel, scnt = acc.cluster_representatives(case["x"], case["off"], case["mem"], cent, case["n_extra"], **kw)
    pn, cn, rd = acc.cluster_residuals(case["x"], cent, case["pri"], case["coff"], case["cand"], form=case["form"], **kw)
    return {"centroids": c2, "counts": cnt, "selected": sel, "selected_counts": scnt, "primary_norm_sq": pn, "cand_norm_sq": cn, "residual_dot": rd}


def differs(case, got, want):
    bad = []
    for key, w in want.items():
        g = got[key]
        if w is None or g is None:
            if (w is None) != (g is None):
                bad.append(key)
            continue
        if key == "residual_dot":      # undefined for a document without a primary
            n, c = len(case["x"]), len(case["off"]) - 1
            doc = np.repeat(np.arange(n), c) if case["coff"] is None else np.repeat(np.arange(n), np.diff(case["coff"].astype(np.int64)))
            keep = case["pri"][doc] != ao.NONE
            g, w = g[keep], w[keep]
        ok = ao.same_bits(g, w) if w.dtype.kind == "f" else np.array_equal(g, w)
        if not ok:
            bad.append(key)
    return bad


def self_test():
    case = draw(3)
    want = oracle(case)
    assert differs(case, {k: (None if v is None else v.copy()) for k, v in want.items()}, want) == []
    for key in ("centroids", "cand_norm_sq", "selected"):
        got = {k: (None if v is None else v.copy()) for k, v in want.items()}
        flat = got[key].reshape(-1).view(np.uint32 if got[key].dtype.itemsize == 4 else np.uint64)
        flat[flat.size // 2] ^= 1
        assert differs(case, got, want) == [key], key
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
        assert all(w["cand_norm_sq"] is not None for w in wants)
        assert {c["form"] for c in cases} == {0, 1} and {c["host"] for c in cases} == {False, True} and {c["coff"] is None for c in cases} == {False, True}
        print(f"dry run OK: {len(cases)} cases drawn, dims {sorted({c['dim'] for c in cases})}")
        return
    import torch
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)
    failed = 0
    for case in cases:
        want = oracle(case)
        bad = differs(case, device(acc, case, want["centroids"]), want)
        if bad:
            failed += 1
            print("FAIL seed", case["seed"], "dim", case["dim"], "host", case["host"], "form", case["form"], bad)
    acc.close()
    print(f"{len(cases)} cases, {failed} failures" + (" OK" if not failed else ""))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
