"""Seeded stress of the SMALL scan (n <= 16384 rows, <= 16 queries: the fused one-launch kernel and the general path
where its rule steps aside) against the CPU oracle ALONE: nothing of the device is its own authority here.

All cases run on ONE context, in sequence: the workspace (the survivor keys, the ticket counters) carries whatever
the previous case left behind; a large dense case is followed by a small sparse one on purpose.  Every query of every
case goes through _score_edges.compare against oracle.scan_cosine / scan_cosine_records / scan_l2 (scan_l2_f32acc for the
fp32-accumulate flags, which route off the fused path).  Whether the fused launch answered (the context's timed region
"small_scan") and diag.path must be what the rule stated at yams_scan_diag_t.path says.  No case and no query is skipped
or sampled.  The harness stops at the first failing case, prints one JSON line with its draw, and
never retries.

    python tests/stress_small.py [--cases N] [--seed S]     on the GPU
    python tests/stress_small.py --dry-run                  draws + oracle only: reports the path counters
    python tests/stress_small.py --self-test                compare() must report each mutated oracle answer
"""
import argparse, json, math, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

import _oracle
import _score_edges as se
from _score_edges import SCAN_COSINE, SCAN_L2, FLAG_DEFER_THRESHOLD, FLAG_RECORD_PATH

DEFAULT_SEED, DEFAULT_CASES = 3, 200
FLAG_L2_ACC_F32, FLAG_L2_ACC_F32X8, FLAG_L2_ACC_F32X16, FLAG_L2_ACC_FUSED = 256, 512, 768, 2048
ACC_LANES = {FLAG_L2_ACC_F32: 1, FLAG_L2_ACC_F32X8: 8, FLAG_L2_ACC_F32X16: 16}

N_EDGE = [1, 2, 63, 64, 65, 255, 256, 257, 513, 4095, 4096, 4097, 16383, 16384]
DIMS = [32, 64, 96, 128, 160, 384, 768, 1024]          # 1, 2, 3, 4, 5, 12, 24, 32 chunks of 32: every residue mod 4
NQS = [1, 2, 3, 4, 5, 8, 15, 16]
KS = [1, 2, 15, 16, 17, 63, 64, 65, 100, 255, 256]
THRESHOLDS = [-1.0, -0.0, 0.0, 0.1, se.DENORM_MIN]
DUP_LABELS = ["2", "kk-1", "kk", "kk+1", "65", "257", "1100"]
MASK_KINDS = ["none", "dense", "sparse", "one", "empty"]
# (k, workgroups) whose survivor product ceil(n / 256) * min(k, 256) is exactly 1024, and one workgroup above the limit
SURV_EXACT = [(256, 4), (64, 16), (16, 64)]
SURV_OVER = [(256, 5), (255, 5), (100, 11), (65, 16), (64, 17), (63, 17), (17, 61)]
FLT_MAX_4 = np.float32(np.finfo(np.float32).max / 4)


def dup_width(label, kk):
    named = {"2": 2, "kk-1": kk - 1, "kk": kk, "kk+1": kk + 1}
    return named[label] if label in named else int(label)


def draw_case(rng, i, prev):
    """The draw of case i: plain numbers and strings (the JSON line of a failure is this dict)."""
    slot = i % 12
    d = {"case": i, "seed": int(rng.integers(1, 1 << 30))}
    d["n"] = int(rng.choice(N_EDGE)) if rng.random() < 0.5 else int(math.exp(rng.uniform(0.0, math.log(16384.0))))
    d["dim"] = int(rng.choice(DIMS)); d["nq"] = int(rng.choice(NQS)); d["k"] = int(rng.choice(KS))
    # (a zero plateau is a cosine matter; most of its cases keep the whole plateau in play: no mask, a threshold <= 0)
    d["content"] = str(rng.choice(["philox", "dup", "zero", "invalid"], p=[0.25, 0.35, 0.25, 0.15]))
    zero = d["content"] == "zero"
    d["metric"] = SCAN_L2 if (rng.random() < 0.3 and not zero) else SCAN_COSINE
    d["tie"] = bool(rng.random() < 0.5)
    d["mask"] = str(rng.choice(MASK_KINDS, p=[0.7, 0.1, 0.1, 0.05, 0.05] if zero else [0.4, 0.2, 0.2, 0.1, 0.1]))
    d["thr"] = float(rng.choice(THRESHOLDS[:3] + THRESHOLDS[:3] + THRESHOLDS if zero else THRESHOLDS))
    d["row_base"] = int(rng.choice([0, 1000, 1 << 33]))
    d["stripes"] = [int(rng.choice([64, 100, 4096])), int(rng.integers(2, 5))] if rng.random() < 0.25 else None
    if d["stripes"]:
        d["stripes"].append(int(rng.integers(0, d["stripes"][1])))
    d["sched"] = None
    if slot == 5:                      # survivor product exactly 1024: the fused path at its limit
        k, wg = SURV_EXACT[int(rng.integers(0, len(SURV_EXACT)))]
        d.update(k=k, n=wg * 256 - int(rng.integers(0, 256)), sched="survivors_1024")
    elif slot == 6:                    # one workgroup above it: the general path answers
        k, wg = SURV_OVER[int(rng.integers(0, len(SURV_OVER)))]
        d.update(k=k, n=wg * 256 - int(rng.integers(0, 256)), sched="survivors_over")
    elif slot == 10:                   # a large dense case ...
        d.update(n=int(rng.choice([16384, 16383, 16000])), k=int(rng.choice([16, 15, 2])), nq=int(rng.choice([4, 5, 16])),
                 mask="none", content="dup", sched="large_dense")
    elif slot == 11 and prev is not None:   # ... then a small sparse one with the same queries' slots: stale keys would show
        d.update(n=int(rng.choice([65, 257, 513, 700])), k=prev["k"], nq=prev["nq"], metric=prev["metric"], dim=prev["dim"],
                 mask=str(rng.choice(["sparse", "one"])), content="philox", sched="small_sparse_after_large")
    flags = 0
    if d["metric"] == SCAN_L2:
        if rng.random() < 0.25:        # fp32 accumulation: off the fused path
            flags |= int(rng.choice([FLAG_L2_ACC_F32, FLAG_L2_ACC_F32X8, FLAG_L2_ACC_F32X16]))
            if rng.random() < 0.5:
                flags |= FLAG_L2_ACC_FUSED
        if rng.random() < 0.3:
            flags |= FLAG_DEFER_THRESHOLD
    elif rng.random() < 0.25:
        flags |= FLAG_RECORD_PATH
    if d["sched"] in ("survivors_1024", "large_dense", "small_sparse_after_large"):
        flags &= ~(FLAG_L2_ACC_F32X16 | FLAG_L2_ACC_FUSED)    # these are cases OF the fused path
    d["flags"] = flags
    n, k, nq, dim = d["n"], d["k"], d["nq"], d["dim"]
    kk = min(k, 256)
    # content that does not fit the shape falls back to plain Philox rows
    if d["content"] == "zero" and not (k >= 3 and n >= k + 3 and dim >= 2 * nq + 1):
        d["content"] = "philox"
    if d["content"] == "zero":
        P = int(rng.integers(0, k - 1))                                  # P <= k - 2
        Z = k - P + 2 + int(rng.integers(0, min(n - k - 2, 300) + 1))    # Z >= k - P + 2, P + Z <= n
        d["P"], d["Z"] = P, Z
    if d["content"] == "dup":
        fit = [l for l in DUP_LABELS if 1 <= dup_width(l, kk) <= max(n - 8, 0)]
        if fit:
            d["dup"] = str(rng.choice(fit))
        else:
            d["content"] = "philox"
    if d["content"] == "invalid":
        d["valid"] = int(rng.integers(0, min(k, n)))                      # fewer than k rows score at all
    return d


def build_case(o, d):
    """(corpus, queries, tie_rank | None, allowed | None) of a draw: everything follows from the draw's numbers."""
    n, dim, nq, k = d["n"], d["dim"], d["nq"], d["k"]
    rng = np.random.default_rng(d["seed"])
    tie = rng.permutation(n).astype(np.uint32) if d["tie"] else None
    if d["content"] == "zero":
        z = se.zero_plateau(d["seed"], n, dim, nq, k, d["P"], d["Z"])
        corpus, q, tie = z["corpus"], z["queries"], z["tie_rank"]        # (the plateau's ranks are the point: always ranked)
    else:
        corpus = o.synth_rows(d["seed"], 0, n, dim) * np.float32(rng.choice([0.25, 1.0, 3.0]))
        q = o.synth_rows(d["seed"], 1 << 40, nq, dim)
        free = rng.permutation(n)
        if d["content"] == "invalid":
            valid = free[:d["valid"]]
            keep = corpus[valid].copy()
            kinds = rng.integers(0, 3, n)
            corpus[kinds == 0] = 0.0                                      # zero rows: skipped by cosine
            corpus[kinds == 1, 0] = np.nan                                # NaN rows: skipped everywhere
            corpus[kinds == 2] = 0.0; corpus[kinds == 2, dim - 1] = np.float32(5e-7)   # norm^2 2.5e-13 <= 1e-12
            corpus[valid] = keep
        elif n >= 16:
            h = free[:8]; free = free[8:]
            corpus[h[0]] = 0.0
            corpus[h[1], int(rng.integers(0, dim))] = np.nan
            corpus[h[2], int(rng.integers(0, dim))] = np.inf
            corpus[h[3]] = 0.0; corpus[h[3], 1] = np.float32(5e-7)        # norm^2 2.5e-13: <= 1e-12, skipped
            corpus[h[4]] = 0.0; corpus[h[4], 2] = np.float32(3e-6)        # norm^2 9e-12 in (1e-12, 1e-10): fast path scores it, record path not
            corpus[h[4], 0] = np.float32(1e-9)
            corpus[h[5]] = FLT_MAX_4; corpus[h[5], 1::2] = -FLT_MAX_4     # +-FLT_MAX / 4
            corpus[h[6]] = -q[0]                                          # similarity -1
            corpus[h[7]] = (q[nq - 1] * np.float32(0.5)).astype(np.float32)   # similarity 1 with the last query
        if d["content"] == "dup":
            w = dup_width(d["dup"], min(k, 256))
            rows = np.sort(free[:w])                                      # spread over the workgroups, not consecutive
            corpus[rows] = q[0] * np.float32(1.0)                         # an exact-duplicate plateau at the very top
    allowed = None
    if d["mask"] == "dense":
        allowed = np.flatnonzero(rng.random(n) < rng.uniform(0.3, 0.95))
    elif d["mask"] == "sparse":
        allowed = np.sort(rng.choice(n, max(1, n // 50), replace=False))
    elif d["mask"] == "one":
        allowed = np.array([int(rng.integers(0, n))])
    elif d["mask"] == "empty":
        allowed = np.zeros(0, np.int64)
    return np.ascontiguousarray(corpus, np.float32), np.ascontiguousarray(q, np.float32), tie, allowed


def oracle_answers(o, d, corpus, q, tie, allowed):
    """Per query (rows, sims, dist | None) in the corpus's own row ordinals."""
    k, thr, metric, flags = d["k"], d["thr"], d["metric"], d["flags"]
    n = corpus.shape[0]
    sel = np.arange(n) if allowed is None else np.asarray(allowed, np.int64)
    rank = (np.arange(n) if tie is None else tie).astype(np.uint64)
    out = []
    for qi in range(q.shape[0]):
        if len(sel) == 0:
            out.append((np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.float32) if metric == SCAN_L2 else None))
        elif metric == SCAN_COSINE and (flags & FLAG_RECORD_PATH):
            allow = np.zeros(n, np.uint8); allow[sel] = 1
            r = o.scan_cosine_records(corpus, q[qi], k, thr, rank, allow)
            out.append((r[0], r[1], None))
        elif metric == SCAN_COSINE:
            r = o.scan_cosine(corpus[sel], q[qi], k, thr, rank[sel])
            assert r is not None, "the harness draws valid queries only"
            out.append((sel[r[0]], r[1], None))
        else:
            t = -np.inf if (flags & FLAG_DEFER_THRESHOLD) else thr
            lanes = ACC_LANES.get(flags & se.FLAG_L2_ACC_MASK)
            if lanes:
                r = o.scan_l2_f32acc(corpus[sel], q[qi], k, t, rank[sel], lanes=-lanes if (flags & FLAG_L2_ACC_FUSED) else lanes)
            else:
                r = o.scan_l2(corpus[sel], q[qi], k, t, rank[sel])
            out.append((sel[r[0]], r[2], r[1]))
    return out


def count_paths(paths, d, path, answers, corpus, q, tie, o):
    def hit(name):
        paths[name] = paths.get(name, 0) + 1
    n, k, nq = d["n"], d["k"], d["nq"]
    kk = min(k, 256)
    wg = -(-n // 256)
    hit("fused" if path else "general")
    if path:
        hit("qb1" if nq == 1 else "qb4")
        if nq > 1 and nq % 4:
            hit("ragged_last_chunk")
        hit("one_level" if kk >= 64 else "two_level")
        if wg * kk == 1024:
            hit("survivors_1024")
    elif se.restated_path(n, d["dim"], nq, 1, d["metric"], d["flags"]) and k <= 256 and (wg - 1) * kk <= 1024 < wg * kk:
        hit("survivors_one_workgroup_over")
    hit("mask_" + d["mask"])
    hit("content_" + d["content"])
    if d["content"] == "dup":
        hit("dup_" + d["dup"])
    if d["sched"]:
        hit(d["sched"])
    if d["metric"] == SCAN_L2:
        hit("l2")
    if d["flags"] & FLAG_RECORD_PATH:
        hit("record_path")
    if d["thr"] == 0.0:
        hit("thr_neg_zero" if math.copysign(1.0, d["thr"]) < 0 else "thr_pos_zero")
    if any(len(a[0]) < k for a in answers):
        hit("valid_rows_below_k")
    if d["content"] == "zero" and d["metric"] == SCAN_COSINE and d["mask"] == "none" and not d["thr"] > 0.0:
        # the plateau straddles the cut: zeros of both signs inside the answer, and an order by score bits answers otherwise
        bits = [set(np.asarray(a[1], np.float32).view(np.uint32).tolist()) for a in answers]
        if all({0, 0x80000000} <= b for b in bits):
            hit("zero_plateau_straddles_cut")


def to_arrays(answers, k, metric):
    """An oracle answer in the shape of a device answer (counts, rows, scores, dist), padded as the device pads."""
    nq = len(answers)
    counts = np.array([len(a[0]) for a in answers], np.uint32)
    rows = np.full((nq, k), -1, np.int64); scores = np.full((nq, k), -np.inf, np.float32); dist = np.full((nq, k), np.inf, np.float32)
    for qi, a in enumerate(answers):
        c = len(a[0])
        rows[qi, :c] = a[0]; scores[qi, :c] = a[1]
        dist[qi, :c] = a[2] if metric == SCAN_L2 else np.float32(1.0) - np.asarray(a[1], np.float32)
    return counts, rows, scores, dist


def self_test(o):
    """compare() must let the oracle's own answer pass and report each of the mutations; returns the list of failures."""
    fails = []
    n, dim, nq, k, P, Z = 600, 32, 2, 20, 5, 60
    z = se.zero_plateau(11, n, dim, nq, k, P, Z)
    d = {"k": k, "thr": -1.0, "metric": SCAN_COSINE, "flags": 0}
    ans = oracle_answers(o, d, z["corpus"], z["queries"], z["tie_rank"], None)

    def cmp(counts, rows, scores, dist, answers=ans, kk=k, visited=nq * n):
        return se.compare(counts, rows, scores, dist, visited, answers, kk, SCAN_COSINE, nq * n)

    def expect(name, msg, must_report=True):
        if (msg is not None) != must_report:
            fails.append("%s: %s" % (name, "not reported" if must_report else msg))
    c, r, s, dd = to_arrays(ans, k, SCAN_COSINE)
    expect("the oracle's own answer", cmp(c, r, s, dd), must_report=False)
    # (1) the order by score bits: every +0.0 ahead of every -0.0
    r1, s1 = r.copy(), s.copy()
    for qi in range(nq):
        full = o.scan_cosine(z["corpus"], z["queries"][qi], n, -1.0, z["tie_rank"].astype(np.uint64))
        pr, ps = se.packed_key_order(full[0], full[1], z["tie_rank"][full[0]], k)
        r1[qi], s1[qi] = pr, ps
    expect("packed-key order of a zero plateau", cmp(c, r1, s1, dd))
    # (2) two rows of one score swapped (each keeps its own bits)
    i = next(i for i in range(k - 1) if s[0, i] == s[0, i + 1])
    r2, s2 = r.copy(), s.copy()
    r2[0, [i, i + 1]] = r2[0, [i + 1, i]]; s2[0, [i, i + 1]] = s2[0, [i + 1, i]]
    expect("two equal-score rows swapped", cmp(c, r2, s2, dd))
    # (3) a count off by one, the padding in place
    c3, r3, s3, d3 = c.copy(), r.copy(), s.copy(), dd.copy()
    c3[1] -= 1; r3[1, k - 1] = -1; s3[1, k - 1] = -np.inf; d3[1, k - 1] = np.inf
    expect("count off by one", cmp(c3, r3, s3, d3))
    # (4) wrong padding behind a short count (the smallest denormal as threshold drops the plateau: P rows come back)
    d4 = dict(d, thr=se.DENORM_MIN)
    ans4 = oracle_answers(o, d4, z["corpus"], z["queries"], z["tie_rank"], None)
    c4, r4, s4, dd4 = to_arrays(ans4, k, SCAN_COSINE)
    if not all(len(a[0]) == P for a in ans4):
        fails.append("denormal threshold: the plateau was not dropped")
    expect("short answer, right padding", cmp(c4, r4, s4, dd4, ans4), must_report=False)
    for name, (ri, si, di) in {"rows": (0, None, None), "scores": (None, 0.0, None), "distances": (None, None, 0.0)}.items():
        rr, ss, d5 = r4.copy(), s4.copy(), dd4.copy()
        if ri is not None: rr[0, k - 1] = ri
        if si is not None: ss[0, P] = si
        if di is not None: d5[1, P] = di
        expect("wrong padding of " + name, cmp(c4, rr, ss, d5, ans4))
    # (5) the sign bit of a returned zero flipped
    s6 = s.copy()
    j = int(np.flatnonzero(s6[0] == 0.0)[0])
    s6[0, j] = -s6[0, j]
    expect("sign bit of a returned zero flipped", cmp(c, r, s6, dd))
    expect("rows_visited", cmp(c, r, s, dd, visited=nq * n - 1))
    return fails


def run(cases=DEFAULT_CASES, seed=DEFAULT_SEED, dry_run=False, on_case=None):
    """Returns the summary dict ("mismatches": 0) or, at the first failing case, {"failed": {...}} with its draw."""
    o = _oracle.oracle()
    rng = np.random.default_rng(seed)
    acc = None
    if not dry_run:
        import torch  # noqa: F401  (plumbing: the HIP runtime the library shares)
        from yams_amd.accel import Accel
        acc = Accel(0)
    paths, queries, prev, t0 = {}, 0, None, time.time()
    try:
        for i in range(cases):
            d = draw_case(rng, i, prev)
            prev = d
            corpus, q, tie, allowed = build_case(o, d)
            answers = oracle_answers(o, d, corpus, q, tie, allowed)
            want_path = se.restated_path(d["n"], d["dim"], d["nq"], d["k"], d["metric"], d["flags"])
            count_paths(paths, d, want_path, answers, corpus, q, tie, o)
            if on_case is not None:
                on_case(d, corpus, q, tie, allowed, answers)
            queries += d["nq"]
            if dry_run:
                continue
            msg = device_case(acc, d, corpus, q, tie, allowed, answers, want_path)
            if msg is not None:
                return {"failed": {"case": i, "difference": msg, "draw": d}, "cases_passed": i}
    finally:
        if acc is not None:
            acc.close()
    return {"cases": cases, "queries": queries, "mismatches": 0, "seed": seed, "dry_run": dry_run, "paths": dict(sorted(paths.items())),
            "seconds": round(time.time() - t0, 1)}


def device_case(acc, d, corpus, q, tie, allowed, answers, want_path):
    n, dim = corpus.shape
    bufs = [acc.to_device(corpus)]
    tie_p = inv_p = mask_p = None
    if tie is not None:
        inv = np.empty_like(tie); inv[tie] = np.arange(n, dtype=tie.dtype)
        bufs += [acc.to_device(tie), acc.to_device(inv)]
        tie_p, inv_p = bufs[1].ptr, bufs[2].ptr
    n_allowed = 0
    if allowed is not None:
        words = np.zeros((n + 31) // 32, np.uint32)
        a = np.asarray(allowed, np.int64)
        np.bitwise_or.at(words, a >> 5, (np.uint32(1) << (a & 31).astype(np.uint32)))
        bufs.append(acc.to_device(words)); mask_p = bufs[-1].ptr; n_allowed = len(a)
    sr, ns, si = d["stripes"] or (0, 0, 0)
    base = d["row_base"]
    try:
        view = acc.corpus_view(bufs[0].ptr, n, dim, tie_p, inv_p, base, mask_p, n_allowed, stripe_rows=sr, n_stripes=ns, stripe_index=si)
        acc.enable_timing(True)                        # (clears the context's timed regions: what is there afterwards is this call's)
        r = acc.scan_topk(view, q, d["k"], d["thr"], d["metric"], d["flags"])
        fused = acc.kernel_ms("small_scan")[1]
    finally:
        for b in bufs:
            b.free()
    if fused != want_path:
        return "fused launches %d != %d (the stated rule)" % (fused, want_path)
    want_diag = se.restated_diag_path(n, None if allowed is None else n_allowed, dim, d["nq"], d["k"], d["metric"], d["flags"])
    if r.diag["path"] != want_diag:
        return "diag.path %d != %d (the stated rule)" % (r.diag["path"], want_diag)
    row_map = (lambda x: base + x) if not sr else (lambda x: base + ((x // sr) * ns + si) * sr + x % sr)
    n_eff = n if allowed is None else n_allowed
    return se.compare(r.counts, r.rows, r.scores, r.dist, r.diag["rows_visited"], answers, d["k"], d["metric"], d["nq"] * n_eff, row_map)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=DEFAULT_CASES)
    ap.add_argument("--seed", type=int, default=DEFAULT_SEED)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--self-test", action="store_true")
    a = ap.parse_args()
    if a.self_test:
        fails = self_test(_oracle.oracle())
        print(json.dumps({"self_test_failures": fails}))
        return 1 if fails else 0
    res = run(a.cases, a.seed, a.dry_run)
    print(json.dumps(res))
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
