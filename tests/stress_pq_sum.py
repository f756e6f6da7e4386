"""Randomised stress of the ADC sum orders (YAMS_PQ_SUM_*: lanes | combine | tail) of yams_scan_pq_topk_device against the numpy
restatement (tests/_pq_sum.py): seeded cases on ONE context — a random definition out of the 25, m from 7 to 128 on both sides
of the table-group boundaries of both ADC kernels, index sizes on both sides of the filtered form's switch (65 536), 1 to 9
queries, with and without a candidate list, tie keys and row maps.  Every case is built so that the order of the additions
decides which rows come back (_pq_sum.make_case); a case whose expected rows under the drawn definition do NOT differ from
those under every other function (_pq_sum.discriminates) is still compared but not counted.

    python tests/stress_pq_sum.py [--cases 100] [--seed 5] [--time-limit 240]
    python tests/stress_pq_sum.py --dry-run      # no GPU: draws the cases and counts the ones that discriminate
    python tests/stress_pq_sum.py --self-test    # no GPU: the harness's own comparison and the restatement's pruning

Rows, score bits and counts of every query must be identical.  Prints one JSON line; exit status 1 on a mismatch, on more
than --max-blind cases that do not discriminate, or when the time limit ends the run early.
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _pq_sum as S

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=100)
ap.add_argument("--seed", type=int, default=5)
ap.add_argument("--time-limit", type=float, default=240.0)
ap.add_argument("--max-blind", type=int, default=10)
ap.add_argument("--dry-run", action="store_true")
ap.add_argument("--self-test", action="store_true")
a = ap.parse_args()

M_CHOICES = [7, 8, 12, 16, 20, 24, 31, 32, 33, 36, 37, 40, 48, 64, 65, 72, 73, 100, 127, 128]
FILTER_MIN = 65536


def draw_case(seed, i):
    """Case i of the stream `seed`: (case, flags)."""
    rng = np.random.default_rng([seed, i])
    flags = int(rng.choice(S.definitions()))
    m = int(rng.choice(M_CHOICES))
    big = i % 3 == 0                                       # a third of the cases take the filtered form
    n = int(rng.integers(FILTER_MIN, 80_000)) if big else int(rng.integers(600, 6_000))
    if rng.random() < 0.15:
        n = int(rng.choice([FILTER_MIN - 1, FILTER_MIN, FILTER_MIN + 1]))
    nq = int(rng.integers(1, 10))
    family = int(rng.integers(120, 400))
    rf = int(rng.integers(1, 4))
    approx = int(rng.integers(family // 4, 3 * family // 4))     # the cut runs through the family
    k = max(1, approx // rf)
    n_cand = None
    if rng.random() < 0.4:                                   # a candidate list: sparse, or long enough for the filtered form
        lo = FILTER_MIN if (n > FILTER_MIN + 1000 and rng.random() < 0.5) else family + 50
        n_cand = int(rng.integers(lo, n))
    case = S.make_case(int(rng.integers(1 << 30)), m, n, family, nq, k, rf, with_maps=bool(rng.random() < 0.5), n_cand=n_cand)
    return case, flags


def compare(case, flags, rows, scores, counts):
    """None, or what differs first between a result and the restatement's."""
    for qi, (e_rows, e_sims) in enumerate(S.expected(case, flags)):
        cnt = int(counts[qi])
        if cnt != len(e_rows):
            return {"query": qi, "why": "count %d != %d" % (cnt, len(e_rows))}
        if [int(x) for x in rows[qi][:cnt]] != e_rows:
            return {"query": qi, "why": "rows"}
        if not np.array_equal(np.asarray(scores[qi][:cnt], np.float32).view(np.uint32), np.array(e_sims, np.float32).view(np.uint32)):
            return {"query": qi, "why": "score bits"}
    return None


def describe(case, flags, i):
    return {"case": i, "order": S.name(flags), "m": case.m, "n": case.n, "nq": case.nq, "k": case.k, "rf": case.rf, "family": case.family,
            "cand": None if case.cand is None else int(case.cand.size), "maps": case.keys is not None}


if a.self_test:
    # 1. the pruning of the restatement changes no expected result; 2. compare() accepts the restatement's own answer and
    # refuses the answer of another function (rows), one row count, one score bit
    fails = []
    for i in range(6):
        case, flags = draw_case(77, 3 * i + 1)            # (small cases: the unpruned pipeline is the slow one)
        full = S.expected(case, flags, prune=False)
        case._vals = {}
        if [r for r, _ in S.expected(case, flags)] != [r for r, _ in full]:
            fails.append(("prune", i))
        pad = lambda e: (np.array([r + [-1] * (case.k - len(r)) for r, _ in e], np.int64),
                         np.array([list(s) + [0.0] * (case.k - len(s)) for _, s in e], np.float32), np.array([len(r) for r, _ in e]))
        rows, scores, counts = pad(full)
        if compare(case, flags, rows, scores, counts) is not None:
            fails.append(("own answer refused", i))
        other = next(c[0] for c in S.classes(case.m) if S.tree(c[0], case.m) != S.tree(flags, case.m))
        if S.discriminates(case, flags) and compare(case, flags, *pad(S.expected(case, other))) is None:
            fails.append(("another order accepted", i))
        if counts[0] > 0:
            c2 = counts.copy(); c2[0] -= 1
            s2 = scores.copy(); s2.view(np.uint32)[0, 0] ^= 1
            if compare(case, flags, rows, scores, c2) is None or compare(case, flags, rows, s2, counts) is None:
                fails.append(("count or score bit accepted", i))
    print(json.dumps({"self_test": "ok" if not fails else "failed", "fails": fails}))
    sys.exit(1 if fails else 0)

if not a.dry_run:
    import torch
    from yams_amd.accel import Accel
    acc = Accel(0, torch.cuda.current_stream().cuda_stream)

t0 = time.time()
bad, counted, blind, ran, filtered, unfiltered, orders = [], 0, [], 0, 0, 0, set()
timed_out = False
for i in range(a.cases):
    if time.time() - t0 > a.time_limit:
        timed_out = True
        break
    case, flags = draw_case(a.seed, i)
    sees = S.discriminates(case, flags)
    if not sees:
        blind.append(i)
    if not a.dry_run:
        d_rows = acc.to_device(case.corpus)
        bufs = [d_rows]
        tie_p = inv_p = None
        if case.rank is not None:
            inv = np.empty_like(case.rank); inv[case.rank] = np.arange(case.rank.size, dtype=np.uint32)
            bufs += [acc.to_device(case.rank), acc.to_device(inv)]
            tie_p, inv_p = bufs[1].ptr, bufs[2].ptr
        try:
            v = acc.corpus_view(d_rows.ptr, case.corpus.shape[0], case.dim, tie_rank_ptr=tie_p, rank_row_ptr=inv_p)
            r = acc.scan_pq_topk(v, case.codes, case.luts, case.queries, case.k, case.thr, case.rf, tie_keys=case.keys,
                                 row_of_index=case.roi, candidates=case.cand, sum_flags=flags)
        except Exception as e:                               # every drawn call is a valid one
            bad.append(dict(describe(case, flags, i), error=str(e)[:200]))
            break                                            # (nothing more is started on the device after a failed call)
        finally:
            for b in bufs:
                b.free()
        why = compare(case, flags, r.rows, r.scores, r.counts)
        if why:
            bad.append(dict(describe(case, flags, i), **why))
            break
        n_items = case.n if case.cand is None else case.cand.size
        filtered += n_items >= FILTER_MIN
        unfiltered += n_items < FILTER_MIN
    ran += 1
    counted += sees
    orders.add(S.name(flags))
res = {"cases": a.cases, "ran": ran, "counted": counted, "blind": blind, "mismatches": len(bad), "filtered_calls": filtered,
       "unfiltered_calls": unfiltered, "orders": len(orders), "dry_run": a.dry_run, "timed_out": timed_out,
       "seconds": round(time.time() - t0, 1), "first_bad": bad[:1]}
print(json.dumps(res))
sys.exit(1 if bad or timed_out or len(blind) > a.max_blind or ran != a.cases else 0)
