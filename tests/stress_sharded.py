"""Randomised stress of the sharded search end to end — per-shard search, exchange of the packed records, merge_topk_kernel,
download — through ShardedScan (yams_scan_sharded_topk_host and submit / wait) against the oracle over the WHOLE, unsplit
corpus.  Test infrastructure.

    python tests/stress_sharded.py [--cases 120] [--seed 1] [--dry-run] [--keep-going]

Each case draws 1..8 shards on device 0 and the exchange a one-GPU box can reach (collective="peer", or "rccl" bound to the
stand-in of tests/stub_coll — also with ONE rank), a contiguous split with uneven random cuts (a shard of one row, shards
with fewer rows than k, a shard of zero rows) or a striped one (stripe_rows 64 / 100 / 4096, the last stripe partial, some
shards one stripe short), a dimension of every filter tier (64, 100, 256, 384; from 256 up with int8 shadows, half of them
in the rotated layout, the same on every shard), a few thousand to about 60 000 rows, duplicate rows planted within and
across shards (one query IS a duplicated row, the group often larger than k: a tie group straddling position k), tie ranks
(none, or a corpus-wide permutation passed as rank_of_row with per-shard local rank / inverse tables; under L2 they are
passed and must be ignored), allow-masks cut from one global mask (none, sparse, dense; some shards masked out entirely),
the metric (cosine, or L2 under one of the seven accumulate definitions, the oracle set to the same one), a threshold that
leaves some shards short or empty (cosine) or cuts inside the merged top k (L2), k from {1, 7, 100, 1024} and 1..40 queries.
Every tenth case submits two or three different batches on different lanes before waiting, and waits in reverse order.
Compared: rows, order, score bits, distance bits under L2, counts, every output slot behind a count, and rows_visited as
the sum over the shards.

Once per run, outside the loop: nine shards x k = 1024 is over the merge's limit of 8192 entries — the batch fails with
YAMS_ERR_UNSUPPORTED and the handle serves the next batch.

The harness stops at the first failing case (--keep-going: counts them all) and never retries.  --dry-run draws the cases (and asks the oracle where ties
and thresholds fall) without touching the device: the summary's path counts depend on the generator alone.  The paths
(the GPU test asserts floors on them): see PATHS.
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _oracle

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=120)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--dry-run", action="store_true")
ap.add_argument("--keep-going", action="store_true", help="count the mismatching batches instead of stopping at the first")
a = ap.parse_args()
rng = np.random.default_rng(a.seed)
o = _oracle.oracle()

COSINE, L2 = 0, 1
F32, F32X8, F32X16, FUSED = 256, 512, 768, 2048             # YAMS_SCAN_FLAG_L2_ACC_*
L2_DEFS = [("l2_f64", None, 0), ("l2_f32", 1, F32), ("l2_f32x8", 8, F32X8), ("l2_f32x16", 16, F32X16),
           ("l2_f32_fused", -1, F32 | FUSED), ("l2_f32x8_fused", -8, F32X8 | FUSED), ("l2_f32x16_fused", -16, F32X16 | FUSED)]
I8_ROTATED = 1
PATHS = ["exchange_peer", "exchange_rccl", "exchange_rccl_one_rank", "one_shard", "contiguous", "striped", "stripe_64", "stripe_100",
         "stripe_4096", "shard_of_one_row", "shard_smaller_than_k", "shard_of_zero_rows", "dim_64", "dim_100", "dim_256", "dim_384",
         "i8_plain", "i8_rotated", "tie_none", "tie_ranks", "tie_ranks_under_l2", "mask_none", "mask_sparse", "mask_dense",
         "shard_masked_out", "cosine"] + [d[0] for d in L2_DEFS] + \
        ["cosine_thr_short_lists", "l2_thr_cut_inside", "k_1", "k_7", "k_100", "k_1024", "total_8192", "several_batches_in_flight",
         "tie_group_straddles_k", "cross_shard_duplicates"]


def log_uniform(lo, hi):
    return int(min(hi, np.exp(rng.uniform(np.log(lo), np.log(hi + 1)))))


def draw_case(case):
    c = {"case": case}
    n_shards = c["n_shards"] = int(rng.integers(1, 9))
    c["exchange"] = "rccl" if rng.random() < 0.5 else "peer"
    k = c["k"] = int(rng.choice([1, 7, 100, 1024]))
    if case % 20 == 5:
        n_shards, k = c["n_shards"], c["k"] = 8, 1024                           # pinned: the merge's limit of 8192 entries exactly
    d = c["dim"] = int(rng.choice([64, 100, 256, 384]))
    c["i8_flags"] = I8_ROTATED if d >= 256 and rng.random() < 0.5 else 0
    layout = c["layout"] = "striped" if rng.random() < 0.45 else "contiguous"
    if layout == "striped":
        stripe = c["stripe"] = int(rng.choice([64, 100, 4096]))
        short = int(rng.integers(1, n_shards)) if n_shards > 1 else 0          # shards [short, n_shards) hold one whole stripe fewer
        rounds = 1 if stripe == 4096 else int(rng.integers(1, max(2, 60000 // (stripe * n_shards))))
        if stripe != 4096:
            rounds = max(rounds, 2000 // (stripe * n_shards) + 1)
        n = stripe * (rounds * n_shards + short) + int(rng.integers(1, stripe))   # ... and the last stripe is partial
        t = np.arange(n) // stripe
        parts = [np.flatnonzero(t % n_shards == i) for i in range(n_shards)]
    else:
        n = log_uniform(2000, 60000)
        cuts = np.sort(rng.integers(1, n, n_shards - 1)) if n_shards > 1 else np.zeros(0, np.int64)
        u = rng.random()
        if n_shards > 1 and u < 0.3:
            cuts[0] = 1                                                        # a shard of one row
        elif n_shards > 1 and u < 0.55 and k > 2:
            cuts[0] = int(rng.integers(2, k))                                  # a shard with fewer rows than k
        elif n_shards > 1 and u < 0.7:
            j = int(rng.integers(0, n_shards - 1)); cuts[j] = cuts[j - 1] if j else 0   # a shard of zero rows
        cuts = np.sort(cuts)
        b = [0, *cuts.tolist(), n]
        parts = [np.arange(b[i], b[i + 1]) for i in range(n_shards)]
    c["n"] = n
    corpus = rng.standard_normal((n, d)).astype(np.float32)
    # duplicates: small groups anywhere, and one group the first query is aimed at, often larger than k
    for _ in range(int(rng.integers(2, 10))):
        corpus[rng.choice(n, int(rng.integers(2, 6)), replace=False)] = corpus[int(rng.integers(0, n))]
    group = rng.choice(n, min(n // 2, int(rng.integers(2, 2 * k + 3)), 1500), replace=False)
    corpus[group] = corpus[group[0]]
    metric = c["metric"] = L2 if rng.random() < 0.5 else COSINE
    c["l2_def"] = None
    if metric == L2:                                                           # the seven definitions in turn
        c["l2_def"] = draw_case.l2_cases % 7; draw_case.l2_cases += 1
    batches = int(rng.integers(2, 4)) if case % 10 == 9 else 1
    queries = []
    for bi in range(batches):
        q = rng.standard_normal((int(rng.integers(1, 41)), d)).astype(np.float32)
        q[0] = corpus[group[0]] * (np.float32(1.5) if metric == COSINE else np.float32(1.0))
        if q.shape[0] > 2:
            q[2] = corpus[int(rng.integers(0, n))] + np.float32(1e-3)
        queries.append(q)
    c["nq"] = [q.shape[0] for q in queries]
    rank = rng.permutation(n).astype(np.uint32) if rng.random() < 0.5 else None
    c["ranks"] = rank is not None
    mk = rng.random()
    mask = None
    c["mask"] = "none"
    if mk < 0.25:
        mask = np.zeros(n, bool); mask[rng.choice(n, max(1, int(n * rng.uniform(0.002, 0.03))), replace=False)] = True; c["mask"] = "sparse"
    elif mk < 0.55:
        mask = rng.random(n) < rng.uniform(0.3, 0.95); c["mask"] = "dense"
    c["masked_out"] = 0
    if mask is not None and n_shards > 1 and rng.random() < 0.5:
        for i in rng.choice(n_shards, int(rng.integers(1, max(2, n_shards // 2 + 1))), replace=False):
            mask[parts[int(i)]] = False; c["masked_out"] += 1
        if rng.random() < 0.7:
            mask[group[:max(2, len(group) // 2)]] = True                       # (keep part of the tie group in play)
    allowed = np.flatnonzero(mask) if mask is not None else np.arange(n)
    c["allowed"] = len(allowed)
    # the threshold: from the whole-corpus answer of one query, so that it bites
    c["thr"], c["thr_bites"] = -1.0, False
    if rng.random() < 0.65 and len(allowed):
        qi = int(rng.integers(0, queries[0].shape[0]))
        rows, dist, sims = whole(c, corpus, allowed, rank, queries[0][qi], k, -1.0)
        if len(sims):
            thr = float(sims[int(rng.integers(0, len(sims)))])
            kept = int((~(sims < np.float32(thr))).sum())
            c["thr"] = thr
            c["thr_bites"] = kept < len(sims) if metric == COSINE else 0 < kept < len(sims)
    # does the first query's tie group straddle position k?
    c["straddle"] = False
    if len(allowed) > k:
        rows, dist, sims = whole(c, corpus, allowed, rank, queries[0][0], k + 1, -1.0)
        key = dist if metric == L2 else sims
        c["straddle"] = bool(len(key) == k + 1 and key[k - 1] == key[k])
    owner = np.empty(n, np.int64)
    for i, p in enumerate(parts):
        owner[p] = i
    c["dup_shards"] = int(len(set(owner[group].tolist())))
    return c, corpus, parts, queries, rank, mask, allowed


draw_case.l2_cases = 0


def whole(c, corpus, allowed, rank, q, k, thr):
    """The oracle over the whole corpus (its allowed rows): global rows, distances (None under cosine), similarities."""
    sub = corpus if len(allowed) == corpus.shape[0] else np.ascontiguousarray(corpus[allowed])
    sub_rank = None if rank is None else rank[allowed].astype(np.uint64)
    if len(allowed) == 0:
        return np.zeros(0, np.int64), (np.zeros(0, np.float32) if c["metric"] == L2 else None), np.zeros(0, np.float32)
    if c["metric"] == COSINE:
        rows, sims, _, _ = o.scan_cosine(sub, q, k, thr, sub_rank)
        dist = None
    else:
        lanes = L2_DEFS[c["l2_def"]][1]
        rows, dist, sims = o.scan_l2(sub, q, k, thr, sub_rank) if lanes is None else o.scan_l2_f32acc(sub, q, k, thr, sub_rank, lanes=lanes)
    return allowed[rows], dist, sims


def mask_words(bits):
    n = len(bits)
    b = np.zeros((n + 31) // 32 * 32, np.uint8); b[:n] = bits
    return np.packbits(b.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()


def make_views(sh, c, corpus, parts, rank, mask):
    from yams_amd import _lib
    d = c["dim"]
    keep, views = [], []
    for i, glob in enumerate(parts):
        acc = sh.ctx(i)
        m = len(glob)
        kw = dict(row_base=int(glob[0]) if m else 0) if c["layout"] == "contiguous" else \
            dict(stripe_rows=c["stripe"], n_stripes=c["n_shards"], stripe_index=i)
        if m == 0:
            views.append(acc.corpus_view(None, 0, d, **kw))
            continue
        dc = acc.to_device(np.ascontiguousarray(corpus[glob])); keep.append(dc)
        db, dn = acc.alloc(m * d * 2), acc.alloc(m * 4); keep += [db, dn]
        acc.build_shadow_device(dc.ptr, m, d, db.ptr, dn.ptr)
        kw.update(rows_bf16_ptr=db.ptr, rows_nsq_ptr=dn.ptr)
        if d >= 256:
            d8, dm8 = acc.alloc(_lib.i8_shadow_rows(m) * d), acc.alloc((m + 15) // 16 * 8); keep += [d8, dm8]
            acc.build_shadow_i8_device(dc.ptr, m, d, d8.ptr, dm8.ptr, i8_flags=c["i8_flags"])
            kw.update(rows_i8_ptr=d8.ptr, rows_i8_meta_ptr=dm8.ptr, i8_flags=c["i8_flags"])
        if rank is not None:                    # local tie ranks: a permutation of 0..m-1 that preserves the global order
            order = np.argsort(rank[glob], kind="stable")
            local = np.empty(m, np.uint32); local[order] = np.arange(m, dtype=np.uint32)
            inv = np.empty_like(local); inv[local] = np.arange(m, dtype=np.uint32)
            dr, di = acc.to_device(local), acc.to_device(inv); keep += [dr, di]
            kw.update(tie_rank_ptr=dr.ptr, rank_row_ptr=di.ptr)
        if mask is not None:
            dm = acc.to_device(mask_words(mask[glob])); keep.append(dm)
            kw.update(row_mask_ptr=dm.ptr, row_mask_count=int(mask[glob].sum()))
        acc.synchronize()
        views.append(acc.corpus_view(dc.ptr, m, d, **kw))
    return keep, views


def compare(c, corpus, allowed, rank, q, k, r):
    """None, or what differs between the merged result and the oracle over the whole corpus."""
    for qi in range(q.shape[0]):
        rows, dist, sims = whole(c, corpus, allowed, rank, q[qi], k, c["thr"])
        cnt = int(r.counts[qi])
        if cnt != len(rows):
            return {"query": qi, "what": "count", "got": cnt, "want": len(rows)}
        if not np.array_equal(r.rows[qi, :cnt], rows):
            at = int(np.flatnonzero(r.rows[qi, :cnt] != rows)[0])
            return {"query": qi, "what": "rows", "at": at, "got": r.rows[qi, at:at + 6].tolist(), "want": rows[at:at + 6].tolist()}
        if not np.array_equal(r.scores[qi, :cnt].view(np.uint32), sims.view(np.uint32)):
            return {"query": qi, "what": "score bits"}
        if dist is not None and not np.array_equal(r.dist[qi, :cnt].view(np.uint32), dist.view(np.uint32)):
            return {"query": qi, "what": "distance bits"}
        if not ((r.rows[qi, cnt:] == -1).all() and np.isneginf(r.scores[qi, cnt:]).all() and np.isposinf(r.dist[qi, cnt:]).all()):
            return {"query": qi, "what": "padding"}
    if r.diag["rows_visited"] != q.shape[0] * len(allowed):
        return {"what": "rows_visited", "got": r.diag["rows_visited"], "want": q.shape[0] * len(allowed)}
    return None


def over_the_limit(stub):
    """Nine shards x k = 1024 = 9216 entries: the batch is refused with UNSUPPORTED, the handle serves the next one."""
    from yams_amd import _lib
    from yams_amd.accel import ShardedScan
    bad = []
    c = {"metric": COSINE, "thr": -1.0, "dim": 64, "layout": "contiguous", "n_shards": 9, "i8_flags": 0}
    g = np.random.default_rng(99)
    corpus = g.standard_normal((4000, 64)).astype(np.float32); q = g.standard_normal((3, 64)).astype(np.float32)
    parts = [np.arange(4000 * i // 9, 4000 * (i + 1) // 9) for i in range(9)]
    for kw in (dict(collective="peer"), dict(collective="rccl", rccl_library=stub)):
        sh = ShardedScan([0] * 9, lanes=2, **kw)
        keep, views = make_views(sh, c, corpus, parts, None, None)
        try:
            sh.topk(views, q, 1024)
            bad.append({"check": "over the limit", "exchange": kw["collective"], "status": "OK"})
        except _lib.AccelError as e:
            if e.status != _lib.YAMS_ERR_UNSUPPORTED or "8192" not in str(e):
                bad.append({"check": "over the limit", "exchange": kw["collective"], "status": e.status, "error": str(e)})
        why = compare(c, corpus, np.arange(4000), None, q, 100, sh.topk(views, q, 100))
        if why:
            bad.append({"check": "the batch after the refused one", "exchange": kw["collective"], **why})
        for b in keep:
            b.free()
        sh.close()
    return bad


t0 = time.time()
bad, hits, compared_queries, batches_run, scripted = [], {p: 0 for p in PATHS}, 0, 0, 0
stub = None
if not a.dry_run:
    import _cpp_build
    from yams_amd.accel import ShardedScan
    stub = _cpp_build.build_stub_collective()
    bad += over_the_limit(stub); scripted = 2
for case in range(a.cases if not bad else 0):
    c, corpus, parts, queries, rank, mask, allowed = draw_case(case)
    k, metric = c["k"], c["metric"]
    flags = L2_DEFS[c["l2_def"]][2] if metric == L2 else 0
    if not a.dry_run:
        desc = {x: c[x] for x in c}
        try:
            sh = ShardedScan([0] * c["n_shards"], lanes=3, collective=c["exchange"], rccl_library=stub if c["exchange"] == "rccl" else None)
            info = sh.info()
            want_mode = "rccl" if c["exchange"] == "rccl" else ("none" if c["n_shards"] == 1 else "peer_copy")
            if info["collective"] != want_mode:
                bad.append(dict(desc, what="exchange form", got=info["collective"], want=want_mode)); break
            keep, views = make_views(sh, c, corpus, parts, rank, mask)
            drank = sh.ctx(0).to_device(rank) if rank is not None else None
            kw = dict(rank_of_row_ptr=drank.ptr if drank else None, rank_row_base=0)
            if len(queries) == 1:
                results = [sh.topk(views, queries[0], k, c["thr"], metric, flags, **kw)]
            else:                               # several batches in flight on different lanes, waited for in reverse order
                lanes = [sh.submit(views, q, k, c["thr"], metric, flags, **kw) for q in queries]
                if len(set(lanes)) != len(lanes):
                    bad.append(dict(desc, what="lanes", got=lanes)); break
                results = [None] * len(queries)
                for bi in reversed(range(len(queries))):
                    results[bi] = sh.wait(lanes[bi])
            for b in keep + ([drank] if drank else []):
                b.free()
            sh.close()
        except Exception as e:                  # every drawn call is a valid one
            bad.append(dict(desc, error=str(e)[:300]))
            break
        n_bad = len(bad)
        for q, r in zip(queries, results):
            why = compare(c, corpus, allowed, rank, q, k, r)
            batches_run += 1; compared_queries += q.shape[0]
            if why:
                bad.append(dict(desc, **why))
                break
        if len(bad) > n_bad and not a.keep_going:
            break
    # the paths this case reached
    h = hits
    sizes = [len(p) for p in parts]
    if c["n_shards"] == 1:
        h["one_shard"] += 1
    h["exchange_rccl_one_rank" if c["exchange"] == "rccl" and c["n_shards"] == 1 else "exchange_" + c["exchange"]] += c["n_shards"] > 1 or c["exchange"] == "rccl"
    h[c["layout"]] += 1
    if c["layout"] == "striped":
        h["stripe_%d" % c["stripe"]] += 1
    h["shard_of_one_row"] += 1 in sizes
    h["shard_smaller_than_k"] += any(0 < s < k for s in sizes)
    h["shard_of_zero_rows"] += 0 in sizes
    h["dim_%d" % c["dim"]] += 1
    if c["dim"] >= 256:
        h["i8_rotated" if c["i8_flags"] else "i8_plain"] += 1
    h["tie_ranks" if c["ranks"] else "tie_none"] += 1
    h["tie_ranks_under_l2"] += c["ranks"] and metric == L2
    h["mask_" + c["mask"]] += 1
    h["shard_masked_out"] += c["masked_out"] > 0
    h["cosine" if metric == COSINE else L2_DEFS[c["l2_def"]][0]] += 1
    h["cosine_thr_short_lists"] += metric == COSINE and c["thr_bites"]
    h["l2_thr_cut_inside"] += metric == L2 and c["thr_bites"]
    h["k_%d" % k] += 1
    h["total_8192"] += c["n_shards"] * k == 8192
    h["several_batches_in_flight"] += len(queries) > 1
    h["tie_group_straddles_k"] += c["straddle"] and c["n_shards"] > 1
    h["cross_shard_duplicates"] += c["dup_shards"] > 1
print(json.dumps({"mode": "dry-run" if a.dry_run else "device", "cases": a.cases, "seed": a.seed, "mismatches": len(bad), "batches": batches_run,
                  "compared_queries": compared_queries, "scripted_checks": scripted, "paths": hits, "wall_s": round(time.time() - t0, 1),
                  "first_bad": bad[:3]}, default=str))
sys.exit(1 if bad else 0)
