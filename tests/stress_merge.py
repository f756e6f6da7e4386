"""Randomised stress of the shard merge ALONE (merge_topk_kernel through yams_scan_merge_topk_device and
yams_scan_merge_records_device) on synthetic per-shard records, against the plain model of tests/_merge_model.py — whose
authority is the CPU pin of tests/test_merge_model_cpu.py.  No scan runs, so thousands of merges are cheap.  One case is one
merge.  Test infrastructure.

    python tests/stress_merge.py [--cases 3000] [--seed 1] [--dry-run] [--keep-going]

Each case draws n_shards (1..64) and k (1..1024) with n_shards * k <= 8192 — pinned shapes: a total of 1, 8192 as 8 x 1024
and as 64 x 128, totals one below / one above a power of two, k = 1, one shard —, 1..300 queries, counts of 0 / 1 / a random
value below k / k per shard and query (some queries empty in every shard, some alive in exactly one: the first, the last or
a middle one), scores and distances from a pool of at most 8 values (±0.0, a denormal, ±1, neighbours one ulp apart; under
L2 equal distances with different similarities) or random ones, every list sorted by the contract as a shard's search
emits it, globally unique int64 row ids (some above 2^32, some planted in two shards with equal and with different ranks),
the tie source (none, the records' own ranks, rank_of_row with rank_row_base 0 or positive, both — the records' ranks win —,
every rank equal), the metric, a threshold below / inside / above the merged top k, the defer flag, the entry point (dense
arrays, or packed records in all four with/without combinations of distances and ranks, with record_stride = layout.bytes
or padded by a poisoned gap), and out_dist (null, from the input distances, or 1 - score).

What the two entry points do with YAMS_SCAN_FLAG_DEFER_THRESHOLD under L2 is pinned as it is today: merge_records honours
it (nothing is dropped), merge_topk ignores it (the threshold is applied).

Every input slot at or behind its count holds a decoy that would change the answer if read (score +inf, distance -inf,
rank 0, the row id of some other entry); padding between records repeats a valid row id.  No poison is a value that could
take a wrong kernel out of the buffers: rows always index rank_of_row inside the table.  Outputs are pre-filled with a
sentinel and ALL n_queries * k slots are compared: scores and distances bit for bit, rows and counts exactly.

Argument handling is checked once per run, outside the random loop (statuses, and that nothing was written).  The harness
stops at the first failing case (--keep-going: counts them all) and never retries.  --dry-run draws the cases and runs the model without touching the
device: the summary's path counts depend on the generator alone.  The paths (each must be reached, the GPU test asserts
floors): see PATHS.
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _merge_model as mm

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=3000)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--dry-run", action="store_true")
ap.add_argument("--keep-going", action="store_true", help="count the mismatching cases instead of stopping at the first")
a = ap.parse_args()
rng = np.random.default_rng(a.seed)

PATHS = ["entry_dense", "entry_records", "layout_plain", "layout_dist", "layout_ranks", "layout_dist_ranks",
         "stride_exact", "stride_padded", "tie_none", "tie_own_ranks", "tie_rank_of_row_base0", "tie_rank_of_row_based",
         "tie_both", "tie_all_equal", "cosine_thr_below", "cosine_thr_inside", "cosine_thr_above", "l2_thr_below",
         "l2_thr_inside", "l2_thr_above", "l2_defer_dense_ignored", "l2_defer_records_honoured", "l2_cut_dense", "l2_cut_records",
         "out_dist_null", "out_dist_from_input", "out_dist_one_minus_score", "total_1", "total_8192_as_8x1024",
         "total_8192_as_64x128", "total_pow2_minus_1", "total_pow2_plus_1", "k_1", "one_shard", "queries_gt_1",
         "query_empty_everywhere", "query_alive_in_one_shard", "short_lists", "rows_above_2_32", "duplicate_row_equal_ranks",
         "duplicate_row_different_ranks", "tie_pool", "random_values", "cross_shard_tie_at_k"]
ONE = np.float32(1.0)
SCORE_POOL = np.array([0.0, -0.0, 1e-40, 1.0, -1.0, np.nextafter(ONE, np.float32(0)), 0.5, np.nextafter(np.float32(0.5), ONE)], np.float32)
DIST_POOL = np.array([0.0, 1e-40, 0.5, 1.0, np.nextafter(ONE, np.float32(2))], np.float32)
SENTINEL32, SENTINEL_ROW = 0xDEADBEEF, -7777
FLAG_DEFER = 1                                      # YAMS_SCAN_FLAG_DEFER_THRESHOLD
NO_PART = (1 << 64) - 1


def log_uniform(lo, hi):
    return int(min(hi, np.exp(rng.uniform(np.log(lo), np.log(hi + 1)))))


def draw_shape(case):
    pin = case % 25
    if pin == 0: return 1, 1
    if pin == 1: return 8, 1024
    if pin == 2: return 64, 128
    if pin == 3: return [(3, 21), (7, 73), (1, 1023), (31, 33), (3, 5), (63, 65)][int(rng.integers(0, 6))]       # 63, 511, 1023, 1023, 15, 4095
    if pin == 4: return [(5, 13), (3, 171), (1, 513), (17, 241), (3, 43), (9, 57)][int(rng.integers(0, 6))]       # 65, 513, 513, 4097, 129, 513
    if pin == 5: return log_uniform(1, 64), 1
    if pin == 6: return 1, log_uniform(1, 1024)
    n_shards = log_uniform(1, 64)
    return n_shards, log_uniform(1, min(1024, 8192 // n_shards))


def is_pow2(v):
    return v & (v - 1) == 0


def draw_case(case):
    """All of one merge: the inputs as dense [n_shards][nq][k] arrays plus how they are to be handed over."""
    n_shards, k = draw_shape(case)
    total = n_shards * k
    nq = log_uniform(1, min(300, max(1, 32768 // total)))
    if case % 25 >= 7 and rng.random() < 0.15:
        nq = min(nq, 1 + int(rng.integers(0, 2)))
    metric = mm.L2 if rng.random() < 0.5 else mm.COSINE
    shape = (n_shards, nq, k)
    # counts
    kind = rng.integers(0, 4, (n_shards, nq))
    counts = np.select([kind == 0, kind == 1, kind == 2], [0, 1, rng.integers(0, k, (n_shards, nq))], k).astype(np.int64)
    counts = np.minimum(counts, k)
    empty_q = rng.random(nq) < 0.1
    counts[:, empty_q] = 0
    lone_q = (rng.random(nq) < 0.12) & ~empty_q
    for qi in np.flatnonzero(lone_q):
        s = [0, n_shards - 1, n_shards // 2][int(rng.integers(0, 3))]
        c = max(1, int(counts[s, qi]))
        counts[:, qi] = 0; counts[s, qi] = c
    live = np.arange(k)[None, None, :] < counts[:, :, None]
    # values
    pooled = rng.random() < 0.5
    if pooled:
        scores = rng.choice(SCORE_POOL[rng.permutation(8)[:int(rng.integers(1, 9))]], shape)
        dist = rng.choice(DIST_POOL[rng.permutation(5)[:int(rng.integers(1, 5))]], shape)
    else:
        scores = np.clip(rng.standard_normal(shape) * 0.4, -1, 1).astype(np.float32)
        dist = np.abs(rng.standard_normal(shape)).astype(np.float32)
    # rows: every slot gets an id of its own; the table a rank_of_row lookup may touch covers all of them
    m = n_shards * nq * k + int(rng.integers(1, 64))
    big = rng.random() < 0.3
    base = int(rng.choice([1 << 32, (1 << 40) + 12345, (1 << 32) - 5])) if big else int(rng.choice([0, 0, 0, 1000]))
    ids = rng.permutation(m)[:n_shards * nq * k].reshape(shape).astype(np.int64)
    # tie source
    source = ["none", "own", "table", "table", "both", "equal"][int(rng.integers(0, 6))]
    table = rng.permutation(m).astype(np.uint32)
    table2 = rng.permutation(m).astype(np.uint32)
    if rng.random() < 0.3:
        table2 %= np.uint32(max(2, m // 8))                        # own ranks that collide: the order falls through to the row id
    if source == "equal":
        table[:] = 7; table2[:] = 7
    own = source in ("own", "both") or (source == "equal" and rng.random() < 0.5)
    use_table = source in ("table", "both") or (source == "equal" and not own)
    if use_table and source != "both" and rng.random() < 0.5 and not big:
        base = 0
    rank_row_base = base if use_table else 0
    # one row id in two shards, every key above it equal
    dup = None
    both_alive = np.flatnonzero(((counts > 0).sum(axis=0) >= 2))
    if n_shards >= 2 and len(both_alive) and rng.random() < 0.3:
        qi = int(rng.choice(both_alive))
        sa, sb = [int(x) for x in rng.choice(np.flatnonzero(counts[:, qi] > 0), 2, replace=False)]
        ia, ib = int(rng.integers(0, counts[sa, qi])), int(rng.integers(0, counts[sb, qi]))
        ids[sb, qi, ib] = ids[sa, qi, ia]; scores[sb, qi, ib] = scores[sa, qi, ia]; dist[sb, qi, ib] = dist[sa, qi, ia]
        dup = (qi, sa, ia, sb, ib)
    ranks = table2[ids].astype(np.int64)
    dup_kind = None
    if dup is not None:
        dup_kind = "equal"
        if own and metric == mm.COSINE and source != "equal" and rng.random() < 0.5:
            qi, sa, ia, sb, ib = dup
            ranks[sb, qi, ib] = ranks[sa, qi, ia] - 1 if ranks[sa, qi, ia] > 0 and rng.random() < 0.5 else ranks[sa, qi, ia] + 1
            dup_kind = "different"
    rows = ids + base
    # each list in the order its shard would emit it
    eff = ranks if own else (table[ids].astype(np.int64) if use_table else np.zeros(shape, np.int64))
    if metric == mm.L2:
        order = np.lexsort((rows, dist, ~live), axis=-1)
    else:
        order = np.lexsort((rows, eff, -scores, ~live), axis=-1)
    scores, dist, rows, ranks, ids = (np.take_along_axis(x, order, axis=-1) for x in (scores, dist, rows, ranks, ids))
    # decoys behind the counts
    live_ids = rows[live]
    decoy_rows = rng.choice(live_ids, shape) if len(live_ids) else np.full(shape, base, np.int64)
    scores = np.where(live, scores, np.float32(np.inf)).astype(np.float32)
    dist = np.where(live, dist, np.float32(-np.inf)).astype(np.float32)
    rows = np.where(live, rows, decoy_rows).astype(np.int64)
    ranks = np.where(live, ranks, 0).astype(np.uint32)
    # how it is handed over
    records = use_table or rng.random() < 0.5
    with_dist = metric == mm.L2 or rng.random() < 0.5
    want_out_dist = rng.random() < 0.7
    stride_pad = 8 * int(rng.integers(1, 40)) if records and rng.random() < 0.5 else 0
    c = {"case": case, "n_shards": n_shards, "k": k, "nq": nq, "metric": metric, "pooled": pooled, "source": source, "own": own,
         "use_table": use_table, "base": base, "rank_row_base": rank_row_base, "records": records, "with_dist": with_dist,
         "want_out_dist": want_out_dist, "stride_pad": stride_pad, "dup_kind": dup_kind, "big": big,
         "empty_q": int(((counts > 0).sum(axis=0) == 0).sum()), "lone_q": int(((counts > 0).sum(axis=0) == 1).sum()) if n_shards > 1 else 0,
         "short": bool((counts < k).any())}
    arrays = {"scores": scores, "rows": rows, "counts": counts.astype(np.uint32), "dist": dist, "ranks": ranks, "table": table,
              "gap_row": int(live_ids[0]) if len(live_ids) else base}
    return c, arrays


def model_shards(c, arrays):
    out = []
    for s in range(c["n_shards"]):
        sh = {"scores": arrays["scores"][s], "rows": arrays["rows"][s], "counts": arrays["counts"][s]}
        if c["with_dist"]:
            sh["dist"] = arrays["dist"][s]
        if c["own"]:
            sh["ranks"] = arrays["ranks"][s]
        out.append(sh)
    return out


def choose_threshold(c, uncut):
    """A threshold below, inside or above the merged top k (of one query, for `inside`), and where it really fell."""
    S, _, Cn, _ = uncut
    alive = np.flatnonzero(Cn > 0)
    want = ["below", "inside", "above"][int(rng.integers(0, 3))]
    thr = float(rng.uniform(-1, 1))
    if len(alive):
        used = np.arange(c["k"])[None, :] < Cn[:, None]
        if want == "below":
            thr = float(np.nextafter(S[used].min(), np.float32(-np.inf))) if rng.random() < 0.7 else -np.inf
        elif want == "above":
            thr = float(np.nextafter(S[used].max(), np.float32(np.inf)))
        else:
            qi = int(rng.choice(alive))
            vals = np.unique(S[qi, :Cn[qi]])                 # ascending; -0.0 and +0.0 are one value
            thr = float(vals[int(rng.integers(1, len(vals)))]) if len(vals) > 1 else float(vals[0])
        kept = ((~(S < np.float32(thr))) & used).sum(axis=1)
        where = "inside" if ((kept > 0) & (kept < Cn)).any() else ("below" if (kept == Cn).all() else ("above" if (kept == 0).all() else None))
    else:
        where = None
    return thr, where


def pack_records(acc, c, arrays):
    """The shards as packed records `stride` bytes apart; the gaps (alignment padding and the stride's tail) repeat a row id."""
    lay = acc.record_layout(c["nq"], c["k"], c["with_dist"], c["own"]) if acc is not None else host_layout(c["nq"], c["k"], c["with_dist"], c["own"])
    ref = host_layout(c["nq"], c["k"], c["with_dist"], c["own"])
    got = tuple(int(getattr(lay, f)) for f in ("scores_off", "rows_off", "counts_off", "dist_off", "ranks_off", "bytes"))
    assert got == ref_tuple(ref), ("yams_scan_record_layout", got, ref_tuple(ref))
    stride = got[5] + c["stride_pad"]
    buf = np.full(c["n_shards"] * stride // 8, arrays["gap_row"], np.int64).view(np.uint8)
    for s in range(c["n_shards"]):
        rec = buf[s * stride:(s + 1) * stride]
        parts = [("scores", got[0]), ("rows", got[1]), ("counts", got[2])] + ([("dist", got[3])] if c["with_dist"] else []) + \
                ([("ranks", got[4])] if c["own"] else [])
        for name, off in parts:
            raw = np.ascontiguousarray(arrays[name][s]).view(np.uint8).reshape(-1)
            rec[off:off + raw.size] = raw
    return lay, stride, buf


class host_layout:
    """yams_scan_record_layout restated from the header: scores | rows | counts (| dist) (| ranks), every part 16-byte aligned."""
    def __init__(self, nq, k, with_dist, with_ranks):
        al = lambda v: (v + 15) & ~15
        qk = nq * max(k, 1)
        self.scores_off = 0; off = al(qk * 4)
        self.rows_off = off; off = al(off + qk * 8)
        self.counts_off = off; off = al(off + nq * 4)
        self.dist_off = off if with_dist else NO_PART
        if with_dist: off = al(off + qk * 4)
        self.ranks_off = off if with_ranks else NO_PART
        if with_ranks: off = al(off + qk * 4)
        self.bytes = off


def ref_tuple(l):
    return (l.scores_off, l.rows_off, l.counts_off, l.dist_off, l.ranks_off, l.bytes)


def run_device(acc, c, arrays, thr, flags):
    nq, k, n_shards = c["nq"], c["k"], c["n_shards"]
    keep = []
    up = lambda x: keep.append(acc.to_device(x)) or keep[-1]
    o_s = up(np.full(nq * k, SENTINEL32, np.uint32)); o_r = up(np.full(nq * k, SENTINEL_ROW, np.int64))
    o_c = up(np.full(nq, SENTINEL32, np.uint32)); o_d = up(np.full(nq * k, SENTINEL32, np.uint32)) if c["want_out_dist"] else None
    try:
        if c["records"]:
            lay, stride, buf = pack_records(acc, c, arrays)
            d_rec = up(buf)
            d_tab = up(arrays["table"]) if c["use_table"] else None
            acc.merge_records_device(n_shards, nq, k, thr, c["metric"], d_rec.ptr, stride, lay, d_tab.ptr if d_tab else None,
                                     c["rank_row_base"], o_s.ptr, o_r.ptr, o_c.ptr, o_d.ptr if o_d else None, flags=flags)
        else:
            d_s, d_r, d_c = up(arrays["scores"]), up(arrays["rows"]), up(arrays["counts"])
            d_d = up(arrays["dist"]) if c["with_dist"] else None
            d_k = up(arrays["ranks"]) if c["own"] else None
            acc.merge_topk_device(n_shards, nq, k, thr, c["metric"], d_s.ptr, d_r.ptr, d_c.ptr, d_d.ptr if d_d else None,
                                  d_k.ptr if d_k else None, o_s.ptr, o_r.ptr, o_c.ptr, o_d.ptr if o_d else None, flags=flags)
        acc.synchronize()
        return (o_s.download(np.uint32, nq * k).reshape(nq, k), o_r.download(np.int64, nq * k).reshape(nq, k), o_c.download(np.uint32, nq),
                o_d.download(np.uint32, nq * k).reshape(nq, k) if o_d else None)
    finally:
        for b in keep:
            b.free()


def check_arguments(acc):
    """Statuses that must come back without a launch; the outputs keep their sentinel.  Returns the list of failures."""
    import ctypes as C
    from yams_amd import _lib
    from yams_amd._lib import ScanParams, AccelError
    bad = []
    nq, k, n_shards = 2, 3, 2
    lay = acc.record_layout(nq, k, True, True)
    lay_nodist = acc.record_layout(nq, k, False, False)
    rec = acc.to_device(np.zeros(n_shards * (lay.bytes + 64), np.uint8))
    big = acc.to_device(np.zeros(8193 * 32, np.uint8))                 # holds a whole record of k = 8193, were it ever read
    outs = [acc.to_device(np.full(8193 * nq, SENTINEL32, np.uint32)), acc.to_device(np.full(8193 * nq, SENTINEL_ROW, np.int64)),
            acc.to_device(np.full(nq, SENTINEL32, np.uint32)), acc.to_device(np.full(8193 * nq, SENTINEL32, np.uint32))]

    def untouched(counts_zeroed=False):
        acc.synchronize()
        s, r, c, d = outs[0].download(np.uint32, 8193 * nq), outs[1].download(np.int64, 8193 * nq), outs[2].download(np.uint32, nq), outs[3].download(np.uint32, 8193 * nq)
        ok = (s == SENTINEL32).all() and (r == SENTINEL_ROW).all() and (d == SENTINEL32).all() and ((c == 0).all() if counts_zeroed else (c == SENTINEL32).all())
        outs[2].upload(np.full(nq, SENTINEL32, np.uint32))
        return bool(ok)

    def dense(name, want, n_sh, n_q, kk, metric=mm.COSINE, params=True, with_dist=True, zeroed=False):
        prm = ScanParams(kk, 0.0, metric, 0)
        st = acc.L.yams_scan_merge_topk_device(acc.ctx, n_sh, n_q, C.byref(prm) if params else None, big.ptr, big.ptr, big.ptr,
                                               big.ptr if with_dist else None, None, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr)
        if st != want or not untouched(zeroed):
            bad.append({"check": "merge_topk: " + name, "status": st, "want": want})

    def records(name, want, n_sh, n_q, kk, metric=mm.COSINE, params=True, layout=lay, stride=None, zeroed=False, buf=rec):
        prm = ScanParams(kk, 0.0, metric, 0)
        st = acc.L.yams_scan_merge_records_device(acc.ctx, n_sh, n_q, C.byref(prm) if params else None, buf.ptr,
                                                  layout.bytes if stride is None else stride, C.byref(layout), None, 0,
                                                  outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr)
        if st != want or not untouched(zeroed):
            bad.append({"check": "merge_records: " + name, "status": st, "want": want})

    lay8193 = acc.record_layout(1, 8193, True, True)
    INV, UNS, OK = _lib.YAMS_ERR_INVALID_ARG, _lib.YAMS_ERR_UNSUPPORTED, _lib.YAMS_OK
    dense("n_shards * k == 8193", UNS, 1, 1, 8193); records("n_shards * k == 8193", UNS, 1, 1, 8193, layout=lay8193, buf=big)
    dense("n_shards == 0", INV, 0, nq, k); records("n_shards == 0", INV, 0, nq, k)
    dense("null params", INV, n_shards, nq, k, params=False); records("null params", INV, n_shards, nq, k, params=False)
    records("stride not a multiple of 8", INV, n_shards, nq, k, stride=lay.bytes + 4)
    records("stride smaller than the record", INV, n_shards, nq, k, stride=lay.bytes - 8)
    dense("L2 without distances", INV, n_shards, nq, k, metric=mm.L2, with_dist=False)
    records("L2 without distances", INV, n_shards, nq, k, metric=mm.L2, layout=lay_nodist)
    dense("k == 0", OK, n_shards, nq, 0, zeroed=True); records("k == 0", OK, n_shards, nq, 0, zeroed=True)
    dense("n_queries == 0", OK, n_shards, 0, k); records("n_queries == 0", OK, n_shards, 0, k)
    for b in [rec, big] + outs:
        b.free()
    return bad, 15


t0 = time.time()
acc = None
bad, hits, merges, slots, arg_checks = [], {p: 0 for p in PATHS}, 0, 0, 0
if not a.dry_run:
    from yams_amd.accel import Accel
    acc = Accel(0)
    arg_bad, arg_checks = check_arguments(acc)
    bad += arg_bad
for case in range(a.cases if not bad else 0):
    c, arrays = draw_case(case)
    shards = model_shards(c, arrays)
    table = arrays["table"] if c["use_table"] else None
    uncut = mm.merge(shards, c["k"], c["metric"], rank_of_row=table, rank_row_base=c["rank_row_base"], defer=True)
    thr, where = choose_threshold(c, uncut)
    defer_flag = rng.random() < 0.4
    honoured = defer_flag and c["records"]                       # pinned: merge_topk ignores the flag, merge_records honours it
    if c["metric"] == mm.COSINE or honoured:
        want = uncut
    else:
        want = mm.merge(shards, c["k"], c["metric"], thr, rank_of_row=table, rank_row_base=c["rank_row_base"], defer=False)
    c.update(thr=thr, where=where, defer_flag=bool(defer_flag))
    merges += 1
    if acc is not None:
        try:
            got = run_device(acc, c, arrays, thr, FLAG_DEFER if defer_flag else 0)
        except Exception as e:                                   # every drawn call is a valid one
            bad.append(dict(c, error=str(e)[:300]))
            break
        n_bad = len(bad)
        checks = [("scores", got[0], want[0].view(np.uint32)), ("rows", got[1], want[1]), ("counts", got[2], want[2])]
        if c["want_out_dist"]:
            checks.append(("dist", got[3], want[3].view(np.uint32)))
        for name, g, w in checks:
            if not np.array_equal(g, w):
                at = np.argwhere(g != w)[0].tolist()
                qi = at[0]
                bad.append(dict(c, what=name, at=at, got_rows=got[1][qi, :8].tolist(), want_rows=want[1][qi, :8].tolist(),
                                got_scores=got[0][qi, :8].tolist(), want_scores=want[0][qi, :8].view(np.uint32).tolist(),
                                got_count=int(got[2][qi]), want_count=int(want[2][qi])))
                break
        if len(bad) > n_bad and not a.keep_going:
            break
        slots += c["nq"] * c["k"]
    # the paths this case reached
    total, l2 = c["n_shards"] * c["k"], c["metric"] == mm.L2
    h = hits
    h["entry_records" if c["records"] else "entry_dense"] += 1
    if c["records"]:
        h[{(0, 0): "layout_plain", (1, 0): "layout_dist", (0, 1): "layout_ranks", (1, 1): "layout_dist_ranks"}[(int(c["with_dist"]), int(c["own"]))]] += 1
        h["stride_padded" if c["stride_pad"] else "stride_exact"] += 1
    if c["source"] == "equal": h["tie_all_equal"] += 1
    elif c["source"] == "both": h["tie_both"] += 1
    elif c["own"]: h["tie_own_ranks"] += 1
    elif c["use_table"]: h["tie_rank_of_row_based" if c["rank_row_base"] else "tie_rank_of_row_base0"] += 1
    else: h["tie_none"] += 1
    if where:
        h[("l2" if l2 else "cosine") + "_thr_" + where] += 1
    if l2:
        if defer_flag: h["l2_defer_records_honoured" if c["records"] else "l2_defer_dense_ignored"] += 1
        elif where in ("inside", "above"): h["l2_cut_records" if c["records"] else "l2_cut_dense"] += 1
    h["out_dist_null" if not c["want_out_dist"] else ("out_dist_from_input" if c["with_dist"] else "out_dist_one_minus_score")] += 1
    h["total_1"] += total == 1
    h["total_8192_as_8x1024"] += (c["n_shards"], c["k"]) == (8, 1024)
    h["total_8192_as_64x128"] += (c["n_shards"], c["k"]) == (64, 128)
    h["total_pow2_minus_1"] += total > 2 and is_pow2(total + 1)
    h["total_pow2_plus_1"] += total > 3 and is_pow2(total - 1)
    h["k_1"] += c["k"] == 1
    h["one_shard"] += c["n_shards"] == 1
    h["queries_gt_1"] += c["nq"] > 1
    h["query_empty_everywhere"] += c["empty_q"] > 0
    h["query_alive_in_one_shard"] += c["lone_q"] > 0
    h["short_lists"] += c["short"]
    h["rows_above_2_32"] += c["big"]
    h["duplicate_row_equal_ranks"] += c["dup_kind"] == "equal"
    h["duplicate_row_different_ranks"] += c["dup_kind"] == "different"
    h["tie_pool" if c["pooled"] else "random_values"] += 1
    # a group of equal keys straddling position k whose members come from different shards
    S, R, Cn, D = uncut
    full = np.flatnonzero(Cn == c["k"])
    if c["n_shards"] > 1 and len(full):
        key = D if l2 else S
        live_total = arrays["counts"].sum(axis=0)
        for qi in full[:8]:
            if live_total[qi] > c["k"]:
                last = key[qi, c["k"] - 1]
                n_eq = sum(int((arrays["dist" if l2 else "scores"][s, qi, :arrays["counts"][s, qi]] == last).sum() > 0) for s in range(c["n_shards"]))
                n_all = sum(int((arrays["dist" if l2 else "scores"][s, qi, :arrays["counts"][s, qi]] == last).sum()) for s in range(c["n_shards"]))
                if n_eq >= 2 and n_all > int((key[qi] == last).sum()):
                    h["cross_shard_tie_at_k"] += 1
                    break
if acc is not None:
    acc.close()
print(json.dumps({"mode": "dry-run" if a.dry_run else "device", "cases": a.cases, "seed": a.seed, "merges": merges, "mismatches": len(bad),
                  "slots_compared": slots, "arg_checks": arg_checks, "paths": hits, "wall_s": round(time.time() - t0, 1), "first_bad": bad[:3]},
                 default=str))
sys.exit(1 if bad else 0)
