"""Seeded stress of the GENERAL scan across the dimension lattice (tests/_dim_lattice.py: every class of dim % 4 / 16 / 32 /
64 / 128 and base alignment, on every tier and kernel form the class can reach) against the CPU oracle, bit for bit.

Cases cycle through the (class, form, metric) cells, so every cell occurs at any seed; the dim inside the cell, the rows
(4096 .. 5001: ragged against the 64-, 128- and 256-row tiles), the queries (1 .. 257), k, the threshold, a dense allow-mask, a
shuffled tie rank and the L2 accumulation flag are drawn.  Half the queries of a case are localised on a group of at most 16
elements with planted rows that make that group decide the answer (_dim_lattice.discriminates proves it per case, from the
oracle alone).  Per case:

  * up to 8 queries (the first, the last, both sides of 64 and 128, at least three localised ones) against the oracle's
    single-query functions: count, row ids, score bits, distance bits under L2, the padding behind the count;
  * EVERY query against the same call under FLAG_FORCE_EXACT — the exhaustive path shares no filter code with the tiers and
    is itself held to the oracle on the picked queries; where the default call already is the exhaustive path (classes A
    and B, an allow-mask below 16384 rows) every query goes through the oracle while n * dim * nq <= 4e8, else 16 do;
  * diag.path and diag.filter_tier against _dim_lattice.restated_route (not where it returns None: the choice depends on the
    device's CU count), rows_visited and exact_distance_evaluations against nq * n_eff;
  * exact_fallback_queries == 0 wherever a filter ran: the rows are continuous draws without a duplicate plateau, so an
    exhaustive pass there would stand in for a list that lost its rows.

All cases run on ONE context, in sequence.  The harness stops at the first failing case, prints one JSON line with its draw,
and never retries.

    python tests/stress_dims.py [--cases N] [--seed S]     on the GPU
    python tests/stress_dims.py --dry-run                  draws + discriminates + oracle only: reports the counters
    python tests/stress_dims.py --self-test                compare_query() must report each mutated oracle answer
"""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

import _oracle
import _dim_lattice as dl
from _dim_lattice import SCAN_COSINE, SCAN_L2, FLAG_FORCE_EXACT

DEFAULT_SEED, DEFAULT_CASES = 5, 138            # 6 rounds over the 23 cells
TIER_NAMES = {0: "none", 1: "i8", 2: "bf16", 3: "split", 4: "f32", None: "cu_dependent"}
ACC_NAMES = {0: "f64", 256: "f32", 512: "f32x8", 768: "f32x16", 256 | 2048: "f32_fused", 512 | 2048: "f32x8_fused",
             768 | 2048: "f32x16_fused"}
# exact_fallback_queries == 0 is asserted on every case a filter answers, except the shapes named here (docs/LAB_NOTES.md
# records the counts seen): none.
FALLBACK_NOT_ASSERTED = set()


def required_counters():
    """The counters a run of the default size must reach (tests/test_dim_lattice_cpu.py: at least 5 times each)."""
    out = ["cell_%s_%s_%s" % (cls, form, "l2" if m == SCAN_L2 else "cos") for cls, form, m in dl.cells()]
    out += ["g_" + kd for kd in dl.G_KINDS] + ["walk_staged", "walk_vec4_tail", "walk_scalar"]
    out += ["fused", "rotated_two_transforms", "rotated_one_transform", "bare_view", "masked", "tie_rank"]
    out += ["l2_acc_" + v for v in ACC_NAMES.values()]
    return out


def count_case(counters, c, want, tier_answered=None):
    def hit(name):
        counters[name] = counters.get(name, 0) + 1
    d = c.d
    path, tier = want
    hit("cell_%s_%s_%s" % (d["cls"], d["form"], "l2" if d["metric"] == SCAN_L2 else "cos"))
    hit("tier_%s_%s_%s" % (d["cls"], TIER_NAMES[tier if tier_answered is None else tier_answered], d["form"]))
    if tier is None and tier_answered is not None:
        hit("cu_dependent_answered_" + TIER_NAMES[tier_answered])
    for qi in c.localised:
        hit("g_" + c.kinds[qi])
    hit("walk_" + dl.walk(d["dim"], dl.aligned(d)))
    if dl.se.restated_path(d["n"], d["dim"], d["nq"], d["k"], d["metric"], d["flags"], dl.aligned(d)):
        hit("fused")
    if d["i8_flags"] & dl.I8_ROTATED and path == 0:
        hit("rotated_one_transform" if dl.i8_rotation_window(d["dim"]) == d["dim"] else "rotated_two_transforms")
    if d["form"] == "bare":
        hit("bare_view")
    if d["mask"]:
        hit("masked")
    if d["tie"]:
        hit("tie_rank")
    if d["metric"] == SCAN_L2:
        hit("l2_acc_" + ACC_NAMES[d["flags"] & (dl.se.FLAG_L2_ACC_MASK | dl.FLAG_L2_ACC_FUSED)])


def oracle_picks(rng, c, want_path, limit):
    """The queries of the case that go through the oracle."""
    d = c.d
    if want_path == 1 and not dl.se.restated_path(d["n"], d["dim"], d["nq"], d["k"], d["metric"], d["flags"], dl.aligned(d)):
        # the default call IS the exhaustive path: nothing else of the device vouches for it
        limit = d["nq"] if d["n"] * d["dim"] * d["nq"] <= 4e8 else 16
    return dl.pick_queries(rng, d["nq"], c.localised, limit)


def device_case(acc, c, picks, answers, want):
    """The case on the device.  (None | the first difference, info)."""
    d = c.d
    n, dim = c.corpus.shape
    k, metric, flags = d["k"], d["metric"], d["flags"]
    bufs = []

    def dev(arr):
        bufs.append(acc.to_device(arr))
        return bufs[-1].ptr
    try:
        if d["offset"]:                                 # class B: the rows start 4, 8 or 12 bytes into a larger allocation
            big = acc.alloc(c.corpus.nbytes + 32)
            bufs.append(big)
            big.upload(c.corpus, d["offset"])
            rows_p = big.ptr + d["offset"]
        else:
            rows_p = dev(c.corpus)
        kw = {}
        if "bf16" in d["shadows"]:
            db, dn = acc.alloc(c.corpus.size * 2), acc.alloc(n * 4)
            bufs += [db, dn]
            acc.build_shadow_device(rows_p, n, dim, db.ptr, dn.ptr)
            kw.update(rows_bf16_ptr=db.ptr, rows_nsq_ptr=dn.ptr)
        if "i8" in d["shadows"]:
            d8, dm = acc.alloc(dl.i8_shadow_rows(n) * dim), acc.alloc((n + 15) // 16 * 8)
            bufs += [d8, dm]
            acc.build_shadow_i8_device(rows_p, n, dim, d8.ptr, dm.ptr, i8_flags=d["i8_flags"])
            kw.update(rows_i8_ptr=d8.ptr, rows_i8_meta_ptr=dm.ptr, i8_flags=d["i8_flags"])
        if c.tie is not None:
            inv = np.empty_like(c.tie); inv[c.tie] = np.arange(n, dtype=c.tie.dtype)
            kw.update(tie_rank_ptr=dev(c.tie), rank_row_ptr=dev(inv))
        n_eff = n
        if c.allowed is not None:
            bits = np.zeros((n + 31) // 32 * 32, bool); bits[c.allowed] = True
            kw.update(row_mask_ptr=dev(np.packbits(bits, bitorder="little").view(np.uint32)), row_mask_count=len(c.allowed))
            n_eff = len(c.allowed)
        view = acc.corpus_view(rows_p, n, dim, **kw)
        t0 = time.time()
        r = acc.scan_topk(view, c.queries, k, d["thr"], metric, flags)
        info = {"diag": {x: int(v) for x, v in r.diag.items()}, "scan_s": round(time.time() - t0, 3)}
        want_path, want_tier = want
        if r.diag["path"] != want_path:
            return "diag.path %d != %d (the restated route)" % (r.diag["path"], want_path), info
        if want_tier is not None and r.diag["filter_tier"] != want_tier:
            return "diag.filter_tier %d != %d (the restated route)" % (r.diag["filter_tier"], want_tier), info
        for name in ("rows_visited", "exact_distance_evaluations"):
            if r.diag[name] != d["nq"] * n_eff:
                return "%s %d != %d" % (name, r.diag[name], d["nq"] * n_eff), info
        if r.diag["used_exact_scan"] != 1:
            return "used_exact_scan %d" % r.diag["used_exact_scan"], info
        for qi, e in zip(picks, answers):
            msg = dl.compare_query(qi, int(r.counts[qi]), r.rows[qi], r.scores[qi], r.dist[qi], e, k, metric)
            if msg is not None:
                return msg, info
        fused = dl.se.restated_path(n, dim, d["nq"], k, metric, flags, dl.aligned(d))
        if want_path == 0 or fused:
            x = acc.scan_topk(view, c.queries, k, d["thr"], metric, flags | FLAG_FORCE_EXACT)
            if x.diag["path"] != 1 or x.diag["filter_tier"] != 0:
                return "FORCE_EXACT: path %d, filter_tier %d" % (x.diag["path"], x.diag["filter_tier"]), info
            msg = dl.compare_calls(r, x, k, metric)
            if msg is not None:
                return msg, info
            for qi, e in zip(picks, answers):           # (the exhaustive path is itself held to the oracle)
                msg = dl.compare_query(qi, int(x.counts[qi]), x.rows[qi], x.scores[qi], x.dist[qi], e, k, metric)
                if msg is not None:
                    return "FORCE_EXACT " + msg, info
        if want_path == 0 and r.diag["exact_fallback_queries"] != 0 and (d["cls"], d["form"], dim) not in FALLBACK_NOT_ASSERTED:
            return "exact_fallback_queries %d: an exhaustive pass stood in for the filter" % r.diag["exact_fallback_queries"], info
        return None, info
    finally:
        for b in bufs:
            b.free()


def check_case(o, d, acc=None, limit=8, counters=None, rng=None):
    """One draw end to end: build, discriminates, the oracle on the picked queries, (with acc) the device.
    Returns (None | the first difference, info)."""
    rng = rng or np.random.default_rng(d["seed"])
    c = dl.build_case(d)
    msg = dl.discriminates(o, c)
    if msg is not None:
        return "the case does not discriminate: " + msg, {}
    want = dl.route(d, None if c.allowed is None else len(c.allowed))
    picks = oracle_picks(rng, c, want[0], limit)
    if len(c.localised) >= 3 and sum(q in c.localised for q in picks) < 3:
        return "fewer than three localised queries among the picked ones", {}
    answers = [dl.oracle_query(o, c, qi) for qi in picks]
    info = {"picked": len(picks), "localised": len(c.localised)}
    tier_answered = None
    if acc is not None:
        msg, dinfo = device_case(acc, c, picks, answers, want)
        info.update(dinfo)
        if "diag" in dinfo:
            tier_answered = dinfo["diag"]["filter_tier"]
    if counters is not None:
        count_case(counters, c, want, tier_answered)
    return msg, info


def check_forms(o, acc, d, forms, limit=8):
    """One corpus, its discriminates() and its oracle answers shared by several forms of one class (the corpus follows from
    seed, shape and metric alone): the draw `d` with each form's flags, shadows and layout in turn on the device.
    Returns (None | "<form>: the first difference", {form: info})."""
    rng = np.random.default_rng(d["seed"])
    c = dl.build_case(d)
    msg = dl.discriminates(o, c)
    if msg is not None:
        return "the case does not discriminate: " + msg, {}
    infos, cache = {}, {}
    l2_acc = d["flags"] & (dl.se.FLAG_L2_ACC_MASK | dl.FLAG_L2_ACC_FUSED)
    for form in forms:
        c.d = dict(d, form=form, **dl.form_fields(d["cls"], form, d["metric"], l2_acc))
        want = dl.route(c.d, None if c.allowed is None else len(c.allowed))
        picks = tuple(oracle_picks(np.random.default_rng(d["seed"]), c, want[0], limit))
        if picks not in cache:
            cache[picks] = [dl.oracle_query(o, c, qi) for qi in picks]
        msg, infos[form] = device_case(acc, c, list(picks), cache[picks], want)
        if msg is not None:
            return "%s: %s" % (form, msg), infos
    return None, infos


def scripted_draws(cls, dim):
    """The scripted cells of one dim (tests/test_dim_lattice_gpu.py; rehearsed on the CPU by tests/test_dim_lattice_cpu.py):
    per metric (metric, forms, l2_acc, oracle-checked queries, draw).  The shapes keep a dim at a few seconds — the oracle walks
    n * dim per query: 65 or 33 queries up to dim 560, 17 up to 2100, 3 above."""
    nq, limit = (65, 8) if dim <= 560 else ((17, 6) if dim <= 2100 else (3, 3))
    idx = dl.CLASSES[cls].index(dim)
    k = [10, 100][idx % 2]
    if nq == 65 and k == 100:       # (33 localised queries x 154 planted rows would not fit the corpus)
        nq = 33
    out = []
    for metric in (SCAN_COSINE, SCAN_L2):
        forms = [f for f in dl.FORMS[cls] if dl.form_applies(cls, f, dim, metric)]
        l2_acc = dl.L2_ACCS[idx % len(dl.L2_ACCS)] if metric == SCAN_L2 and cls != "F" else 0
        d = dl.fixed_draw(cls, forms[0], metric, dim, n=[4097, 4223, 4352][idx % 3] if dim < 2048 else 4097, nq=nq, k=k,
                          seed=1000 + dim, offset=dl.B_OFFSETS[idx % 3], l2_acc=l2_acc, g0=idx)
        out.append((metric, forms, l2_acc, limit, d))
    return out


def masked_draws():
    """Class D under a dense allow-mask that still meets the filter (>= 16384 admitted rows of 21 000): (draw, forms)."""
    return [(dl.fixed_draw("D", "default", metric, dim, n=21_000, nq=17, k=10, seed=3000 + dim, mask=True, mask_keep=0.84), ["default", "split"])
            for dim, metric in ((112, SCAN_COSINE), (48, SCAN_L2), (1040, SCAN_COSINE))]


def filter_pass_draws():
    """Class F at 16 700 rows.  Up to 8192 rows every tile of a shard is a SAMPLE tile, and the int8 tier's sample pass keeps
    group maxima only — i8_collect_sample_kernel re-derives the scores of the listed rows — so the half-tile kernel's k loop
    cannot change an answer there (a mutant of its last-slab body passed every 4096 .. 5001-row case).  From 16384 rows on
    every second tile is a FILTER tile, whose survivors come from that loop: odd and even slab counts, with and without the
    resident maximum below them.  (draw, forms)"""
    out = []
    for dim in (320, 448, 832, 1088):
        forms = ["plain", "rotated"]
        out.append((dl.fixed_draw("F", "plain", SCAN_COSINE, dim, n=16_700, nq=17, k=10, seed=5000 + dim, g0=dim // 64), forms))
    return out


def planner_draws():
    """The row counts at which padding groups of a ragged last sample tile made the plan's threshold -inf (make_plan), and the
    first count past them: (draw, forms)."""
    return [(dl.fixed_draw("E", "default", SCAN_COSINE, 64, n=n, nq=17, k=k, seed=4000 + n), ["default", "wide", "bare"])
            for n in (4097, 4112, 4223, 4351, 4352) for k in (1, 10)]


def self_test(o):
    """compare_query() must let the oracle's own answer pass and report each mutation; returns the list of failures."""
    fails = []
    rng = np.random.default_rng(17)
    n, dim, k = 600, 36, 20
    corpus = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    corpus[40:46] = q * np.float32(0.5)                          # six rows of one score: the tie rank decides among them
    tie = rng.permutation(n).astype(np.uint64)
    rows, sims, _, _ = o.scan_cosine(corpus, q, k, -1.0, tie)
    lr, ld, ls = o.scan_l2(corpus, q, k, -1.0, None)

    def cmp(count, r, s, dd, exp, metric):
        return dl.compare_query(0, count, r, s, dd, exp, k, metric)

    def expect(name, msg, must_report=True):
        if (msg is not None) != must_report:
            fails.append("%s: %s" % (name, "not reported" if must_report else msg))
    dist = (np.float32(1.0) - sims).astype(np.float32)
    expect("the oracle's own answer", cmp(k, rows, sims, dist, (rows, sims, None), SCAN_COSINE), must_report=False)
    expect("the oracle's own L2 answer", cmp(k, lr, ls, ld, (lr, ls, ld), SCAN_L2), must_report=False)
    i = next(i for i in range(k - 1) if sims[i] == sims[i + 1])
    r2 = rows.copy(); r2[[i, i + 1]] = r2[[i + 1, i]]
    expect("a row swapped inside a tie", cmp(k, r2, sims, dist, (rows, sims, None), SCAN_COSINE))
    s3 = sims.copy(); s3.view(np.uint32)[k - 1] ^= 1
    expect("one score bit", cmp(k, rows, s3, dist, (rows, sims, None), SCAN_COSINE))
    r4, s4, d4 = rows.copy(), sims.copy(), dist.copy()
    r4[k - 1] = -1; s4[k - 1] = -np.inf; d4[k - 1] = np.inf
    expect("a count off by one", cmp(k - 1, r4, s4, d4, (rows, sims, None), SCAN_COSINE))
    short = (rows[:k - 2], sims[:k - 2], None)
    r5, s5, d5 = r4.copy(), s4.copy(), d4.copy()
    r5[k - 2] = -1; s5[k - 2] = -np.inf; d5[k - 2] = np.inf
    expect("a short answer, right padding", cmp(k - 2, r5, s5, d5, short, SCAN_COSINE), must_report=False)
    r6 = r5.copy(); r6[k - 1] = 0
    expect("padding not -1", cmp(k - 2, r6, s5, d5, short, SCAN_COSINE))
    d7 = ld.copy(); d7.view(np.uint32)[3] ^= 1
    expect("a distance bit", cmp(k, lr, ls, d7, (lr, ls, ld), SCAN_L2))
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
    counters, queries, picked, cell_list, t0 = {}, 0, 0, dl.cells(), time.time()
    try:
        for i in range(cases):
            d = dl.draw_case(rng, i, cell_list)
            msg, info = check_case(o, d, acc, 8, counters, rng)
            if on_case is not None:
                on_case(d, msg, info)
            if msg is not None:
                return {"failed": {"case": i, "difference": msg, "draw": d, "info": info}, "cases_passed": i}
            queries += d["nq"]; picked += info["picked"]
    finally:
        if acc is not None:
            acc.close()
    return {"cases": cases, "queries": queries, "oracle_queries": picked, "mismatches": 0, "seed": seed, "dry_run": dry_run,
            "counters": dict(sorted(counters.items())), "seconds": round(time.time() - t0, 1)}


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
