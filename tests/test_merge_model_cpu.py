"""tests/_merge_model.py gets its authority here, without a GPU: the model applied to the ORACLE's per-shard results must
equal the oracle over the whole, unsplit corpus — rows, order, score bits, distance bits and counts — for
Oracle.scan_cosine and Oracle.scan_l2 (both pinned on reference-compiled code: tests/test_scan_ref_pin.py,
tests/test_scan_ref_l2_pin.py), over contiguous and striped splits, planted cross-shard duplicates, with and without a
corpus-wide chunk-id ranking (each shard searching under a local rank table that preserves the global order, exactly as
vs_corpus_set_tie_ranks builds it), a range of thresholds, and global row ids with a base.  A tuple sort written out in
plain Python covers what no search produces (the records' own ranks, one row id in two shards), the Python merge
tests/_dist_worker.py falls back to is held to the model, and the two stress harnesses' generators must reach every path
they name for the seeds the GPU suite replays (--dry-run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _merge_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _split(n, n_shards, layout, rng):
    """Global row ordinals of each shard, ascending."""
    if layout == "contiguous":
        cuts = np.sort(rng.choice(np.arange(1, n), n_shards - 1, replace=False)) if n_shards > 1 else np.zeros(0, np.int64)
        if n_shards > 1 and rng.random() < 0.5:
            cuts[0] = 1                                             # a shard of one row: fewer rows than k
        b = [0, *cuts.tolist(), n]
        return [np.arange(b[i], b[i + 1]) for i in range(n_shards)]
    stripe = int(rng.choice([7, 16, 50]))
    t = np.arange(n) // stripe
    return [np.flatnonzero(t % n_shards == i) for i in range(n_shards)]


def _local_rank(rank, glob):
    """A permutation of 0..n_local-1 that preserves the global order (vs_corpus_set_tie_ranks)."""
    order = np.argsort(rank[glob], kind="stable")
    local = np.empty(len(glob), np.uint64); local[order] = np.arange(len(glob), dtype=np.uint64)
    return local


def _shard_lists(oracle, corpus, parts, queries, k, metric, thr, rank, base, own_ranks):
    """What each shard's search emits: its oracle result in global row ids, laid out as yams_scan_topk_device writes it."""
    nq = queries.shape[0]
    shards = []
    for glob in parts:
        sh = {"scores": np.full((nq, k), np.inf, np.float32), "rows": np.full((nq, k), base, np.int64),      # decoys behind the counts
              "counts": np.zeros(nq, np.uint32)}
        if metric == mm.L2:
            sh["dist"] = np.full((nq, k), -np.inf, np.float32)
        if own_ranks:
            sh["ranks"] = np.zeros((nq, k), np.uint32)
        local = _local_rank(rank, glob) if rank is not None else None
        part = np.ascontiguousarray(corpus[glob])
        for qi in range(nq):
            if len(glob) == 0:
                continue
            if metric == mm.COSINE:
                r, s, _, _ = oracle.scan_cosine(part, queries[qi], k, thr, local)
            else:
                r, d, s = oracle.scan_l2(part, queries[qi], k, -2.0, local)      # the threshold is deferred to the merge
                sh["dist"][qi, :len(r)] = d
            c = len(r)
            sh["scores"][qi, :c] = s; sh["rows"][qi, :c] = glob[r] + base; sh["counts"][qi] = c
            if own_ranks:
                sh["ranks"][qi, :c] = rank[glob[r]] if rank is not None else glob[r]
        shards.append(sh)
    return shards


def _whole(oracle, corpus, queries, k, metric, thr, rank, base):
    nq = queries.shape[0]
    S = np.full((nq, k), -np.inf, np.float32); R = np.full((nq, k), -1, np.int64); D = np.full((nq, k), np.inf, np.float32)
    Cn = np.zeros(nq, np.uint32)
    tr = rank.astype(np.uint64) if rank is not None else None
    for qi in range(nq):
        if metric == mm.COSINE:
            r, s, _, _ = oracle.scan_cosine(corpus, queries[qi], k, thr, tr)
            d = (np.float32(1.0) - s).astype(np.float32)
        else:
            r, d, s = oracle.scan_l2(corpus, queries[qi], k, thr, tr)
        c = len(r)
        S[qi, :c] = s; R[qi, :c] = r + base; D[qi, :c] = d; Cn[qi] = c
    return S, R, Cn, D


def _same(got, want, what):
    for g, w, name in zip(got, want, ("scores", "rows", "counts", "dist")):
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("metric", [mm.COSINE, mm.L2])
@pytest.mark.parametrize("layout", ["contiguous", "striped"])
@pytest.mark.parametrize("ranking", ["none", "rank_of_row", "own_ranks"])
def test_model_over_the_oracles_shard_results_equals_the_oracle_over_the_whole_corpus(oracle, metric, layout, ranking):
    rng = np.random.default_rng(1000 + 100 * metric + 10 * (layout == "striped") + len(ranking))
    short_lists = cuts_inside = 0
    for case in range(12):
        n, d = int(rng.integers(60, 900)), int(rng.choice([4, 8, 24]))
        n_shards = int(rng.integers(1, 7))
        k = int(rng.choice([1, 3, 10, 40, 100]))
        nq = int(rng.integers(1, 6))
        if case % 3 == 0:                                            # shards with fewer rows than k: short lists under either metric
            n, n_shards, k = int(rng.integers(8, 20)), int(rng.integers(2, 7)), int(rng.choice([10, 40]))
        corpus = rng.standard_normal((n, d)).astype(np.float32)
        for _ in range(int(rng.integers(2, 8))):                     # duplicates, far apart: most land in different shards
            src = int(rng.integers(0, n))
            corpus[rng.choice(n, int(rng.integers(1, 6)), replace=False)] = corpus[src]
        queries = rng.standard_normal((nq, d)).astype(np.float32)
        queries[0] = corpus[int(rng.integers(0, n))] * np.float32(1.5)
        parts = _split(n, n_shards, layout, rng)
        rank = rng.permutation(n).astype(np.uint32) if ranking != "none" else None
        base = int(rng.choice([0, 0, 1000, 1 << 33]))
        if metric == mm.COSINE:
            thr = float(rng.choice([-1.0, 0.0, 0.2, 0.5, 0.9]))
        else:
            thr = float(rng.choice([-1.0, 0.0, 0.1, 0.3, 2.0]))
        own = ranking == "own_ranks"
        shards = _shard_lists(oracle, corpus, parts, queries, k, metric, thr, rank, base, own)
        table = None
        if ranking == "rank_of_row":
            table = rank
        got = mm.merge(shards, k, metric, thr, rank_of_row=table, rank_row_base=base)
        want = _whole(oracle, corpus, queries, k, metric, thr, rank, base)
        _same(got, want, (case, n, d, n_shards, k, thr, base))
        if metric == mm.L2:                                         # ... and with the threshold deferred: the k nearest, uncut
            got = mm.merge(shards, k, metric, thr, rank_of_row=table, rank_row_base=base, defer=True)
            _same(got, _whole(oracle, corpus, queries, k, metric, -2.0, rank, base), (case, "defer"))
            cuts_inside += int(((want[2] > 0) & (want[2] < got[2])).any())
        short_lists += int(any((sh["counts"] < k).any() for sh in shards))
    assert short_lists >= 3, short_lists
    if metric == mm.L2:
        assert cuts_inside >= 2, cuts_inside


def _plain_merge_one_query(entries, k, metric, threshold, defer):
    """entries: (score, dist, rank, row, shard, position) of one query.  The contract as a tuple sort."""
    key = (lambda e: (float(e[1]), e[3], e[4], e[5])) if metric == mm.L2 else (lambda e: (-float(e[0]), e[2], e[3], e[4], e[5]))
    first = sorted(entries, key=key)[:k]
    if metric == mm.L2 and not defer:
        first = [e for e in first if not (e[0] < np.float32(threshold))]
    return first


@pytest.mark.parametrize("metric", [mm.COSINE, mm.L2])
def test_model_equals_a_tuple_sort_on_tie_heavy_records(metric):
    """Scores from a pool of a few values (±0.0, a denormal, neighbours one ulp apart), the records' own ranks, rank_of_row
    with a base, all ranks equal, one row id in two shards, short and empty lists."""
    rng = np.random.default_rng(77 + metric)
    one = np.float32(1.0)
    pool = np.array([0.0, -0.0, 1e-40, 1.0, np.nextafter(one, np.float32(0)), -1.0, 0.5, np.nextafter(np.float32(0.5), one)], np.float32)
    for case in range(150):
        n_shards, k, nq = int(rng.integers(1, 6)), int(rng.integers(1, 9)), int(rng.integers(1, 5))
        base = int(rng.choice([0, 5, 1 << 34]))
        m = n_shards * k * nq + 3
        source = ["none", "own", "table", "equal"][case % 4]
        table = rng.permutation(m).astype(np.uint32) if source != "equal" else np.full(m, 9, np.uint32)
        ids = rng.permutation(m)[:n_shards * k * nq].reshape(n_shards, nq, k)
        if n_shards > 1 and case % 3 == 0:
            ids[1, 0, 0] = ids[0, 0, 0]                              # the same row id in two shards
        shards, entries = [], [[] for _ in range(nq)]
        for s in range(n_shards):
            sh = {"scores": rng.choice(pool, (nq, k)), "rows": ids[s] + base, "counts": rng.integers(0, k + 1, nq).astype(np.uint32),
                  "dist": np.abs(rng.choice(pool, (nq, k)))}
            if source == "own":
                sh["ranks"] = rng.integers(0, 4, (nq, k)).astype(np.uint32)
            for qi in range(nq):
                for i in range(int(sh["counts"][qi])):
                    rk = int(sh["ranks"][qi, i]) if source == "own" else (int(table[ids[s, qi, i]]) if source in ("table", "equal") else 0)
                    entries[qi].append((sh["scores"][qi, i], sh["dist"][qi, i], rk, int(sh["rows"][qi, i]), s, i))
            shards.append(sh)
        thr, defer = float(rng.choice(pool)), bool(rng.integers(0, 2))
        S, R, Cn, D = mm.merge(shards, k, metric, thr, rank_of_row=table if source in ("table", "equal") else None,
                               rank_row_base=base, defer=defer)
        for qi in range(nq):
            want = _plain_merge_one_query(entries[qi], k, metric, thr, defer)
            c = len(want)
            assert Cn[qi] == c, (case, qi)
            assert R[qi, :c].tolist() == [e[3] for e in want], (case, qi, source)
            assert S[qi, :c].view(np.uint32).tolist() == [int(np.float32(e[0]).view(np.uint32)) for e in want], (case, qi)
            assert D[qi, :c].view(np.uint32).tolist() == [int(np.float32(e[1]).view(np.uint32)) for e in want], (case, qi)
            assert np.isneginf(S[qi, c:]).all() and (R[qi, c:] == -1).all() and np.isposinf(D[qi, c:]).all()


def test_model_writes_one_minus_score_when_the_shards_carry_no_distances():
    sh = {"scores": np.array([[0.75, 0.25, np.inf]], np.float32), "rows": np.array([[4, 9, 4]], np.int64), "counts": np.array([2], np.uint32)}
    S, R, Cn, D = mm.merge([sh], 3, mm.COSINE, threshold=0.5)       # (the cosine threshold plays no part in the merge)
    assert Cn.tolist() == [2] and R.tolist() == [[4, 9, -1]]
    assert D[0, :2].tolist() == [0.25, 0.75] and np.isposinf(D[0, 2]) and np.isneginf(S[0, 2])
    with pytest.raises(ValueError):
        mm.merge([sh], 3, mm.L2)


def test_python_merge_of_the_dist_worker_equals_the_model():
    from _dist_fallback import python_merge
    rng = np.random.default_rng(5)
    pool = np.array([0.0, -0.0, 0.5, 1.0, -1.0, 0.25], np.float32)
    for case in range(60):
        world, nq, k = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(1, 12))
        scores = rng.choice(pool, (world, nq, k)) if case % 2 else rng.standard_normal((world, nq, k)).astype(np.float32)
        rows = rng.permutation(world * nq * k).reshape(world, nq, k).astype(np.int64)
        counts = rng.integers(0, k + 1, (world, nq)).astype(np.uint32)
        for s in range(world):                                       # each list sorted as a shard's search emits it
            for qi in range(nq):
                c = int(counts[s, qi])
                o = np.lexsort((rows[s, qi, :c], -scores[s, qi, :c]))
                scores[s, qi, :c] = scores[s, qi, :c][o]; rows[s, qi, :c] = rows[s, qi, :c][o]
        out = {"scores": np.full((nq, k), -np.inf, np.float32), "rows": np.full((nq, k), -1, np.int64), "counts": np.zeros(nq, np.uint32)}
        python_merge({"scores": scores, "rows": rows, "counts": counts}, out, world, nq, k)
        S, R, Cn, _ = mm.merge([{"scores": scores[s], "rows": rows[s], "counts": counts[s]} for s in range(world)], k, mm.COSINE)
        assert np.array_equal(out["counts"], Cn) and np.array_equal(out["rows"], R), case
        # (the fallback rebuilds a score as -(-s): +0.0 and -0.0 are one value to it, as to the comparator)
        assert np.array_equal(out["scores"], S) and not np.isnan(S).any(), case


def _dry_run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), "--dry-run", *args], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(lines[-1])


def test_merge_harness_generator_reaches_every_path_for_the_pinned_seed():
    import test_merge_gpu as t
    res = _dry_run("stress_merge.py", "--cases", str(t.MERGE_CASES), "--seed", str(t.MERGE_SEED))
    assert res["mode"] == "dry-run"
    t.check_merge_summary(res)


def test_sharded_harness_generator_reaches_every_path_for_the_pinned_seed():
    import test_merge_gpu as t
    res = _dry_run("stress_sharded.py", "--cases", str(t.SHARDED_CASES), "--seed", str(t.SHARDED_SEED))
    assert res["mode"] == "dry-run"
    t.check_sharded_summary(res)
