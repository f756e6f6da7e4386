"""A plain model of the shard-merge contract (include/yams_mi355x_accel.h, yams_scan_merge_topk_device /
yams_scan_merge_records_device): numpy only, no device code.  Test infrastructure.

Per query, the entries of every shard's list (the first counts[shard][query] slots; what lies behind them is never read)
are put into ONE order and the first k are kept:

  cosine   similarity descending under float compare (-0.0f == +0.0f); equal similarities by tie rank ascending — the
           records' own ranks if the records carry them, else rank_of_row[row - rank_row_base] if that table is given,
           else no rank at all —; then by row id ascending
  L2       distance ascending under float compare; then row id ascending.  Ranks of either kind are ignored (vec0's
           `ORDER BY distance`: tests/test_scan_ref_l2_pin.py)
  both     entries that are still equal (the same row id in two shards) keep the order of their element index:
           shard ascending, then position in the shard's list

Under L2 only, and only without the defer flag, entries of those first k whose similarity is < threshold are then dropped
("the k nearest, then the threshold"); the survivors keep their order.  Under cosine the threshold plays no part: each
shard has applied it already.  counts[query] is what is left; unused output slots hold -inf / -1 / +inf.  out_dist is the
input distance of the entry, or 1 - similarity (fp32) when the shards carry no distances.

Scores and distances are taken to be free of NaN (no search emits one).  tests/test_merge_model_cpu.py pins this model to
the oracle over the whole corpus; tests/stress_merge.py holds merge_topk_kernel to it.
"""
import numpy as np

COSINE, L2 = 0, 1


def merge(shards, k, metric=COSINE, threshold=-np.inf, rank_of_row=None, rank_row_base=0, defer=False):
    """shards: one dict per shard with "scores" f32 [nq][k], "rows" i64 [nq][k], "counts" u32 [nq] and optionally
    "dist" f32 [nq][k], "ranks" u32 [nq][k] (all shards carry the same parts).
    Returns (scores f32 [nq][k], rows i64 [nq][k], counts u32 [nq], dist f32 [nq][k])."""
    nq = len(shards[0]["counts"])
    has_dist, has_ranks = "dist" in shards[0], "ranks" in shards[0]
    if metric == L2 and not has_dist:
        raise ValueError("an L2 merge needs distances")
    # element e = shard * k + position, as the lists lie side by side
    score = np.concatenate([np.asarray(s["scores"], np.float32).reshape(nq, k) for s in shards], axis=1)
    row = np.concatenate([np.asarray(s["rows"], np.int64).reshape(nq, k) for s in shards], axis=1)
    live = np.concatenate([np.arange(k)[None, :] < np.asarray(s["counts"], np.int64)[:, None] for s in shards], axis=1)
    dist = np.concatenate([np.asarray(s["dist"], np.float32).reshape(nq, k) for s in shards], axis=1) if has_dist else None
    element = np.broadcast_to(np.arange(len(shards) * k), score.shape)

    rank = np.zeros(score.shape, np.int64)                      # "no rank at all": every entry equal
    if metric == COSINE:
        if has_ranks:
            rank = np.concatenate([np.asarray(s["ranks"], np.uint32).reshape(nq, k) for s in shards], axis=1).astype(np.int64)
        elif rank_of_row is not None:
            rank[live] = np.asarray(rank_of_row)[row[live] - rank_row_base]
    primary = dist if metric == L2 else -score                  # ascending either way; float compare: -0.0 == +0.0
    primary = np.where(live, primary, np.float32(0))            # (slots behind a count take no part)
    rank = np.where(live, rank, 0)
    # np.lexsort: the LAST key is the most significant one
    order = np.lexsort((element, np.where(live, row, 0), rank, primary, ~live), axis=-1)[:, :k]

    take = lambda a: np.take_along_axis(a, order, axis=1)
    keep = take(live)
    if metric == L2 and not defer:
        keep &= ~(take(score) < np.float32(threshold))
    counts = keep.sum(axis=1).astype(np.uint32)
    front = np.argsort(~keep, axis=1, kind="stable")            # survivors first, order preserved
    order = np.take_along_axis(order, front, axis=1)
    used = np.arange(k)[None, :] < counts[:, None]
    out_scores = np.where(used, take(score), np.float32(-np.inf)).astype(np.float32)
    out_rows = np.where(used, take(row), np.int64(-1))
    out_dist = take(dist) if has_dist else (np.float32(1.0) - take(score)).astype(np.float32)
    out_dist = np.where(used, out_dist, np.float32(np.inf)).astype(np.float32)
    return out_scores, out_rows, counts, out_dist
