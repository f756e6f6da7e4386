"""Every _host twin of a flat entry against its _device twin, through the Accel wrappers (which hold both to "64 guard bytes
behind each output come back untouched" and "a refused call wrote nothing").  One table, three runs per twin at a handful of
rows: (a) one list empty, every optional input absent; (b) every optional input and output present; (c) one refusal, where the
family has one that only shows after staging (an index equal to n, a non-finite row), else the host twin's own first verdict.
What the values ARE is each family's own test file's business (test_artifacts_gpu, test_features_gpu, ...): the device
twins are held to the oracles there, and (a) and (b) hold the host twins to the device twins bit for bit here.  The slices
of yams_cluster_residuals_host are the table's two residual rows (lists and every-cluster): both run the slice loop."""
import numpy as np
import pytest

from yams_amd import _lib

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = _lib.YAMS_ERR_INVALID_ARG, _lib.YAMS_ERR_UNSUPPORTED
FUSED = _lib.RESIDUAL_FUSED
NONE = 0xffffffff

_rng = np.random.default_rng(20261021)
ROWS = _rng.standard_normal((5, 3)).astype(np.float32)                  # 5 rows of dim 3
NAN_ROWS = ROWS.copy(); NAN_ROWS[3, 1] = np.nan
CENT = _rng.standard_normal((3, 3)).astype(np.float32)                  # 3 clusters
OFF = np.array([0, 2, 2, 5], np.uint64)                                 # three lists, the middle one empty
FULL_OFF = np.array([0, 2, 3, 5], np.uint64)
LIST = np.array([4, 0, 1, 3, 2], np.uint32)                             # row indices
LIST_N = np.array([4, 0, 5, 3, 2], np.uint32)                           # ... one equal to n
DOC_OFF = np.array([0, 2, 2, 3, 3, 5], np.uint64)                       # cluster indices of 5 documents, two lists empty
CAND = np.array([2, 0, 1, 0, 2], np.uint32)
CAND_C = np.array([2, 0, 3, 0, 2], np.uint32)                           # ... one equal to n_clusters
PRIMARY = np.array([0, NONE, 2, 1, 0], np.uint32)
QUERY = _rng.standard_normal((2, 3)).astype(np.float32)                 # 2 query tokens
DOCS = np.array([0, 5, 5], np.uint64)                                   # 2 documents, the second empty
HIDDEN = _rng.standard_normal((2, 3, 3)).astype(np.float32)             # batch 2, seq 3
MASK = np.array([[1, 0, 1], [0, 1, 1]], np.int32)
ROUTE = dict(vectors=ROWS, cluster_offsets=[0, 3, 5], has_centroid=[1, 0], position=[0, 0, 1, 0, 1])      # 2 clusters
COLS = np.array([1, 4, 0, 3, 2], np.uint32)                             # the CSR graph OFF + two empty rows
SGC_OFF = np.array([0, 2, 2, 5, 5, 5], np.uint64)
SGC_W = np.array([0.5, 1.0, 0.25, 2.0, 1.5], np.float32)


def _route(acc, host, **kw):
    ix = acc.route_index(**ROUTE)
    try:
        return acc.route_dense(ix, host_entry=host, **kw)
    finally:
        ix.close()


# name -> (a, b, (c, status)): each a callable (acc, host_entry) -> the wrapper's result
TWINS = {
    "cluster_centroids": (
        lambda acc, h: acc.cluster_centroids(ROWS, OFF, LIST, host_entry=h),
        lambda acc, h: acc.cluster_centroids(ROWS, FULL_OFF, LIST, host_entry=h),      # (no optional input: no list empty)
        (lambda acc, h: acc.cluster_centroids(ROWS, OFF, LIST_N, host_entry=h), INVALID)),
    "cluster_representatives": (
        lambda acc, h: acc.cluster_representatives(ROWS, OFF, LIST, CENT, 2, host_entry=h),
        lambda acc, h: acc.cluster_representatives(ROWS, OFF, LIST, CENT, 2, centroid_empty=[0, 1, 0], host_entry=h),
        (lambda acc, h: acc.cluster_representatives(NAN_ROWS, OFF, LIST, CENT, 2, host_entry=h), INVALID)),
    "cluster_residuals (lists)": (
        lambda acc, h: acc.cluster_residuals(ROWS, CENT, None, DOC_OFF, CAND, host_entry=h),
        lambda acc, h: acc.cluster_residuals(ROWS, CENT, PRIMARY, DOC_OFF, CAND, form=FUSED, host_entry=h),
        (lambda acc, h: acc.cluster_residuals(ROWS, CENT, PRIMARY, DOC_OFF, CAND_C, host_entry=h), INVALID)),
    "cluster_residuals (every cluster)": (
        lambda acc, h: acc.cluster_residuals(ROWS, CENT, host_entry=h),
        lambda acc, h: acc.cluster_residuals(ROWS, CENT, PRIMARY, form=FUSED, host_entry=h),
        (lambda acc, h: acc.cluster_residuals(ROWS, CENT, np.array([0, NONE, 3, 1, 0], np.uint32), host_entry=h), INVALID)),
    "features_aggregate": (
        lambda acc, h: acc.features_aggregate(ROWS, OFF, LIST, host_entry=h),
        lambda acc, h: acc.features_aggregate(ROWS, FULL_OFF, LIST, host_entry=h),
        (lambda acc, h: acc.features_aggregate(ROWS, OFF, LIST_N, host_entry=h), INVALID)),
    "features_variance": (
        lambda acc, h: acc.features_variance(ROWS, host_entry=h),
        lambda acc, h: acc.features_variance(ROWS, select=[4, 1, 1, 0], form=FUSED, host_entry=h),
        (lambda acc, h: acc.features_variance(ROWS, select=[4, 5, 1], host_entry=h), INVALID)),      # the host twin judges first
    "features_compose": (
        lambda acc, h: acc.features_compose(ROWS, host_entry=h),
        lambda acc, h: acc.features_compose(ROWS, weights=[1.0, 0.0, 0.5], entity=ROWS[:, :2], entity_on=[1, 0, 1, 1, 0],
                                            sig=(np.arange(20).reshape(5, 4) * 37 % 101).astype(np.uint32), sketch_on=[0, 1, 1, 0, 1],
                                            sketch_dim=4, alpha_e=0.5, alpha_m=0.25, host_entry=h),
        (lambda acc, h: acc.features_compose(ROWS, out_stride=2, host_entry=h), INVALID)),      # (no refusal needs the arrays)
    "rerank_maxsim": (
        lambda acc, h: acc.rerank_maxsim(QUERY, ROWS, DOCS, host_entry=h),
        lambda acc, h: acc.rerank_maxsim(QUERY, ROWS, DOCS, form=FUSED, want_rowmax=True, host_entry=h),
        (lambda acc, h: acc.rerank_maxsim(QUERY, ROWS, [0, 5, 3], host_entry=h), INVALID)),
    "rerank_maxpool": (
        lambda acc, h: acc.rerank_maxpool(ROWS, DOCS, host_entry=h),
        lambda acc, h: acc.rerank_maxpool(ROWS, [0, 2, 5], host_entry=h),
        (lambda acc, h: acc.rerank_maxpool(ROWS, [0, 5, 3], host_entry=h), INVALID)),
    "embed_pool": (
        lambda acc, h: acc.embed_pool(HIDDEN, None, _lib.EMBED_POOL_MAX, normalize=False, host_entry=h),
        lambda acc, h: acc.embed_pool(HIDDEN, MASK, _lib.EMBED_POOL_MEAN, normalize=True, host_entry=h),
        (lambda acc, h: acc.embed_pool(HIDDEN, MASK * 2, _lib.EMBED_POOL_MEAN, host_entry=h), UNSUPPORTED)),
    "embed_pool (CLS: the strided upload)": (
        lambda acc, h: acc.embed_pool(HIDDEN, None, _lib.EMBED_POOL_CLS, normalize=False, host_entry=h),
        lambda acc, h: acc.embed_pool(HIDDEN, MASK, _lib.EMBED_POOL_CLS, normalize=True, host_entry=h),
        None),
    "embed_normalize": (
        lambda acc, h: acc.embed_normalize(ROWS, host_entry=h),
        lambda acc, h: acc.embed_normalize(ROWS[:2], host_entry=h),
        (lambda acc, h: acc.embed_normalize(np.ones((1, _lib.EMBED_MAX_DIM + 1), np.float32), host_entry=h), UNSUPPORTED)),
    "route_dense": (
        lambda acc, h: _route(acc, h, queries=QUERY),
        lambda acc, h: _route(acc, h, queries=QUERY, rep_limit=2, candidates=[[1, 0], [1, 1]]),
        (lambda acc, h: _route(acc, h, queries=np.ones((1025, 3), np.float32)), INVALID)),      # (no refusal needs the arrays)
    "cluster_kmeans": (
        lambda acc, h: acc.cluster_kmeans(ROWS, host_entry=h),
        lambda acc, h: acc.cluster_kmeans(ROWS, k=3, max_iterations=4, host_entry=h),
        (lambda acc, h: acc.cluster_kmeans(NAN_ROWS, host_entry=h), INVALID)),
    "semantic_neighbors": (
        lambda acc, h: acc.semantic_neighbors(ROWS, 2, host_entry=h),
        lambda acc, h: acc.semantic_neighbors(ROWS, 2, tie_rank=[3, 0, 4, 1, 2], source_rows=[4, 0, 4], threshold=-0.5, host_entry=h),
        (lambda acc, h: acc.semantic_neighbors(ROWS, 2, source_rows=[4, 5], host_entry=h), INVALID)),
    "sgc_smooth": (
        lambda acc, h: acc.sgc_smooth(ROWS, SGC_OFF, COLS, SGC_W, 1, host_entry=h),
        lambda acc, h: acc.sgc_smooth(ROWS, SGC_OFF, COLS, SGC_W, 3, host_entry=h),
        (lambda acc, h: acc.sgc_smooth(ROWS, SGC_OFF, np.array([1, 4, 0, 5, 2], np.uint32), SGC_W, 2, host_entry=h), INVALID)),
    "persistence_h0": (
        lambda acc, h: acc.persistence_h0(ROWS, host_entry=h),
        lambda acc, h: acc.persistence_h0(ROWS, select=[4, 1, 0, 2], form=FUSED, want_distances=True, want_weights=True, host_entry=h),
        (lambda acc, h: acc.persistence_h0(ROWS, select=[4, 5, 1], host_entry=h), INVALID)),      # the host twin judges first
}


def _same(a, b, where):
    """Bit for bit: arrays by their bytes (a NaN equals itself), containers item by item, the rest by ==."""
    if isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, where
        assert a.tobytes() == b.tobytes(), (where, a, b)
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            _same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), (where, a, b)
    else:
        assert a == b, (where, a, b)


@pytest.mark.parametrize("name", list(TWINS))
def test_a_host_twin_equals_its_device_twin_and_refuses_alike(acc, name):
    bare, full, refusal = TWINS[name]
    _same(bare(acc, True), bare(acc, False), f"{name} (a)")
    _same(full(acc, True), full(acc, False), f"{name} (b)")
    if refusal is None:
        return
    call, status = refusal
    for host in (False, True):      # (the wrapper asserts that every output byte of the refused call is still the guard pattern)
        with pytest.raises(_lib.AccelError) as e:
            call(acc, host)
        assert e.value.status == status, (name, host, str(e.value))
    _same(bare(acc, True), bare(acc, False), f"{name} after a refusal")      # the context serves on
