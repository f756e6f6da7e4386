"""The cluster router's dense signal on the GPU (yams_route_index_* / yams_route_dense_*, _device and _host) against the
restatement of tests/_route_oracle.py.  Every comparison is on bits; the only tolerance is that a NaN matches any NaN.  Every
output is followed by guard bytes that the wrapper checks, also after a refusal."""
import numpy as np
import pytest

import _route_oracle as ro

pytestmark = pytest.mark.gpu
F32 = np.float32
# segments of 1 + R rows with R in {0, 1, 63, 64} (and clusters without a centroid, and empty ones), mixed so that segments
# straddle the 64-lane, 128-row and 256-row boundaries of the kernels
SIZES = [1, 2, 64, 65, 0, 64, 2, 65, 1, 63, 65, 64, 3]


def refused(call):
    from yams_amd._lib import AccelError, YAMS_ERR_INVALID_ARG
    with pytest.raises(AccelError) as e:
        call()
    assert e.value.status == YAMS_ERR_INVALID_ARG
    return True


def check(acc, index, table, queries, rep_limit=0, candidates=None, host=False, misalign=0):
    dense, obs, ev, diag = acc.route_dense(index, queries, rep_limit, candidates, host_entry=host, misalign=misalign)
    want = ro.dense_signal(table, queries, rep_limit, candidates)
    assert ro.same_bits(dense, want[0]), np.argwhere(~((ro.bits(dense) == ro.bits(want[0])) | (np.isnan(dense) & np.isnan(want[0]))))[:5]
    assert (obs == want[1]).all() and ev.tolist() == want[2].tolist()
    return diag


@pytest.fixture(scope="module")
def mixed():
    """One index of mixed segments at dim 33 with special values, its restatement computed once."""
    rng = np.random.default_rng(2024)
    table = ro.random_table(rng, 33, SIZES, special=True)
    queries = rng.standard_normal((129, 33)).astype(F32)
    queries[3] = 0.0
    queries[7, 5] = np.nan
    queries[11, 0] = np.inf
    queries[13] *= F32(1e-30)
    return table, queries


@pytest.mark.parametrize("dim", [1, 3, 4, 33, 64, 1024, 4096])
def test_dims_both_forms_and_entries(acc, dim):
    rng = np.random.default_rng(dim)
    table = ro.random_table(rng, dim, [1, 4, 0, 65, 2] if dim >= 1024 else SIZES)
    for misalign in (0, 4):
        index = acc.route_index(table.vectors, table.offsets, table.has_centroid, table.position, misalign=misalign)
        assert ro.same_bits(index.norms, table.norms)
        for nq in (1, 9):      # one lane per row / the fp64 tile
            q = rng.standard_normal((nq, dim)).astype(F32)
            diag = check(acc, index, table, q, misalign=misalign)
            assert diag["form"] == (0 if nq <= 8 else 1) and diag["pairs"] == nq * table.vectors.shape[0]
        index.close()
    index = acc.route_index(table.vectors, table.offsets, table.has_centroid, table.position, host_entry=True)
    assert ro.same_bits(index.norms, table.norms)
    check(acc, index, table, rng.standard_normal((5, dim)).astype(F32), host=True)
    assert index.info() == {"n_vectors": table.vectors.shape[0], "n_clusters": table.n_clusters, "dim": dim, "bytes": index.info()["bytes"]}
    index.close()


@pytest.mark.parametrize("nq", [1, 4, 5, 8, 9, 63, 64, 65, 129])
def test_query_counts_with_special_values(acc, mixed, nq):
    table, queries = mixed
    index = acc.route_index(table.vectors, table.offsets, table.has_centroid, table.position)
    # the slice that holds the zero, NaN, inf and tiny queries where it fits
    q = queries[:nq] if nq > 13 else queries[[3, 7, 11, 13, 0, 1, 2, 4][:nq]]
    check(acc, index, table, q)
    check(acc, index, table, q, host=(nq % 2 == 1))
    index.close()


@pytest.mark.parametrize("c", [1, 2, 257])
def test_cluster_counts_and_candidate_masks(acc, c):
    rng = np.random.default_rng(c)
    sizes = [int(rng.choice([1, 2, 5])) for _ in range(c)]
    table = ro.random_table(rng, 64, sizes)
    index = acc.route_index(table.vectors, table.offsets, table.has_centroid, table.position)
    for nq in (3, 11):
        q = rng.standard_normal((nq, 64)).astype(F32)
        none = np.zeros((nq, c), bool)
        dense, obs, ev, _ = acc.route_dense(index, q, candidates=none)
        assert not dense.view(np.uint32).any() and not obs.any() and not ev.any()      # 0.0F, unobserved, not counted
        one = none.copy()
        one[np.arange(nq), rng.integers(0, c, nq)] = True
        check(acc, index, table, q, candidates=one)
        check(acc, index, table, q, candidates=rng.random((nq, c)) < 0.5, host=True)
    index.close()


@pytest.mark.parametrize("nq", [2, 10])
def test_representative_limit_counts_positions(acc, nq):
    """rep_limit at 0, 1, R and R + 1 (R = 5 representatives), over positions with gaps: the limit counts places in the
    reference's list, not rows of the table."""
    rng = np.random.default_rng(77 + nq)
    table = ro.random_table(rng, 33, [6, 5, 6, 1, 6])
    index = acc.route_index(table.vectors, table.offsets, table.has_centroid, table.position)
    q = rng.standard_normal((nq, 33)).astype(F32)
    counts = []
    for limit in (0, 1, 2, 5, 6, int(table.position.max()) + 1, int(table.position.max()) + 2, 70000):
        check(acc, index, table, q, rep_limit=limit)
        counts.append(int(ro.dense_signal(table, q, limit)[2][0]))
    assert counts[1] < counts[2] <= counts[3] <= counts[4] and counts[-2] == counts[0] == counts[-1]     # the cases differ
    index.close()


@pytest.mark.parametrize("name", sorted(ro.GOLDEN_CASES))
def test_golden_special_values(acc, name):
    """Every golden case's table and query through _device and _host: dense, observed and the evaluation count."""
    case = ro.GOLDEN_CASES[name]
    query = case["request"]["query"]
    table = ro.table_of(case["clusters"], query.size)
    want = ro.route(case, ro.standin_ann(case))
    for host in (False, True):
        index = acc.route_index(table.vectors, table.offsets, table.has_centroid, table.position, host_entry=host)
        diag = check(acc, index, table, query[None, :], rep_limit=case["request"]["max_reps"], host=host)
        assert diag["form"] == 0
        check(acc, index, table, np.repeat(query[None, :], 9, axis=0), rep_limit=case["request"]["max_reps"], host=host)   # the tile form
        index.close()
    if not want["work"]["ann_used"] and F32(case["request"]["alpha"]) < 1:      # the whole route's counter is the device's
        assert ro.dense_signal(table, query[None, :], case["request"]["max_reps"])[2][0] == want["work"]["exact_evaluations"]


def test_refusals_at_each_limit_with_guards(acc):
    rng = np.random.default_rng(9)
    ok = ro.random_table(rng, 8, [3, 2])

    def create(vectors=ok.vectors, off=ok.offsets, has=ok.has_centroid, pos=ok.position, host=False):
        return acc.route_index(vectors, off, has, pos, host_entry=host)
    for host in (False, True):
        create(host=host).close()
        assert refused(lambda: create(vectors=np.zeros((5, 4097), F32), host=host))                       # dim beyond the limit
        create(vectors=np.zeros((5, 4096), F32), host=host).close()
        assert refused(lambda: create(off=[1, 3, 5], host=host))                                          # does not start at 0
        assert refused(lambda: create(off=[0, 4, 3], host=host))                                          # decreases
        assert refused(lambda: create(off=[0, 3, 4], host=host))                                          # does not end at n_vectors
        assert refused(lambda: create(off=[0, 5, 5], has=[1, 1], host=host))                              # a centroid flag on an empty segment
        assert refused(lambda: create(pos=[0, 0, 0xFFFF, 0, 0], host=host))                               # the reserved position
        # 64 representatives beside a centroid is the most; 65 are refused, as are 65 without a centroid
        big = ro.random_table(rng, 4, [65])
        create(big.vectors, big.offsets, [1], np.arange(65), host=host).close()
        assert refused(lambda: create(big.vectors, big.offsets, [0], np.arange(65), host=host))
        more = np.zeros((66, 4), F32)
        assert refused(lambda: create(more, [0, 66], [1], np.arange(66), host=host))
    # n_clusters at the limit, and one beyond (every cluster one row)
    c = 65536
    one = np.ones((c + 1, 1), F32)
    index = acc.route_index(one[:c], np.arange(c + 1), np.ones(c, np.uint8), np.zeros(c, np.uint16))
    assert refused(lambda: acc.route_index(one, np.arange(c + 2), np.ones(c + 1, np.uint8), np.zeros(c + 1, np.uint16)))
    index.close()
    # queries: 1024 are served, 1025 refused, outputs and guards untouched (the wrapper reads them back)
    index = create()
    q = rng.standard_normal((1025, 8)).astype(F32)
    for host in (False, True):
        check(acc, index, ok, q[:1024], host=host)
        assert refused(lambda: acc.route_dense(index, q, host_entry=host))
    assert acc.route_dense(index, np.zeros((0, 8), F32))[2].size == 0
    index.close()


def test_destroy_and_recreate_on_one_context(acc):
    rng = np.random.default_rng(31)
    for round_ in range(6):
        dim = [8, 33, 64][round_ % 3]
        table = ro.random_table(rng, dim, [int(x) for x in rng.integers(0, 9, 20 + round_)], special=round_ % 2 == 1)
        a = acc.route_index(table.vectors, table.offsets, table.has_centroid, table.position, host_entry=round_ % 2 == 0)
        b = acc.route_index(np.zeros((0, dim), F32), [0, 0], [0], [])      # an empty index lives beside it
        q = rng.standard_normal((1 + round_ * 3, dim)).astype(F32)
        check(acc, a, table, q)
        dense, obs, ev, _ = acc.route_dense(b, q)
        assert dense.shape == (q.shape[0], 1) and not dense.view(np.uint32).any() and not obs.any() and not ev.any()
        a.close(); b.close()


def test_host_call_of_two_slices(acc):
    """65536 clusters x 1024 queries: 5 bytes of output per pair exceed the 256 MiB a _host call keeps on the device at a time,
    so the queries are served in two slices (and the (query, row) values of each in slices of their own).  dim 1: a cosine is
    +-1, dense 0.0 or 1.0 — the restatement is written out directly."""
    rng = np.random.default_rng(5)
    c, nq = 65536, 1024
    cent = np.where(rng.random(c) < 0.5, -1, 1).astype(F32) * rng.uniform(0.5, 2.0, c).astype(F32)
    cent[::97] = 0.0                                                   # zero-norm centroids: not evaluated
    q = np.where(rng.random(nq) < 0.5, -1, 1).astype(F32) * rng.uniform(0.5, 2.0, nq).astype(F32)
    q[5] = 0.0
    index = acc.route_index(cent[:, None], np.arange(c + 1), np.ones(c, np.uint8), np.zeros(c, np.uint16), host_entry=True)
    dense, obs, ev, diag = acc.route_dense(index, q[:, None], host_entry=True)
    index.close()
    want_obs = (q[:, None] != 0) & (cent[None, :] != 0)
    want = np.where(want_obs & (np.sign(q)[:, None] == np.sign(cent)[None, :]), F32(1.0), F32(0.0))
    small = ro.Table(cent[:300, None], np.arange(301), np.ones(300, np.uint8), np.zeros(300, np.uint16))
    assert ro.same_bits(ro.dense_signal(small, q[:40, None])[0], want[:40, :300])      # the shortcut is the restatement
    assert diag["slices"] >= 2 and diag["pairs"] == nq * c
    assert (obs == want_obs).all() and ro.same_bits(dense, want) and ev.tolist() == want_obs.sum(axis=1).tolist()


# ---- topology_route_v1 and the shell over it ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def route_vt():
    import ctypes as C
    from yams_amd import _lib
    L = _lib.load()
    assert L.yams_plugin_init(b'{"device": 0}', None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"topology_route_v1", 1, C.byref(p)) == 0
    yield C.cast(p, C.POINTER(_lib.TopologyRouteV1)).contents
    L.yams_plugin_shutdown()


def test_plugin_interface_serves_the_golden_special_values(route_vt):
    """index_create -> index_info -> dense -> index_destroy through topology_route_v1 for every golden case, two indexes alive
    at a time; a destroyed or unknown id is NOT_FOUND and writes nothing."""
    import ctypes as C
    from yams_amd import _lib
    from yams_amd.accel import pack_candidates
    vp = C.c_void_p

    def ptr(a):
        return a.ctypes.data_as(vp) if a.size else None
    previous = None
    for name in sorted(ro.GOLDEN_CASES):
        case = ro.GOLDEN_CASES[name]
        query = case["request"]["query"]
        table = ro.table_of(case["clusters"], query.size)
        v, c = table.vectors.shape[0], table.n_clusters
        norms = np.full(v + 16, 7.0, F32)
        ident = C.c_uint64(0)
        assert route_vt.index_create(None, ptr(table.vectors), v, table.dim, ptr(table.offsets), ptr(table.has_centroid), ptr(table.position), c,
                                     C.byref(ident), ptr(norms)) == 0
        assert ro.same_bits(norms[:v], table.norms) and (norms[v:] == 7.0).all()
        info = _lib.RouteIndexInfo()
        assert route_vt.index_info(None, ident.value, C.byref(info)) == 0 and (info.n_vectors, info.n_clusters, info.dim) == (v, c, table.dim)
        whole = ro.route(case, ro.standin_ann(case))
        cand = np.array(whole["candidates"], bool)[None, :]
        bits = pack_candidates(cand)
        dense = np.full(c + 16, 7.0, F32); obs = np.full(c + 16, 7, np.uint8); ev = np.full(1 + 16, 7, np.uint32)
        assert route_vt.dense(None, ident.value, ptr(query), 1, case["request"]["max_reps"], ptr(bits), ptr(dense), ptr(obs), ptr(ev), None) == 0
        want = ro.dense_signal(table, query[None, :], case["request"]["max_reps"], cand)
        assert ro.same_bits(dense[:c], want[0][0]) and (obs[:c] == want[1][0]).all() and ev[0] == want[2][0], name
        assert (dense[c:] == 7.0).all() and (obs[c:] == 7).all() and (ev[1:] == 7).all()
        if np.float32(case["request"]["alpha"]) < 1:      # ... which is the whole route's dense signal
            assert ro.same_bits(dense[:c], whole["dense"]) and ev[0] == whole["work"]["exact_evaluations"], name
        if previous is not None:
            assert route_vt.index_destroy(None, previous) == 0
            assert route_vt.index_destroy(None, previous) == _lib.YAMS_ERR_NOT_FOUND
            assert route_vt.dense(None, previous, ptr(query), 1, 0, None, ptr(dense), ptr(obs), ptr(ev), None) == _lib.YAMS_ERR_NOT_FOUND
            assert (dense[c:] == 7.0).all() and ro.same_bits(dense[:c], want[0][0])
        previous = ident.value
    assert route_vt.index_destroy(None, previous) == 0


def test_shell_through_the_real_plugin_equals_the_golden_file():
    """include/yams_accel/topology_route.hpp over the real topology_route_v1 against what the reference's own functions returned
    (tests/golden/cluster_route.json), single routes and routeBatch."""
    import json
    import os
    import subprocess
    import tempfile
    from _route_build import build_shell_test
    from yams_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    golden = {c["name"]: c for c in json.load(open(os.path.join(root, "tests", "golden", "cluster_route.json")))["cases"]}
    exe = build_shell_test()
    names = sorted(ro.GOLDEN_CASES)
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, name + ".bin") for name in names]
        for name, path in zip(names, paths):
            ro.write_case(path, ro.GOLDEN_CASES[name])
        # every case in one process (one plugin, one shell, an index each), then two of them again through routeBatch
        r = subprocess.run([exe, *paths, "--plugin", _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-1500:])
        answers = r.stdout.split("case ")[1:]
        assert len(answers) == len(names)
        for name, text in zip(names, answers):
            got = ro.parse_driver(text)
            assert "error" not in got and ro.same_result(got, golden[name]), (name, got, golden[name])
        batch = ["plain", "candidate_mask_weighted_seeds"]
        r = subprocess.run([exe, *[paths[names.index(n)] for n in batch], "--batch", "--plugin", _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-1500:])
        for name, text in zip(batch, r.stdout.split("case ")[1:]):
            parts = text.split("request ")
            for k in (1, 3):      # (the middle request has another representative limit: tests/test_route_cpu.py holds it to the restatement)
                assert ro.same_result(ro.parse_driver(parts[0] + parts[k].split("\n", 1)[1]), golden[name]), (name, k)


def test_stress_harness():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "stress_route.py"), "--cases", "60"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "60 cases, 0 failures OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
